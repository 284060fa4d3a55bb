// The kernel of the smoothing (volym_smooth_labels): the vote of a majority filter over a box of texels.  Included by smooth.hip
// alone.  The vote reads labels and density and writes NO label: for every chunk in which a texel changes
// it appends one record -- the chunk's index and its 16 bytes as they will be -- to the journal's staging area (journal_append) and
// tallies the change (tally_texel, tally_reduce).  volym_label_swap_kernel of relabel_kernels.h (relabel.hip launches it) applies the records afterwards.
// From edit_chunks.h: the one-owner rule (crop_chunk, relabel_owns_chunk, the keep mask), the tally and the journal.  Here: the
// unit a workgroup stages in LDS, in either layout, and the count.
#pragma once

#include "edit_chunks.h"

namespace volym {

// ---- the unit -----------------------------------------------------------------------------------------------------------------------
// A workgroup decides one UNIT per step: 256 dwords of positions, one per thread, of which the middle ones are owned (their chunks
// are this unit's items of the slab walk) and the ends are the halo along x.
//   linear:  a unit is up to 63 consecutive chunks of one run of the walk, bytes [a, a + 1008) of the layout, with 8 bytes of halo on
//            either side: position dword t holds bytes a - 8 + 4 t.  A texel's neighbour (dx, dy, dz) lies dx + nx dy + nx ny dz
//            bytes further in the FLAT layout wherever the texel sits, so chunks that wrap rows and slices (nx no multiple of 16)
//            need nothing special: only which neighbours exist depends on the texel's coordinates.
//   bricked: a unit is up to 14 consecutive bricks of one brick row of the walk (56 chunks) with one brick of halo on either side:
//            position dword t is row t & 3 of the 4 x 4 patch at z = t >> 2 & 3 of brick t >> 4, the x neighbours of a dword are the
//            dwords 16 further on either side.
// Row (dy, dz) of the unit, rows[(dz + rz) (2 ry + 1) + dy + ry][t], holds the four labels at (x .. x + 3, y + dy, z + dz) for
// position dword t at (x, y, z): one aligned dword load from the bricked layout, two and a byte shift from the linear one.  Never a
// byte load from global memory.
constexpr uint32_t SMOOTH_LINEAR_CHUNKS = 63u, SMOOTH_LINEAR_BASE = 2u;      // owned chunks of a unit and its first owned dword
constexpr uint32_t SMOOTH_BRICK_CHUNKS = 56u, SMOOTH_BRICK_BASE = 16u, SMOOTH_BRICKS = 14u;

// the request as the kernel reads it (all of it uniform) and the walk's units (smooth.hip counts them)
struct SmoothRule {
    uint32_t min_byte, max_byte;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t radius[3];
    uint32_t n_units, blocks;       // the units, and the blocks of 63 chunks per run (linear) or of 14 bricks per brick row (bricked)
    uint32_t alloc_dwords;          // linear: the dwords of the labels' allocation, ceil(n / 16) * 4
};
struct SmoothTables { uint8_t give[256], take[256]; };

template <uint32_t ROWS>
struct SmoothShared {
    uint32_t rows[ROWS][256];       // the staged labels
    uint32_t col[2][256];           // per position, the votes of the label in hand summed over y and z: a byte each (<= 49)
    uint32_t fresh[256];            // the owned dwords as they will be
    uint32_t set[8];                // the labels the unit holds, a bit each
    uint32_t keep[64];              // per owned chunk, the texels its owner decides (0: not this unit's)
    uint32_t any;                   // does any owner of the unit keep a texel?
    uint8_t give[256], take[256];
};

// What a position byte knows of its texel (x, y, z): how far its neighbourhood reaches on each side before it leaves the volume,
// two bits each -- y below, y above, z below, z above, then bit 8: it is a texel, then x below and x above (bits 9.., 11..).
__device__ __forceinline__ uint32_t smooth_reach(uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t r[3])
{
    return min(r[1], y) | (min(r[1], ny - 1u - y) << 2) | (min(r[2], z) << 4) | (min(r[2], nz - 1u - z) << 6) | 256u | (min(r[0], x) << 9) |
           (min(r[0], nx - 1u - x) << 11);
}

// does the texel of reach g have a neighbour in row (dy, dz)?
__device__ __forceinline__ bool smooth_row_has(uint32_t g, int dy, int dz)
{
    return (g & 256u) && dy >= -static_cast<int>(g & 3u) && dy <= static_cast<int>((g >> 2) & 3u) && dz >= -static_cast<int>((g >> 4) & 3u) &&
           dz <= static_cast<int>((g >> 6) & 3u);
}

// 0x01 in every byte of the position dword whose texel has a neighbour in row (dy, dz).  same: the four bytes share g[0]'s rows.
__device__ __forceinline__ uint32_t smooth_row_mask(const uint32_t g[4], bool same, int dy, int dz)
{
    if (same) return smooth_row_has(g[0], dy, dz) ? 0x01010101u : 0u;
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) m |= smooth_row_has(g[j], dy, dz) ? 1u << (8u * j) : 0u;
    return m;
}

// 0x01 in every byte of v that equals the byte mm is made of (mm = m * 0x01010101)
__device__ __forceinline__ uint32_t smooth_equal_bytes(uint32_t v, uint32_t mm)
{
    const uint32_t x = v ^ mm;
    return (~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;
}

// One pass over the units of slab s (make_crop_slab over the request's box, s.box_lo/hi the box itself, no plane), in either layout.
// Per unit: the owners' keep masks (a unit that keeps no texel is left before any load); the rows, staged by dword loads, and the set
// of labels they hold; a unit that holds ONE label is left before any counting (exact: the own label then has every vote); else per
// label of the set that gives or takes, ascending: the votes per position summed over the rows (four positions per dword, SWAR),
// then along x, and the running winner under the tie rule -- the own label wins a tie, else the smallest label; then window, tally,
// and the chunks that changed into the journal.  The neighbourhood is unconstrained: box, window and give act on the texel alone.
template <uint32_t ROWS>
__global__ __launch_bounds__(256) void volym_smooth_vote_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ vol, RelabelOut out,
                                                                SmoothTables tables, CropSlab s, SmoothRule rule, LabelJournal journal, uint32_t nx, uint32_t ny,
                                                                uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ SmoothShared<ROWS> ssh;
    const uint32_t t = threadIdx.x;
    sh.to[t] = static_cast<uint8_t>(t);                                  // (no table: the tally alone is used)
    ssh.give[t] = tables.give[t];
    ssh.take[t] = tables.take[t];
    tally_init(sh);
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t slice = nx * ny, bx = brick_count(nx), by = brick_count(ny);
    const int ry = static_cast<int>(rule.radius[1]), rz = static_cast<int>(rule.radius[2]);
    const uint32_t width = 2u * rule.radius[1] + 1u, centre = rule.radius[2] * width + rule.radius[1];
    const uint32_t base = bricked ? SMOOTH_BRICK_BASE : SMOOTH_LINEAR_BASE, chunks = bricked ? SMOOTH_BRICK_CHUNKS : SMOOTH_LINEAR_CHUNKS;
    const uint32_t xs = bricked ? 16u : 1u;
    const bool owned = t >= base && t < base + 4u * chunks;
    const bool windowed = rule.min_byte > 0u || rule.max_byte < 255u;   // (uniform)
    RelabelTally tl;

    for (uint32_t u = blockIdx.x; u < rule.n_units; u += gridDim.x) {
        __syncthreads();                                                 // the unit before has let go of the LDS (and the tables are there)
        if (t < 8u) ssh.set[t] = 0u;
        const uint32_t line = u / rule.blocks, block = u - line * rule.blocks;

        // the owners: lane c of wave 0 for chunk c of the unit, by the walk's own rule
        uint64_t k = 0;
        uint32_t keep = 0;
        if (t < chunks) {
            uint32_t i = 0, moved;
            bool have;
            if (bricked) {
                const uint32_t brick = block * SMOOTH_BRICKS + (t >> 2);
                have = brick < s.b_n[0];
                i = (line * s.b_n[0] + brick) * 4u + (t & 3u);
            } else {
                const uint32_t ci = block * SMOOTH_LINEAR_CHUNKS + t;
                have = ci < s.chunks_per_run;
                i = line * s.chunks_per_run + ci;
            }
            have = have && i < n_items && crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved);
            if (have && !bricked && !relabel_owns_chunk(s, i, nx, ny, k)) have = false;
            if (!have) keep = 0u;
        }
        if (t < 64u) {                                                   // (wave 0: the owners are all there)
            ssh.keep[t] = keep;
            const unsigned long long some = __ballot(keep != 0u);
            if (t == 0u) ssh.any = some != 0ull ? 1u : 0u;
        }
        __syncthreads();
        if (ssh.any == 0u) continue;                                     // (uniform) nothing to decide here: before any load

        // where this thread's position dword lies: its first texel, and the reach of each of its four bytes
        uint32_t g[4] = {0u, 0u, 0u, 0u};
        uint32_t x0 = 0, y0 = 0, z0 = 0;
        int64_t o = 0;                                                   // linear: the dword's first byte in the layout
        bool patch = false;                                              // bricked: the dword is a row of a patch of the volume
        if (bricked) {
            const uint32_t byi = s.b_lo[1] + line % s.b_n[1], bzi = s.b_lo[2] + line / s.b_n[1];
            const int32_t bxi = static_cast<int32_t>(s.b_lo[0] + block * SMOOTH_BRICKS + (t >> 4)) - 1;
            y0 = byi * 4u + (t & 3u); z0 = bzi * 4u + ((t >> 2) & 3u);
            patch = bxi >= 0 && static_cast<uint32_t>(bxi) < bx && y0 < ny && z0 < nz;
            if (patch) {
                x0 = static_cast<uint32_t>(bxi) * 4u;
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) if (x0 + j < nx) g[j] = smooth_reach(x0 + j, y0, z0, nx, ny, nz, rule.radius);
            }
        } else {
            const uint32_t rys = line % s.runs_y, rzs = line / s.runs_y;
            const uint64_t start = s.lo[0] + static_cast<uint64_t>(nx) * ((s.lo[1] + rys) + static_cast<uint64_t>(ny) * (s.lo[2] + rzs));
            o = static_cast<int64_t>(((start >> 4) + static_cast<uint64_t>(block) * SMOOTH_LINEAR_CHUNKS) * 16u) - 8 + 4 * static_cast<int64_t>(t);
            if (o >= 0 && static_cast<uint64_t>(o) < n) {
                const uint32_t ou = static_cast<uint32_t>(o);
                z0 = ou / slice; y0 = (ou - z0 * slice) / nx; x0 = ou - z0 * slice - y0 * nx;
                ChunkCursor c = {x0, y0, z0};
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    if (static_cast<uint64_t>(o) + j < n) g[j] = smooth_reach(c.x, c.y, c.z, nx, ny, nz, rule.radius);
                    c.next(0u, nx, ny);
                }
            }
        }
        const bool same = (g[0] & 256u) && ((g[0] ^ g[1]) & 0x1ffu) == 0u && ((g[0] ^ g[2]) & 0x1ffu) == 0u && ((g[0] ^ g[3]) & 0x1ffu) == 0u;

        // stage the rows and collect the labels they hold: a lane's run of one label costs it one LDS atomic
        uint32_t seen = 0x100u;                                          // (no label yet)
        uint32_t row = 0;
        for (int dz = -rz; dz <= rz; ++dz) {
            for (int dy = -ry; dy <= ry; ++dy, ++row) {
                uint32_t v = 0;
                if (bricked) {
                    const uint32_t y = y0 + static_cast<uint32_t>(dy), z = z0 + static_cast<uint32_t>(dz);    // (wraps below 0: >= ny, nz)
                    if (patch && y < ny && z < nz) v = labels[layout_offset(true, bx, bx * by, x0, y, z) >> 2];
                } else {
                    const int64_t at = o + static_cast<int64_t>(dy) * nx + static_cast<int64_t>(dz) * slice;
                    const int64_t q = at >> 2;
                    const uint32_t shift = 8u * static_cast<uint32_t>(at & 3);
                    const uint32_t lo = q >= 0 && q < static_cast<int64_t>(rule.alloc_dwords) ? labels[q] : 0u;
                    v = lo;
                    if (shift) {                                         // (uniform: the positions are dwords apart)
                        const uint32_t hi = q + 1 >= 0 && q + 1 < static_cast<int64_t>(rule.alloc_dwords) ? labels[q + 1] : 0u;
                        v = (lo >> shift) | (hi << (32u - shift));
                    }
                }
                ssh.rows[row][t] = v;
                const uint32_t mask = smooth_row_mask(g, same, dy, dz);
                if (mask == 0x01010101u && seen < 0x100u && v == seen * 0x01010101u) continue;
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t l = (v >> (8u * j)) & 0xffu;
                    if ((mask & (1u << (8u * j))) && l != seen) { atomicOr(&ssh.set[l >> 5], 1u << (l & 31u)); seen = l; }
                }
            }
        }
        __syncthreads();
        uint32_t present = 0;
#pragma unroll
        for (uint32_t w = 0; w < 8u; ++w) present += static_cast<uint32_t>(__popc(ssh.set[w]));
        if (present <= 1u) continue;                                     // (uniform) one label: every texel keeps it

        // the count, label by label
        const uint32_t mine = ssh.rows[centre][t];
        uint32_t own[4] = {0u, 0u, 0u, 0u}, best[4] = {0u, 0u, 0u, 0u}, best_label[4] = {0u, 0u, 0u, 0u};
        uint32_t parity = 0;
        for (uint32_t w = 0; w < 8u; ++w) {
            uint32_t bits = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(ssh.set[w])));
            while (bits) {                                               // (uniform)
                const uint32_t m = w * 32u + static_cast<uint32_t>(__ffs(static_cast<int>(bits))) - 1u;
                bits &= bits - 1u;
                const bool takes = ssh.take[m] != 0u;
                if (!takes && ssh.give[m] == 0u) continue;               // no candidate of any texel that may change
                const uint32_t mm = m * 0x01010101u;
                uint32_t acc = 0;
                row = 0;
                for (int dz = -rz; dz <= rz; ++dz)
                    for (int dy = -ry; dy <= ry; ++dy, ++row) acc += smooth_equal_bytes(ssh.rows[row][t], mm) & smooth_row_mask(g, same, dy, dz);
                ssh.col[parity][t] = acc;
                __syncthreads();
                if (owned) {
                    const uint32_t c0 = ssh.col[parity][t - xs], c1 = acc, c2 = ssh.col[parity][t + xs];
                    const uint32_t b[12] = {c0 & 0xffu, (c0 >> 8) & 0xffu, (c0 >> 16) & 0xffu, c0 >> 24, c1 & 0xffu, (c1 >> 8) & 0xffu, (c1 >> 16) & 0xffu, c1 >> 24,
                                            c2 & 0xffu, (c2 >> 8) & 0xffu, (c2 >> 16) & 0xffu, c2 >> 24};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int below = static_cast<int>((g[j] >> 9) & 3u), above = static_cast<int>((g[j] >> 11) & 3u);
                        uint32_t cnt = b[4 + j];
#pragma unroll
                        for (int dx = 1; dx <= 3; ++dx) {
                            if (dx <= below) cnt += b[4 + j - dx];
                            if (dx <= above) cnt += b[4 + j + dx];
                        }
                        if (m == ((mine >> (8 * j)) & 0xffu)) own[j] = cnt;
                        else if (takes && cnt > best[j]) { best[j] = cnt; best_label[j] = m; }
                    }
                }
                parity ^= 1u;
            }
        }

        // the change: in the box (keep), gives, the winner is another label, the density in the window
        if (owned) {
            const uint32_t kept = (ssh.keep[(t - base) >> 2] >> (4u * ((t - base) & 3u))) & 0xfu;
            uint32_t cand = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
                if ((kept & (1u << j)) && (g[j] & 256u) && ssh.give[(mine >> (8u * j)) & 0xffu] != 0u && best[j] > own[j]) cand |= 1u << j;
            uint32_t now = mine;
            if (cand) {
                if (windowed) {                                          // (uniform) the own dword of the density, only now
                    const uint32_t d = vol[bricked ? layout_offset(true, bx, bx * by, x0, y0, z0) >> 2 : static_cast<uint32_t>(o >> 2)];
#pragma unroll
                    for (uint32_t j = 0; j < 4u; ++j) {
                        const uint32_t byte = (d >> (8u * j)) & 0xffu;
                        if (byte < rule.min_byte || byte > rule.max_byte) cand &= ~(1u << j);
                    }
                }
                ChunkCursor c = {x0, y0, z0};
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    if (cand & (1u << j)) {
                        now = (now & ~(0xffu << (8u * j))) | (best_label[j] << (8u * j));
                        tally_texel(sh, tl, (mine >> (8u * j)) & 0xffu, best_label[j], c.x, c.y, c.z);
                    }
                    if (bricked) ++c.x; else c.next(0u, nx, ny);
                }
            }
            ssh.fresh[t] = now;
        }
        __syncthreads();
        // the owner of a chunk that changed leaves it in the journal as it will be
        if (t < chunks && keep != 0u && rule.store) {
            const uint32_t d = base + 4u * t;
            const uint4 will = make_uint4(ssh.fresh[d], ssh.fresh[d + 1u], ssh.fresh[d + 2u], ssh.fresh[d + 3u]);
            if (will.x != ssh.rows[centre][d] || will.y != ssh.rows[centre][d + 1u] || will.z != ssh.rows[centre][d + 2u] || will.w != ssh.rows[centre][d + 3u])
                journal_append(journal, k, will);
        }
    }
    __syncthreads();
    tally_reduce(sh, tl, out);
}

}  // namespace volym
