// The kernels of the geodesic pass (volym_geodesic_pass) and of the flood (volym_flood_labels).  Included by geodesic.hip alone.
//
// The pass: for every texel t of a request's box the key steps(t) << 8 | geo_label(t) (include/volym_hip.h has the rule), box-linear.
// The keys are the one fixed point of key(t) = min(key(t), min over the six neighbours u of key(u) + 256) on the medium, the seeds
// held at their label; every kernel below only ever lowers a word towards it, so whatever order anything runs in the bytes agree.
//   zero     the summary, the state's header and the tiles' round flags.
//   init     one wave per row (box_walk.h's walk, layout_offset, either layout): the only kernel that reads scene bytes.  It stores
//            the label on a seed, OPEN on a medium texel, NONE elsewhere; a point is matched by the lane that walks its texel, so no second writer exists.
//            It counts n_seed and n_medium and marks the tile of every seed, and the tile beyond a face the seed lies on, active
//            for round 0.
//   relax    one workgroup per ACTIVE tile of GEO_TX x GEO_TY x GEO_TZ texels, round after round.  It loads the tile and a halo of
//            one texel from the key map into LDS, iterates in LDS until an iteration lowers nothing (__syncthreads_or), stores the
//            words that changed, and for every face on which one changed marks the tile beyond it active FOR THE NEXT ROUND.
//   finish   one wave per row of the key map: OPEN becomes NONE, and the summary through LDS.
//   pack     one thread: the (steps, ~index) key of the maximum becomes max_steps and max_at.
//
// Why no workgroup waits for another, and why no freshness is needed.  A relax workgroup reads words of other tiles (its halo) that
// their owners may be storing in the same launch; a CU's L1 is not refreshed by another CU's stores, so such a load returns the
// word as it was at some time since the launch before -- any of them is a valid upper bound of the final key, because words only
// decrease.  A stale halo therefore only delays a lowering: the owner that lowered a face word has marked this tile, by an atomic
// on the NEXT round's flags and list, which are read only after the kernel boundary.  When a round marks nothing, every tile was
// last relaxed against halo words that have not changed since: a fixed point, and there is one.  Every round that marks a tile has
// lowered a word, and words are bounded below, so the rounds end; the host adds a guard all the same (geodesic.hip).
//
// The state (uint32 words): [0..2] the counts of three consecutive rounds -- round r reads count[r % 3], appends to
// count[(r + 1) % 3] and zeroes count[(r + 2) % 3], which round r - 1 read and round r + 1 will append to; [4..5] the 64-bit key of
// the maximum; [6..7] the tiles relaxed so far, for the timing script; then flag[2][n_tiles] and list[2][n_tiles], by round parity.  A tile is appended to a round's list only by the lane
// whose atomicExch found its flag 0, and the flag is cleared by the workgroup that consumes the entry a round later: a list never
// holds more than n_tiles entries.  Every load and store of the key map is of a texel inside the box (index below the box's texel
// count <= 2^31 - 2); every tile index is checked against n_tiles before it is used.
//
// The flood: an edit kernel built from the pieces of edit_chunks.h, in place, as the fill is (nearest_kernels.h): another middle.
#pragma once

#include "box_walk.h"
#include "edit_chunks.h"

namespace volym {

constexpr uint32_t GEO_TX = 32u, GEO_TY = 8u, GEO_TZ = 8u;      // the tile: 2048 texels, 8 per lane of a 256-lane workgroup
constexpr uint32_t GEO_LX = GEO_TX + 2u, GEO_LY = GEO_TY + 2u, GEO_LZ = GEO_TZ + 2u;   // ... with its halo in LDS: 3400 words
static_assert(GEO_TX * GEO_TY == 256u && GEO_TX == 32u, "a lane owns one (x, y) of the tile and walks its z; the init kernel marks tiles per half wave");

constexpr uint32_t GEODESIC_NONE = VOLYM_GEODESIC_NONE;
constexpr uint32_t GEODESIC_OPEN = 0xfffffffeu;                 // medium, not reached yet (internal: finish turns it into NONE)
// the state's header
enum { GT_COUNT = 0, GT_MAX_KEY = 4, GT_RELAXED = 6, GT_HEADER = 8 };
// struct volym_geodesic_summary as 64-bit words
enum { GS_N_SEED = 0, GS_N_MEDIUM = 1, GS_N_REACHED = 2, GS_MAX = 3, GS_CELL = 5, GS_CELL_MEDIUM = 5 + 256, GS_HIST = 5 + 512, GEODESIC_SUMMARY_WORDS = 5 + 768 };

// the box as tiles
struct GeoTiles {
    uint32_t w, h, d;                   // the box's extents, none 0
    uint32_t ntx, nty, ntz, n_tiles;    // ceil(extent / tile extent), and their product
    uint32_t max_key;                   // max_steps << 8 | 0xff: the largest key the step limit admits
};

// what the init kernel reads of the request beside the walk's arguments
struct GeoRequest {
    uint8_t seed[256], through[256];
    uint32_t max_byte, n_points;
    uint32_t points[VOLYM_GEODESIC_POINTS_MAX][3];
};

__device__ __forceinline__ uint32_t* geo_flags(uint32_t* state, const GeoTiles& g, uint32_t parity) { return state + GT_HEADER + parity * g.n_tiles; }
__device__ __forceinline__ uint32_t* geo_list(uint32_t* state, const GeoTiles& g, uint32_t parity) { return state + GT_HEADER + (2u + parity) * g.n_tiles; }

// tile t is active in the round of `parity`, whose count is *count: the first to set its flag appends it
__device__ __forceinline__ void geo_mark(uint32_t* flags, uint32_t* list, uint32_t* count, uint32_t n_tiles, uint32_t t)
{
    if (t >= n_tiles) return;
    if (atomicExch(&flags[t], 1u) == 0u) {
        const uint32_t at = atomicAdd(count, 1u);
        if (at < n_tiles) list[at] = t;
    }
}

// the summary at rest, the header and the flags of both parities.  Any grid.
__global__ __launch_bounds__(256) void volym_geodesic_zero_kernel(unsigned long long* __restrict__ summary, uint32_t* __restrict__ state, uint32_t n_state)
{
    const uint32_t i0 = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0u) {
        for (uint32_t i = threadIdx.x; i < GEODESIC_SUMMARY_WORDS; i += 256u) summary[i] = i == GS_MAX ? static_cast<unsigned long long>(GEODESIC_NONE) : 0ull;
    }
    for (uint32_t i = i0; i < n_state; i += gridDim.x * 256u) state[i] = 0u;
}

// ---- 1. init ----------------------------------------------------------------------------------------------------------------------------
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_geodesic_init_kernel(BoxWalkArgs a, GeoRequest q, GeoTiles g, uint32_t* __restrict__ keys, uint32_t* __restrict__ state,
                                                                  unsigned long long* __restrict__ summary)
{
    __shared__ uint8_t s_seed[256], s_through[256];
    __shared__ uint32_t s_points[VOLYM_GEODESIC_POINTS_MAX][3];
    s_seed[threadIdx.x] = q.seed[threadIdx.x];
    s_through[threadIdx.x] = q.through[threadIdx.x];
    if (threadIdx.x < 3u * VOLYM_GEODESIC_POINTS_MAX) s_points[threadIdx.x / 3u][threadIdx.x % 3u] = q.points[threadIdx.x / 3u][threadIdx.x % 3u];
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* const flags = geo_flags(state, g, 0u);
    uint32_t* const list = geo_list(state, g, 0u);
    uint32_t* const count = state + GT_COUNT;
    unsigned long long wave_seed = 0ull, wave_medium = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        const uint32_t y = a.lo[1] + ry, z = a.lo[2] + rz;
        const uint32_t base = row * a.w;
        const uint32_t ty = ry / GEO_TY, tz = rz / GEO_TZ;
        // the points of this row, one per lane (at most 64 of them): uniform, and 0 in all but a few rows
        const uint64_t row_points = __ballot(lane < q.n_points && s_points[lane][1] == y && s_points[lane][2] == z);
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < a.w;
            bool seed = false, medium = false;
            uint32_t label = 0u;
            if (in) {
                const uint32_t o = layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z);
                const uint32_t b = a.vol[o];
                const bool window = b >= a.min_byte && b <= q.max_byte;
                bool point = false;
                for (uint64_t m = row_points; m != 0ull; m &= m - 1ull)
                    if (s_points[__builtin_ctzll(m)][0] == a.lo[0] + xi) point = true;
                if (LABELS && (window || point)) label = a.labels[o];
                seed = point || (window && s_seed[label] != 0u);
                medium = window && s_through[label] != 0u;
                keys[base + xi] = seed ? label : (medium ? GEODESIC_OPEN : GEODESIC_NONE);
            }
            const uint64_t s = __ballot(seed);
            wave_seed += static_cast<uint32_t>(__popcll(s));
            wave_medium += static_cast<uint32_t>(__popcll(__ballot(medium && !seed)));
            if (s == 0ull) continue;                                        // (uniform)
            // Round 0's tiles, per half wave (x0 is a multiple of 64, a tile is 32 wide): the tile of a seed, and the tile beyond
            // each face a seed of the half lies on -- a seed on a face lowers that neighbour's texels though its own tile stores nothing.
            const uint32_t half = lane >> 5, l5 = lane & 31u;
            const uint32_t hs = static_cast<uint32_t>(s >> (32u * half));   // the seeds of this lane's half
            if (l5 == 0u && hs != 0u) {
                const uint32_t tx = x0 / GEO_TX + half;
                const uint32_t t = tx + g.ntx * (ty + g.nty * tz);
                geo_mark(flags, list, count, g.n_tiles, t);
                if ((hs & 1u) && tx > 0u) geo_mark(flags, list, count, g.n_tiles, t - 1u);
                if ((hs >> 31) && tx + 1u < g.ntx) geo_mark(flags, list, count, g.n_tiles, t + 1u);
                if (ry % GEO_TY == 0u && ty > 0u) geo_mark(flags, list, count, g.n_tiles, t - g.ntx);
                if (ry % GEO_TY == GEO_TY - 1u && ty + 1u < g.nty) geo_mark(flags, list, count, g.n_tiles, t + g.ntx);
                if (rz % GEO_TZ == 0u && tz > 0u) geo_mark(flags, list, count, g.n_tiles, t - g.ntx * g.nty);
                if (rz % GEO_TZ == GEO_TZ - 1u && tz + 1u < g.ntz) geo_mark(flags, list, count, g.n_tiles, t + g.ntx * g.nty);
            }
        }
    }
    if (lane == 0u && wave_seed) atomicAdd(&summary[GS_N_SEED], wave_seed);
    if (lane == 0u && wave_medium) atomicAdd(&summary[GS_N_MEDIUM], wave_medium);
}

// ---- 2. relax: one round ----------------------------------------------------------------------------------------------------------------
// A fixed grid strides over the round's list, whose count sits in device memory.  Lane (x, y) of the workgroup owns the 8 texels
// (x, y, 0..7) of the tile and walks them in ascending z on even iterations, descending on odd ones, in place in LDS: a word another
// lane is lowering reads as either value, and either is an upper bound.  NONE words (neither seed nor medium, or outside the box) are
// never written; a seed's word is its label, below every key(u) + 256, so min() never moves it.
__global__ __launch_bounds__(256) void volym_geodesic_relax_kernel(GeoTiles g, uint32_t* __restrict__ keys, uint32_t* __restrict__ state, uint32_t round)
{
    __shared__ uint32_t s_key[GEO_LZ][GEO_LY][GEO_LX];
    __shared__ uint32_t s_faces;
    const uint32_t parity = round & 1u;
    uint32_t* const flags = geo_flags(state, g, parity);
    const uint32_t* const list = geo_list(state, g, parity);
    uint32_t* const next_flags = geo_flags(state, g, parity ^ 1u);
    uint32_t* const next_list = geo_list(state, g, parity ^ 1u);
    uint32_t* const next_count = state + GT_COUNT + (round + 1u) % 3u;
    const uint32_t n = min(state[GT_COUNT + round % 3u], g.n_tiles);
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        state[GT_COUNT + (round + 2u) % 3u] = 0u;
        *reinterpret_cast<unsigned long long*>(state + GT_RELAXED) += n;       // (one thread of one launch at a time)
    }
    const uint32_t lx = threadIdx.x % GEO_TX, ly = threadIdx.x / GEO_TX;

    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t t = list[i];
        if (t >= g.n_tiles) continue;                                       // (uniform; never taken: the list holds what geo_mark stored)
        const uint32_t tx = t % g.ntx, ty = (t / g.ntx) % g.nty, tz = t / (g.ntx * g.nty);
        const uint32_t ox = tx * GEO_TX, oy = ty * GEO_TY, oz = tz * GEO_TZ;    // the tile's first texel in the box
        if (threadIdx.x == 0u) { flags[t] = 0u; s_faces = 0u; }
        // the tile and its halo; NONE outside the box (a word with index -1 wraps to >= the extent)
        for (uint32_t j = threadIdx.x; j < GEO_LX * GEO_LY * GEO_LZ; j += 256u) {
            const uint32_t jx = j % GEO_LX, jy = (j / GEO_LX) % GEO_LY, jz = j / (GEO_LX * GEO_LY);
            const uint32_t x = ox + jx - 1u, y = oy + jy - 1u, z = oz + jz - 1u;
            s_key[jz][jy][jx] = (x < g.w && y < g.h && z < g.d) ? keys[x + g.w * (y + g.h * z)] : GEODESIC_NONE;
        }
        __syncthreads();
        uint32_t was[GEO_TZ];
#pragma unroll
        for (uint32_t k = 0u; k < GEO_TZ; ++k) was[k] = s_key[k + 1u][ly + 1u][lx + 1u];

        for (uint32_t it = 0u;; ++it) {
            int lowered = 0;
#pragma unroll
            for (uint32_t k = 0u; k < GEO_TZ; ++k) {
                const uint32_t z = ((it & 1u) ? GEO_TZ - 1u - k : k) + 1u, y = ly + 1u, x = lx + 1u;
                const uint32_t own = s_key[z][y][x];
                if (own == GEODESIC_NONE) continue;
                const uint32_t m = min(min(min(s_key[z][y][x - 1u], s_key[z][y][x + 1u]), min(s_key[z][y - 1u][x], s_key[z][y + 1u][x])),
                                       min(s_key[z - 1u][y][x], s_key[z + 1u][y][x]));
                if (m >= GEODESIC_OPEN) continue;                           // no neighbour reached
                const uint32_t cand = m + 256u;                             // (m <= max_key < 2^32 - 512)
                if (cand <= g.max_key && cand < own) { s_key[z][y][x] = cand; lowered = 1; }
            }
            if (!__syncthreads_or(lowered)) break;
        }

        // the words that changed go to the map; the faces they lie on
        uint32_t faces = 0u;
#pragma unroll
        for (uint32_t k = 0u; k < GEO_TZ; ++k) {
            const uint32_t v = s_key[k + 1u][ly + 1u][lx + 1u];
            if (v != was[k]) {                                              // (a word that is NONE outside the box never changes)
                keys[(ox + lx) + g.w * ((oy + ly) + g.h * (oz + k))] = v;
                faces |= (lx == 0u ? 1u : 0u) | (lx == GEO_TX - 1u ? 2u : 0u) | (ly == 0u ? 4u : 0u) | (ly == GEO_TY - 1u ? 8u : 0u) | (k == 0u ? 16u : 0u) |
                         (k == GEO_TZ - 1u ? 32u : 0u);
            }
        }
        if (faces) atomicOr(&s_faces, faces);
        __syncthreads();
        const uint32_t f = s_faces;
        if (threadIdx.x == 0u && (f & 1u) && tx > 0u) geo_mark(next_flags, next_list, next_count, g.n_tiles, t - 1u);
        if (threadIdx.x == 1u && (f & 2u) && tx + 1u < g.ntx) geo_mark(next_flags, next_list, next_count, g.n_tiles, t + 1u);
        if (threadIdx.x == 2u && (f & 4u) && ty > 0u) geo_mark(next_flags, next_list, next_count, g.n_tiles, t - g.ntx);
        if (threadIdx.x == 3u && (f & 8u) && ty + 1u < g.nty) geo_mark(next_flags, next_list, next_count, g.n_tiles, t + g.ntx);
        if (threadIdx.x == 4u && (f & 16u) && tz > 0u) geo_mark(next_flags, next_list, next_count, g.n_tiles, t - g.ntx * g.nty);
        if (threadIdx.x == 5u && (f & 32u) && tz + 1u < g.ntz) geo_mark(next_flags, next_list, next_count, g.n_tiles, t + g.ntx * g.nty);
        __syncthreads();                                                    // s_key and s_faces are the next tile's from here
    }
}

// ---- 3. finish: OPEN -> NONE, and the summary -------------------------------------------------------------------------------------------
// counts[v] += the lanes of `who`, each of which carries the value v: where they all carry the same one, one lane adds them (the
// nearest pass's resolve kernel counts so)
__device__ __forceinline__ void geodesic_count(uint32_t* counts, uint64_t who, bool mine, uint32_t v, uint32_t lane)
{
    if (!who) return;                                               // (wave-uniform)
    const uint32_t lead = __shfl(v, static_cast<int>(__ffsll(static_cast<unsigned long long>(who))) - 1);
    if (__ballot(mine && v != lead) == 0ull) {
        if (lane == 0u) atomicAdd(&counts[lead], static_cast<uint32_t>(__popcll(who)));
    } else if (mine) {
        atomicAdd(&counts[v], 1u);
    }
}

// One wave per row of the map (n_rows rows of w words).  The maximum as one 64-bit key steps << 32 | ~index: the largest steps, and
// among equals the smallest box-linear index, the first in (z, y, x).  A workgroup walks fewer than 2^32 texels: u32 in LDS.
__global__ __launch_bounds__(256) void volym_geodesic_finish_kernel(uint32_t w, uint32_t n_rows, uint32_t* __restrict__ keys, uint32_t* __restrict__ state,
                                                                    unsigned long long* __restrict__ summary)
{
    __shared__ uint32_t s_cell[256], s_cell_medium[256], s_hist[256];
    __shared__ unsigned long long s_reached, s_max;
    s_cell[threadIdx.x] = s_cell_medium[threadIdx.x] = s_hist[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) { s_reached = 0ull; s_max = 0ull; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long wave_reached = 0ull, best = 0ull;
    for (uint32_t row = box_wave_index(); row < n_rows; row += gridDim.x * 4u) {
        const uint32_t base = row * w;
        for (uint32_t x0 = 0u; x0 < w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < w;
            const uint32_t key = in ? keys[base + xi] : GEODESIC_NONE;
            if (key == GEODESIC_OPEN) keys[base + xi] = GEODESIC_NONE;
            const bool reached = key < GEODESIC_OPEN;
            const uint32_t steps = key >> 8, label = key & 0xffu;
            const bool grown = reached && steps != 0u;                  // reached and no seed
            const uint64_t r = __ballot(reached);
            geodesic_count(s_cell, r, reached, label, lane);
            geodesic_count(s_cell_medium, __ballot(grown), grown, label, lane);
            geodesic_count(s_hist, r, reached, min(steps, 255u), lane);
            wave_reached += static_cast<uint32_t>(__popcll(r));
            if (reached) {
                // (1 + steps, so that a reached seed's key is not 0, the key of "none")
                const unsigned long long k = (static_cast<unsigned long long>(steps + 1u) << 32) | (~(base + xi));
                best = k > best ? k : best;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0u && wave_reached) { atomicAdd(&s_reached, wave_reached); atomicMax(&s_max, best); }
    __syncthreads();
    // only the entries this workgroup touched go to memory
    if (s_cell[threadIdx.x]) atomicAdd(&summary[GS_CELL + threadIdx.x], static_cast<unsigned long long>(s_cell[threadIdx.x]));
    if (s_cell_medium[threadIdx.x]) atomicAdd(&summary[GS_CELL_MEDIUM + threadIdx.x], static_cast<unsigned long long>(s_cell_medium[threadIdx.x]));
    if (s_hist[threadIdx.x]) atomicAdd(&summary[GS_HIST + threadIdx.x], static_cast<unsigned long long>(s_hist[threadIdx.x]));
    if (threadIdx.x == 0u && s_reached) {
        atomicAdd(&summary[GS_N_REACHED], s_reached);
        atomicMax(reinterpret_cast<unsigned long long*>(state + GT_MAX_KEY), s_max);
    }
}

// the key of the maximum into the summary's max_steps and max_at (volume coordinates).  One thread.
__global__ __launch_bounds__(64) void volym_geodesic_pack_kernel(BoxWalkArgs a, const uint32_t* __restrict__ state, unsigned long long* __restrict__ summary)
{
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const unsigned long long k = *reinterpret_cast<const unsigned long long*>(state + GT_MAX_KEY);
    if (k == 0ull) return;                                              // nothing reached: NONE and {0, 0, 0}, as the zero kernel left them
    const uint32_t steps = static_cast<uint32_t>(k >> 32) - 1u, index = ~static_cast<uint32_t>(k);
    const uint32_t x = a.lo[0] + index % a.w, y = a.lo[1] + (index / a.w) % a.h, z = a.lo[2] + index / (a.w * a.h);
    summary[GS_MAX] = static_cast<unsigned long long>(steps) | (static_cast<unsigned long long>(x) << 32);
    summary[GS_MAX + 1] = static_cast<unsigned long long>(y) | (static_cast<unsigned long long>(z) << 32);
}

// ---- the flood (volym_flood_labels) ---------------------------------------------------------------------------------------------------
// what the rule reads beside the `give` marks: the window, the band, the take and to tables, and the pass's box
struct FloodRule {
    uint32_t min_byte, max_byte;
    uint32_t steps_lo, steps_hi;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t box[6];                // the box of the geodesic pass: the map is linear in it, and the request's box lies inside it
    uint8_t take[256], to[256];
};

// One pass over the items of the request's slab, as the fill walks it (nearest_kernels.h fill_pass): the 16 labels first, the table
// `marks` only marks the labels that give; then the density; then per candidate its key from the snapshot: it becomes to[g] iff the
// key is not NONE, take[g], to[g] is not its label, and steps lies in the band.  The chunk is stored only if a byte changed and
// rule.store says so; every texel is decided from the snapshot and the bytes before the edit.
template <bool JOURNAL>
__device__ __forceinline__ void flood_pass(RelabelShared& sh, uint8_t* s_take, uint8_t* s_to, uint4* __restrict__ labels, const uint4* __restrict__ vol,
                                           const uint32_t* __restrict__ keys, const RelabelOut& out, const LabelTable& marks, const CropSlab& s, const FloodRule& rule,
                                           const LabelJournal& journal, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    s_take[threadIdx.x] = rule.take[threadIdx.x];
    s_to[threadIdx.x] = rule.to[threadIdx.x];
    edit_prologue(sh, marks);
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    RelabelTally t;

    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        if (!bricked && !relabel_owns_chunk(s, i, nx, ny, k)) continue;
        if (!keep) continue;                                             // before any load
        const uint4 lv = labels[k];
        uint32_t lb[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t cand = chunk_candidates(sh, lb, keep);
        if (!cand) continue;                                             // no density, no snapshot, no store
        cand = chunk_in_window(vol[k], rule.min_byte, rule.max_byte, cand);
        if (!cand) continue;
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);      // (k < 2^28: a layout has fewer than 2^32 bytes)
        bool stored = false;
        ChunkCursor c = {x0, y0, z0};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            c.at(bricked, j, x0, y0);
            if (cand & (1u << j)) {
                const uint32_t key = keys[box_linear(rule.box, c.x, c.y, c.z)];
                if (key != GEODESIC_NONE) {
                    const uint32_t g = key & 0xffu, steps = key >> 8, becomes = s_to[g];
                    const uint32_t shift = 8u * (j & 3u), l = (lb[j >> 2] >> shift) & 0xffu;
                    if (s_take[g] != 0u && becomes != l && steps >= rule.steps_lo && steps <= rule.steps_hi) {
                        lb[j >> 2] = (lb[j >> 2] & ~(0xffu << shift)) | (becomes << shift);
                        tally_texel(sh, t, l, becomes, c.x, c.y, c.z);
                        stored = true;
                    }
                }
            }
            c.next(bricked, nx, ny);
        }
        if (stored && rule.store) chunk_store<JOURNAL>(labels, k, lv, lb, journal);
    }
    tally_reduce(sh, t, out);
}

__global__ __launch_bounds__(256) void volym_geodesic_flood_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ keys,
                                                                   RelabelOut out, LabelTable marks, CropSlab s, FloodRule rule, uint32_t nx, uint32_t ny, uint32_t nz,
                                                                   uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ uint8_t s_take[256], s_to[256];
    flood_pass<false>(sh, s_take, s_to, labels, vol, keys, out, marks, s, rule, LabelJournal{}, nx, ny, nz, bricked, n_items);
}

// the same edit while the history is on and the request is no DRY_RUN
__global__ __launch_bounds__(256) void volym_geodesic_flood_journal_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ keys,
                                                                           RelabelOut out, LabelTable marks, CropSlab s, FloodRule rule, LabelJournal journal, uint32_t nx,
                                                                           uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ uint8_t s_take[256], s_to[256];
    flood_pass<true>(sh, s_take, s_to, labels, vol, keys, out, marks, s, rule, journal, nx, ny, nz, bricked, n_items);
}

}  // namespace volym
