// The kernels of the nearest pass (volym_nearest_pass) and of the fill (volym_fill_labels).  Included by nearest.hip alone.
//
// The pass: for every texel t of a request's box, site(t) -- the SOLID texel s of the box that minimises the distance pass's d2(t, s),
// ties to the first s in ascending (z, y, x) -- as the box-linear index of s, and near_label(t), the label byte of s.  It is the
// distance pass's separable transform (distance_kernels.h) with the argmin kept beside the min:
//   rows     one wave per row: g = wx * (distance to the nearest seed of the row)^2 and wx[i] = that seed's x offset in the box; the
//            left seed wins dl == dr.
//   columns  along y, then along z: the lower-envelope sweep, in place on g, which also stores the entry that wins each position into
//            wy, then wz, at the position it evaluates -- out of place and coalesced, so the stacks do not grow.  On equal f the sweep
//            keeps the entry with the smaller index: its pop test keeps the older parabola on equality, and a new one wins from
//            floor(meeting point) + 1 on.
//   resolve  one wave per row: z'' = wz[x, y, z], y'' = wy[x, y, z''], x'' = wx[x, y'', z''], the site's index and its label through
//            layout_offset, both stored, and the summary through LDS.
// Why the chain is the rule's site: the first minimiser in (z, y, x) has the smallest z' among the minimisers, within that slice the
// smallest y', within that row the smallest x'; the z sweep picks the smallest z' that attains the minimum, the y sweep of slice z' the
// smallest y', the row sweep the left seed.
// g lives in the words of the site map until the resolve kernel, which reads only the winners, overwrites them with the sites.
// After the rows g is finite exactly in the rows that hold a seed, after the y sweep in the slices that hold one, after the z sweep
// everywhere or nowhere: a winner is read only where it was written, and the box has a site for every texel or for none (n_solid says
// which).  The sweep exists twice, here and in distance_kernels.h: shared as a device function the distance pass's columns kernel came
// out with two operands of one s_and_b64 exchanged, and that kernel's code is pinned.
// Widths are the distance pass's: every index is below the box's texel count <= 2^31 - 2, an axis has at most 4096 texels, so a
// winner fits 16 bits, and every f is below 2^32.  Every load and store is of a texel of the request's box, which volym_nearest_check
// puts inside the volume, or of an element of the maps, the winners or the work arrays with an index below the box's texel count
// (the chain's winners are clamped to their axis, so that no word of memory, whatever it holds, leads outside).
//
// The fill: an edit kernel built from the pieces of edit_chunks.h, in place, whose new label is the texel's near_label.
#pragma once

#include "box_walk.h"
#include "edit_chunks.h"

namespace volym {

struct NearestArgs : BoxWalkArgs {      // w * n_rows <= 2^31 - 2 (volym_nearest_check)
    uint32_t weight[3];
};

constexpr uint32_t NEAREST_NONE = VOLYM_NEAREST_NONE;
// struct volym_nearest_summary as 64-bit words
enum { NS_N_SOLID = 0, NS_N_PRESENT = 1, NS_N_FINITE = 2, NS_CELL = 3, NS_CELL_PRESENT = 3 + 256, NEAREST_SUMMARY_WORDS = 3 + 256 + 256 };

// the summary at rest (what an empty box leaves).  One workgroup.
__global__ __launch_bounds__(256) void volym_nearest_init_kernel(unsigned long long* __restrict__ summary)
{
    for (uint32_t i = threadIdx.x; i < NEAREST_SUMMARY_WORDS; i += 256u) summary[i] = 0ull;
}

// ---- 1. rows ----------------------------------------------------------------------------------------------------------------------------
// The distance pass's row sweep without INSIDE: left to right g gets dl, the distance to the nearest seed at or left of the texel
// (NONE: none), dl == 0 marks the seeds; back from the right the nearer of the two sides, the left one on equality.
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_nearest_rows_kernel(NearestArgs a, BoxSelect select, uint32_t* __restrict__ g, uint16_t* __restrict__ wx,
                                                                 unsigned long long* __restrict__ summary)
{
    __shared__ uint8_t s_select[256];
    s_select[threadIdx.x] = select.v[threadIdx.x];
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);        // bits 0..lane
    const uint64_t from = ~0ull << lane;                                        // bits lane..63
    unsigned long long wave_solid = 0ull, wave_present = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t y = a.lo[1] + row % a.h, z = a.lo[2] + row / a.h;
        const uint32_t base = row * a.w;
        uint32_t carry = NEAREST_NONE;                              // x of the last seed of the chunks before (wave-uniform)
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < a.w;
            bool present = false, solid = false;
            if (in) {
                uint32_t label;
                present = box_present<LABELS>(a, layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z), label);
                solid = present && box_selected(s_select, label);
            }
            const uint64_t s = __ballot(solid);
            const uint64_t left = s & upto;
            const uint32_t at = left ? x0 + (63u - static_cast<uint32_t>(__clzll(left))) : carry;
            if (in) g[base + xi] = at == NEAREST_NONE ? NEAREST_NONE : xi - at;
            if (s) carry = x0 + (63u - static_cast<uint32_t>(__clzll(s)));
            wave_solid += static_cast<uint32_t>(__popcll(s));
            wave_present += static_cast<uint32_t>(__popcll(__ballot(present)));
        }
        // back from the right (each lane reads the words it stored itself); chunk k starts at 64 * k
        carry = NEAREST_NONE;
        for (uint32_t k = (a.w + 63u) / 64u; k-- > 0u;) {
            const uint32_t x0 = k * 64u, xi = x0 + lane;
            const bool in = xi < a.w;
            const uint32_t dl = in ? g[base + xi] : NEAREST_NONE;
            const uint64_t s = __ballot(in && dl == 0u);
            const uint64_t right = s & from;
            const uint32_t at = right ? x0 + static_cast<uint32_t>(__builtin_ctzll(right)) : carry;
            const uint32_t dr = at == NEAREST_NONE ? NEAREST_NONE : at - xi;
            const uint32_t m = min(dl, dr);                         // at most 4095, or NONE
            if (in) {
                g[base + xi] = m == NEAREST_NONE ? NEAREST_NONE : a.weight[0] * m * m;
                wx[base + xi] = static_cast<uint16_t>(m == NEAREST_NONE ? 0xffffu : (dl <= dr ? xi - dl : at));     // the left one wins dl == dr
            }
            if (s) carry = x0 + static_cast<uint32_t>(__builtin_ctzll(s));
        }
    }
    if (lane == 0u && wave_solid) atomicAdd(&summary[NS_N_SOLID], wave_solid);
    if (lane == 0u && wave_present) atomicAdd(&summary[NS_N_PRESENT], wave_present);
}

// ---- 2. columns: in place, f(i) = min_j g(j) + w * (i - j)^2 over the finite g(j), and the j that attains it --------------------------
// floor(num / den) for 0 <= num < 2^34, 0 < den < 2^20: the f64 quotient proposes, the two loops settle it in integers (the distance
// pass's division, distance_kernels.h, which says why neither loop turns)
__device__ __forceinline__ uint32_t nearest_floor_div(uint64_t num, uint32_t den)
{
    uint32_t q = static_cast<uint32_t>(static_cast<double>(num) / static_cast<double>(den));
    while (static_cast<uint64_t>(q) * den > num) --q;
    while (static_cast<uint64_t>(q + 1u) * den <= num) ++q;
    return q;
}

struct NearestColumns {
    uint32_t n;                         // entries of a column (the box's extent along the axis), 2..4096
    uint32_t stride;                    // elements between two entries of a column
    uint32_t n_cols;                    // columns: the texels of the box / n
    uint32_t inner, outer;              // column c starts at element c % inner + (c / inner) * outer
    uint32_t weight;
};

// One lane per column, adjacent lanes on adjacent x: every load and store of g, of the stacks and of the winners is coalesced.  The
// stacks are the distance pass's: entry k of the column that starts at `base` is word base + k * stride of each of the two work
// arrays, (site | first index it wins from << 16) and the site's g, kept because g is evaluated in place.
__global__ __launch_bounds__(64) void volym_nearest_columns_kernel(NearestColumns a, uint32_t* __restrict__ g_map, uint32_t* __restrict__ stack,
                                                                   uint32_t* __restrict__ stack_g, uint16_t* __restrict__ winner)
{
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.n_cols) return;
    const uint32_t base = c % a.inner + (c / a.inner) * a.outer;
    const uint32_t w = a.weight;
    // the stack's top in registers: site, the first index it wins from, the site's g
    int q = -1;
    uint32_t top_s = 0u, top_t = 0u, top_g = 0u;
    for (uint32_t u = 0u; u < a.n; ++u) {
        const uint32_t g = g_map[base + u * a.stride];
        if (g == NEAREST_NONE) continue;                            // no parabola
        // pop while the new parabola is lower where the top's stretch starts; on equality the older one, the smaller site, stays
        while (q >= 0) {
            const uint32_t ds = top_t > top_s ? top_t - top_s : top_s - top_t, du = u - top_t;
            if (w * ds * ds + top_g <= w * du * du + g) break;
            if (--q >= 0) {
                const uint32_t e = stack[base + static_cast<uint32_t>(q) * a.stride];
                top_s = e & 0xffffu; top_t = e >> 16;
                top_g = stack_g[base + static_cast<uint32_t>(q) * a.stride];
            }
        }
        uint32_t first = 0u;
        if (q >= 0) {
            // the first index the new parabola wins from: 1 + floor of where it meets the top's, so that the top keeps an exact tie.  The
            // numerator is no less than 0 (the pop test) and below 64 * 4096^2 + 2^31 < 2^34.
            const uint64_t num = static_cast<uint64_t>(w) * (u * u - top_s * top_s) + g - top_g;      // (unsigned wrap-around of + g - top_g cancels: the sum is >= 0)
            first = nearest_floor_div(num, 2u * w * (u - top_s)) + 1u;
            if (first >= a.n) continue;                             // it wins nowhere in the column
        }
        ++q;
        top_s = u; top_t = first; top_g = g;
        stack[base + static_cast<uint32_t>(q) * a.stride] = u | (first << 16);    // (both below 4096)
        stack_g[base + static_cast<uint32_t>(q) * a.stride] = g;
    }
    if (q < 0) return;                                              // an all-NONE column stays NONE, its winners unwritten
    for (uint32_t u = a.n; u-- > 0u;) {
        const uint32_t d = u > top_s ? u - top_s : top_s - u;
        g_map[base + u * a.stride] = w * d * d + top_g;
        winner[base + u * a.stride] = static_cast<uint16_t>(top_s);
        if (u == top_t && q > 0) {
            --q;
            const uint32_t e = stack[base + static_cast<uint32_t>(q) * a.stride];
            top_s = e & 0xffffu; top_t = e >> 16;
            top_g = stack_g[base + static_cast<uint32_t>(q) * a.stride];
        }
    }
}

// ---- 3. resolve: the chain of the winners, the site, its label, and the summary ---------------------------------------------------------
// counts[v] += the lanes of `who`, each of which carries the value v: where they all carry the same one -- the inside of a cell -- one
// lane adds them
__device__ __forceinline__ void nearest_count(uint32_t* counts, uint64_t who, bool mine, uint32_t v, uint32_t lane)
{
    if (!who) return;                                               // (wave-uniform)
    const uint32_t lead = __shfl(v, static_cast<int>(__ffsll(static_cast<unsigned long long>(who))) - 1);
    if (__ballot(mine && v != lead) == 0ull) {
        if (lane == 0u) atomicAdd(&counts[lead], static_cast<uint32_t>(__popcll(who)));
    } else if (mine) {
        atomicAdd(&counts[v], 1u);
    }
}

// `sites` holds g when the kernel starts; it is never read.  d: the box's extent along z.  A workgroup walks fewer than 2^32 texels
// (4 waves, WALK_ROWS_PER_WAVE rows of at most 4096): u32 in LDS.
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_nearest_resolve_kernel(NearestArgs a, BoxSelect select, uint32_t d, const uint16_t* __restrict__ wx,
                                                                    const uint16_t* __restrict__ wy, const uint16_t* __restrict__ wz, uint32_t* __restrict__ sites,
                                                                    uint8_t* __restrict__ near, unsigned long long* summary)
{
    __shared__ uint8_t s_select[256];
    __shared__ uint32_t s_cell[256], s_cell_present[256];
    __shared__ unsigned long long s_finite;
    s_select[threadIdx.x] = select.v[threadIdx.x];
    s_cell[threadIdx.x] = s_cell_present[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) s_finite = 0ull;
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const bool any = summary[NS_N_SOLID] != 0ull;                   // the rows kernel's count: every texel has a site, or none has
    unsigned long long wave_finite = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        const uint32_t base = row * a.w;
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane, i = base + xi;
            const bool in = xi < a.w, finite = in && any;
            uint32_t site = NEAREST_NONE, nl = 0u;
            bool waits = false;                                     // PRESENT and not SOLID: what a fill of all the matter would move
            if (finite) {
                const uint32_t zz = d > 1u ? min(static_cast<uint32_t>(wz[i]), d - 1u) : rz;
                const uint32_t yy = a.h > 1u ? min(static_cast<uint32_t>(wy[xi + a.w * (ry + a.h * zz)]), a.h - 1u) : ry;
                const uint32_t row_s = a.w * (yy + a.h * zz);
                const uint32_t xx = min(static_cast<uint32_t>(wx[xi + row_s]), a.w - 1u);
                site = xx + row_s;
                if (LABELS) nl = a.labels[layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xx, a.lo[1] + yy, a.lo[2] + zz)];
                uint32_t label;
                waits = box_present<LABELS>(a, layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, a.lo[1] + ry, a.lo[2] + rz), label) &&
                        !box_selected(s_select, label);
            }
            if (in) { sites[i] = site; near[i] = static_cast<uint8_t>(nl); }
            const uint64_t f = __ballot(finite);
            nearest_count(s_cell, f, finite, nl, lane);
            nearest_count(s_cell_present, __ballot(waits), waits, nl, lane);
            wave_finite += static_cast<uint32_t>(__popcll(f));
        }
    }
    if (lane == 0u && wave_finite) atomicAdd(&s_finite, wave_finite);
    __syncthreads();
    // only the entries this workgroup touched go to memory
    if (s_cell[threadIdx.x]) atomicAdd(&summary[NS_CELL + threadIdx.x], static_cast<unsigned long long>(s_cell[threadIdx.x]));
    if (s_cell_present[threadIdx.x]) atomicAdd(&summary[NS_CELL_PRESENT + threadIdx.x], static_cast<unsigned long long>(s_cell_present[threadIdx.x]));
    if (threadIdx.x == 0u && s_finite) atomicAdd(&summary[NS_N_FINITE], s_finite);
}

// out (box-linear in the sub-box, x fastest) = the bytes of a box-linear byte volume of width w and height h, from element `first`
// on: one thread per byte (volym_read_nearest_labels of a sub-box that is no run of whole slices)
__global__ __launch_bounds__(256) void volym_nearest_gather_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, uint32_t w, uint32_t h, uint32_t first,
                                                                   uint32_t sw, uint32_t sh, uint32_t total)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    out[i] = src[first + i % sw + w * ((i / sw) % sh + h * (i / (sw * sh)))];
}

// ---- the fill (volym_fill_labels) -----------------------------------------------------------------------------------------------------
// what the rule reads beside the `give` marks: the window, the band, the take table, and the pass's box and weights
struct FillRule {
    uint32_t min_byte, max_byte;
    uint32_t d2_lo, d2_hi;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t box[6];                // the box of the nearest pass: the maps are linear in it, and the request's box lies inside it
    uint32_t weight[3];             // ... and its weights
    uint8_t take[256];
};

// One pass over the items of the request's slab, as relabel_pass walks it (relabel_kernels.h): a lane at a time, the 16 labels
// first.  The table `to` only marks the labels that give (to[l] != l iff give[l] != 0), for chunk_candidates; a chunk without such a
// texel in the box loads nothing more.  Else the density, then per candidate its site and near label n from the snapshot: it becomes n
// iff it has a site, take[n], n is not its label, and d2(t, site) lies in the band.  The site's coordinates come from its index by two
// 32-bit integer divisions, which are exact.  d2 <= 3 * 64 * 4095^2 < 2^32.  The chunk is stored only if a byte changed and rule.store says so;
// every texel is decided from the snapshot and the bytes before the edit.
template <bool JOURNAL>
__device__ __forceinline__ void fill_pass(RelabelShared& sh, uint8_t* s_take, uint4* __restrict__ labels, const uint4* __restrict__ vol,
                                          const uint32_t* __restrict__ sites, const uint8_t* __restrict__ near, const RelabelOut& out, const LabelTable& to,
                                          const CropSlab& s, const FillRule& rule, const LabelJournal& journal, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked,
                                          uint32_t n_items)
{
    s_take[threadIdx.x] = rule.take[threadIdx.x];
    edit_prologue(sh, to);
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    const uint32_t bw = rule.box[3] - rule.box[0], bh = rule.box[4] - rule.box[1];
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
                const uint32_t at = box_linear(rule.box, c.x, c.y, c.z);
                const uint32_t site = sites[at];
                if (site != NEAREST_NONE) {
                    const uint32_t becomes = near[at];
                    const uint32_t shift = 8u * (j & 3u), l = (lb[j >> 2] >> shift) & 0xffu;
                    if (s_take[becomes] != 0u && becomes != l) {
                        const uint32_t rest = site / bw, sx = site - rest * bw, sz = rest / bh, sy = rest - sz * bh;
                        const uint32_t tx = c.x - rule.box[0], ty = c.y - rule.box[1], tz = c.z - rule.box[2];
                        const uint32_t dx = tx > sx ? tx - sx : sx - tx, dy = ty > sy ? ty - sy : sy - ty, dz = tz > sz ? tz - sz : sz - tz;
                        const uint32_t d2 = rule.weight[0] * dx * dx + rule.weight[1] * dy * dy + rule.weight[2] * dz * dz;
                        if (d2 >= rule.d2_lo && d2 <= rule.d2_hi) {
                            lb[j >> 2] = (lb[j >> 2] & ~(0xffu << shift)) | (becomes << shift);
                            tally_texel(sh, t, l, becomes, c.x, c.y, c.z);
                            stored = true;
                        }
                    }
                }
            }
            c.next(bricked, nx, ny);
        }
        if (stored && rule.store) chunk_store<JOURNAL>(labels, k, lv, lb, journal);
    }
    tally_reduce(sh, t, out);
}

__global__ __launch_bounds__(256) void volym_nearest_fill_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ sites,
                                                                 const uint8_t* __restrict__ near, RelabelOut out, LabelTable to, CropSlab s, FillRule rule, uint32_t nx,
                                                                 uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ uint8_t s_take[256];
    fill_pass<false>(sh, s_take, labels, vol, sites, near, out, to, s, rule, LabelJournal{}, nx, ny, nz, bricked, n_items);
}

// the same edit while the history is on and the request is no DRY_RUN
__global__ __launch_bounds__(256) void volym_nearest_fill_journal_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ sites,
                                                                         const uint8_t* __restrict__ near, RelabelOut out, LabelTable to, CropSlab s, FillRule rule,
                                                                         LabelJournal journal, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ uint8_t s_take[256];
    fill_pass<true>(sh, s_take, labels, vol, sites, near, out, to, s, rule, journal, nx, ny, nz, bricked, n_items);
}

}  // namespace volym
