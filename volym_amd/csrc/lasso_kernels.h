// The kernels of the lasso (volym_lasso_labels): the label edit whose texels are decided by where they project.  Included by
// lasso.hip alone (volym_lasso_raster_kernel is no template).  Everything of the edit kernel but the selection rule is edit_chunks.h's: the walk (wave_chunk_step),
// the tail (selected_chunk_tail), the prologue, the tally and the journal.  Here: the polygon's bit plane, the integer view, the
// half-space cull and the mask of a chunk.
#pragma once

#include "edit_chunks.h"

namespace volym {

// One edge of the polygon, vertex i -> vertex (i + 1) % n, as the host lays it out (lasso.hip).  16 bytes, read by the uniform loop
// index: one scalar load per edge and wave.
struct LassoEdge { int32_t x0, y0, x1, y1; };
static_assert(sizeof(LassoEdge) == 16, "LassoEdge is 16 bytes");

// The request as the kernels read it: the integer view (include/volym_hip.h), the mask's rect {x0, y0, x1, y1} (hi exclusive; empty:
// all 0), the plane's row stride in words, and the edit's window.  All of it is uniform.
struct LassoRule {
    int64_t c[3];
    int64_t depth[2];
    int32_t m[3][3];
    uint32_t rect[4];
    uint32_t stride;
    uint32_t min_byte, max_byte;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t outside;               // 1: VOLYM_LASSO_OUTSIDE
};

// ---- the polygon's bit plane --------------------------------------------------------------------------------------------------------
// A wave covers 64 pixels of one row of the rect, so (y0 <= py) != (y1 <= py) is wave-uniform: an edge that does not span the row is
// skipped by a scalar branch and only the spanning edges cost vector work -- one 64-bit product per lane against a uniform one.
// Every factor is below 2^22: exact.  The wave's 64 parities are one ballot, stored as the two words of the plane it covers by lane
// 0; the bits past the rect's right edge are 0.  Every word of the plane is written by exactly one wave.
__global__ __launch_bounds__(256) void volym_lasso_raster_kernel(uint32_t* __restrict__ plane, const LassoEdge* __restrict__ edges, uint32_t n_edges, uint32_t rx0,
                                                                 uint32_t ry0, uint32_t rx1, uint32_t ry1, uint32_t stride)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const uint32_t per_row = (rx1 - rx0 + 63u) / 64u;
    const uint32_t w = blockIdx.x * 4u + wave;
    const uint32_t row = w / per_row, seg = w - row * per_row;
    if (row >= ry1 - ry0) return;                                        // (uniform)
    const int32_t py = static_cast<int32_t>(ry0 + row);
    const int32_t px = static_cast<int32_t>(rx0 + seg * 64u + lane);
    uint32_t odd = 0;
    for (uint32_t g = 0; g < n_edges; ++g) {
        const LassoEdge e = edges[g];
        if ((e.y0 <= py) == (e.y1 <= py)) continue;                      // (uniform)
        const int64_t lhs = static_cast<int64_t>(px - e.x0) * (e.y1 - e.y0);
        const int64_t rhs = static_cast<int64_t>(e.x1 - e.x0) * (py - e.y0);
        odd ^= (e.y1 > e.y0 ? lhs < rhs : lhs > rhs) ? 1u : 0u;
    }
    const unsigned long long bits = __ballot(odd != 0u && static_cast<uint32_t>(px) < rx1);
    if (lane == 0u) {
        const uint32_t at = row * stride + seg * 2u;
        plane[at] = static_cast<uint32_t>(bits);
        if (seg * 2u + 1u < stride) plane[at + 1u] = static_cast<uint32_t>(bits >> 32);
    }
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
// X < r * D, exact for |X|, |D| < 2^62 and r < 2^31, although r * D may not fit 64 bits: D = dh * 2^32 + dl (dh signed, dl unsigned)
// gives r * D = hi * 2^32 + lo with hi = r * dh + (r * dl >> 32), and the two are compared high word first.
__device__ __forceinline__ bool lasso_below(int64_t X, uint32_t r, int64_t D)
{
    const uint64_t low = static_cast<uint64_t>(r) * static_cast<uint32_t>(D);
    const int64_t hi = static_cast<int64_t>(static_cast<int32_t>(r)) * static_cast<int32_t>(D >> 32) + static_cast<int64_t>(low >> 32);
    const int64_t xh = X >> 32;
    return xh < hi || (xh == hi && static_cast<uint32_t>(X) < static_cast<uint32_t>(low));
}

// row r of the view at texel (x, y, z): m[r] . (2x + 1, 2y + 1, 2z + 1) + c[r]; every product is int32 x int32 -> int64
__device__ __forceinline__ int64_t lasso_row(const LassoRule& v, int r, uint32_t x, uint32_t y, uint32_t z)
{
    return static_cast<int64_t>(v.m[r][0]) * static_cast<int32_t>(2u * x + 1u) + static_cast<int64_t>(v.m[r][1]) * static_cast<int32_t>(2u * y + 1u) +
           static_cast<int64_t>(v.m[r][2]) * static_cast<int32_t>(2u * z + 1u) + v.c[r];
}

// Which of the six conditions of "lands inside the rect" the point (X, Y, D) violates.  Each is a half-space of an AFFINE function of
// the texel (D - depth[0], depth[1] - D, X - rx0 D, rx1 D - X, Y - ry0 D, ry1 D - Y), whatever the sign of D: no division.
__device__ __forceinline__ uint32_t lasso_violations(const LassoRule& v, int64_t X, int64_t Y, int64_t D)
{
    return (D < v.depth[0] ? 1u : 0u) | (D > v.depth[1] ? 2u : 0u) | (lasso_below(X, v.rect[0], D) ? 4u : 0u) | (lasso_below(X, v.rect[2], D) ? 0u : 8u) |
           (lasso_below(Y, v.rect[1], D) ? 16u : 0u) | (lasso_below(Y, v.rect[3], D) ? 0u : 32u);
}

// Can no texel of the box [lo, hi] (hi INCLUSIVE) be inside?  True iff all 8 corners violate the same condition: an affine function
// that is on the wrong side at every corner of a box is on the wrong side in all of it.  False says nothing.
__device__ __forceinline__ bool lasso_box_misses(const LassoRule& v, const uint32_t lo[3], const uint32_t hi[3])
{
    uint32_t all = 63u;
#pragma unroll 1
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t x = (k & 1u) ? hi[0] : lo[0], y = (k & 2u) ? hi[1] : lo[1], z = (k & 4u) ? hi[2] : lo[2];
        all &= lasso_violations(v, lasso_row(v, 0, x, y, z), lasso_row(v, 1, x, y, z), lasso_row(v, 2, x, y, z));
    }
    return all != 0u;
}

// floor(X / D) for 0 <= X < 2^14 * D, 0 < D < 2^51: a float estimate (relative error below 2^-21: off by one at most), corrected by
// multiply and compare -- no 64-bit division.  The estimate is at most one above the quotient, so p * D <= X + D < 2^52.
__device__ __forceinline__ uint32_t lasso_quotient(int64_t X, int64_t D)
{
    uint32_t p = static_cast<uint32_t>(static_cast<float>(X) * __builtin_amdgcn_rcpf(static_cast<float>(D)));
    p = p < 16384u ? p : 16384u;
    int64_t rem = X - static_cast<int64_t>(p) * D;
    while (rem < 0) { --p; rem += D; }
    while (rem >= D) { ++p; rem -= D; }
    return p;
}

// Is the texel at (X, Y, D) inside: does it land on a pixel of the mask?  On-screen test first, then the two quotients, then one bit.
__device__ __forceinline__ bool lasso_inside(const LassoRule& v, const uint32_t* __restrict__ plane, int64_t X, int64_t Y, int64_t D)
{
    if (lasso_violations(v, X, Y, D) != 0u) return false;
    const uint32_t ux = lasso_quotient(X, D) - v.rect[0], uy = lasso_quotient(Y, D) - v.rect[1];
    if (ux >= v.rect[2] - v.rect[0] || uy >= v.rect[3] - v.rect[1]) return false;       // (never: the conditions above say so exactly)
    return ((plane[uy * v.stride + (ux >> 5)] >> (ux & 31u)) & 1u) != 0u;
}

// One pass over the items of slab s (make_crop_slab over the request's box, s.box_lo/hi that box, no plane), in either layout: the
// walk and the tail of edit_chunks.h (wave_chunk_step, selected_chunk_tail) around the lasso's selection rule, the 16-bit mask of
// the chunk's texels that are inside (OUTSIDE: that are not).  The box of the wave's 64 chunks is held against the six half-spaces
// first: if it misses, the wave goes on (or, OUTSIDE, selects all it keeps) without a mask read.  Then the lane's own chunk box, then
// each texel: X, Y and D advance by constants along the chunk, beside the coordinates, in a loop of this pass's own.
template <bool JOURNAL>
__device__ __forceinline__ void lasso_pass(RelabelShared& sh, uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ plane,
                                           const RelabelOut& out, const LabelTable& to, const CropSlab& s, const LassoRule& rule, const LabelJournal& journal,
                                           uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    edit_prologue(sh, to);
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const bool windowed = rule.min_byte > 0u || rule.max_byte < 255u;   // (uniform)
    const bool no_rect = rule.rect[0] == rule.rect[2];                   // (uniform) an empty rect: nothing is inside
    RelabelTally t;

    for (uint32_t base = blockIdx.x * 256u + wave * 64u; base < n_items; base += gridDim.x * 256u) {
        WaveChunk c;
        if (!wave_chunk_step(c, s, base, lane, n_items, nx, ny, n, bricked, bx, by)) continue;
        uint32_t mask = 0;
        if (no_rect || lasso_box_misses(rule, c.wl, c.wh)) {             // (uniform) nothing in the wave's box is inside
            if (!rule.outside) continue;
            mask = c.live ? c.keep : 0u;
        } else if (c.live) {
            if (lasso_box_misses(rule, c.cl, c.ch)) mask = rule.outside ? c.keep : 0u;
            else {
                uint32_t x = c.x0, y = c.y0, z = c.z0;
                const int64_t X0 = lasso_row(rule, 0, x, y, z), Y0 = lasso_row(rule, 1, x, y, z), D0 = lasso_row(rule, 2, x, y, z);
                int64_t X = X0, Y = Y0, D = D0;
#pragma unroll 1
                for (uint32_t j = 0; j < 16u; ++j) {
                    if (bricked) {
                        const int32_t jx = static_cast<int32_t>(2u * (j & 3u)), jy = static_cast<int32_t>(2u * (j >> 2));
                        X = X0 + static_cast<int64_t>(rule.m[0][0]) * jx + static_cast<int64_t>(rule.m[0][1]) * jy;
                        Y = Y0 + static_cast<int64_t>(rule.m[1][0]) * jx + static_cast<int64_t>(rule.m[1][1]) * jy;
                        D = D0 + static_cast<int64_t>(rule.m[2][0]) * jx + static_cast<int64_t>(rule.m[2][1]) * jy;
                    }
                    if ((c.keep & (1u << j)) && lasso_inside(rule, plane, X, Y, D) != (rule.outside != 0u)) mask |= 1u << j;
                    if (!bricked) {
                        if (++x == nx) {
                            x = 0u;
                            if (++y == ny) { y = 0u; ++z; }
                            X = lasso_row(rule, 0, x, y, z); Y = lasso_row(rule, 1, x, y, z); D = lasso_row(rule, 2, x, y, z);
                        } else {
                            X += 2 * static_cast<int64_t>(rule.m[0][0]); Y += 2 * static_cast<int64_t>(rule.m[1][0]); D += 2 * static_cast<int64_t>(rule.m[2][0]);
                        }
                    }
                }
            }
        }
        if (!mask) continue;                                             // before any load of labels or density
        selected_chunk_tail<JOURNAL>(sh, t, labels, vol, c.k, mask, windowed, rule.min_byte, rule.max_byte, rule.store, journal, nx, ny, bricked);
    }
    tally_reduce(sh, t, out);
}

__global__ __launch_bounds__(256) void volym_lasso_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ plane,
                                                          RelabelOut out, LabelTable to, CropSlab s, LassoRule rule, uint32_t nx, uint32_t ny, uint32_t nz,
                                                          uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    lasso_pass<false>(sh, labels, vol, plane, out, to, s, rule, LabelJournal{}, nx, ny, nz, bricked, n_items);
}

// the same lasso while the history is on and the request is no DRY_RUN
__global__ __launch_bounds__(256) void volym_lasso_journal_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ plane,
                                                                  RelabelOut out, LabelTable to, CropSlab s, LassoRule rule, LabelJournal journal, uint32_t nx,
                                                                  uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    lasso_pass<true>(sh, labels, vol, plane, out, to, s, rule, journal, nx, ny, nz, bricked, n_items);
}

}  // namespace volym
