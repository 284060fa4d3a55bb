// The kernel of the brush (volym_brush_labels): the label edit whose texels are decided by geometry, not by a snapshot.  Included by
// scene_bytes.hip alone, AFTER relabel_kernels.h, which this header does not include itself (scene_bytes.hip stays the one place
// that does): it relies on that header's RelabelShared, RelabelTally, RelabelOut and LabelJournal, on tally_init, tally_texel and
// tally_reduce, on relabel_owns_chunk and on wave_min / wave_max, and through it on scene_kernels.h (CropSlab, crop_chunk,
// label_chunk_origin, LabelTable).
#pragma once

#include "scene_kernels.h"

namespace volym {

// One segment of the stroke as the host lays it out (brush.inc): its end points (a == b: a ball), the box of texels that can lie
// within it (the end points' box grown by the brush's reach per axis and clipped to the volume; hi INCLUSIVE), <d,d> and r2 * <d,d>.
// 64 bytes, read by the uniform loop index: one scalar load per segment and wave, no vector register holds any of it.
struct BrushSegment {
    uint32_t a[3], b[3];
    uint32_t lo[3], hi[3];
    uint32_t dd;
    uint32_t r2dd_lo, r2dd_hi;
    uint32_t pad;
};
static_assert(sizeof(BrushSegment) == 64, "BrushSegment is 64 bytes");

struct BrushRule {
    uint32_t min_byte, max_byte;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t n_segments;
    uint32_t r2;
    uint32_t weight[3];
};

// Does texel (x, y, z) lie within segment g?  The rule of include/volym_hip.h, exact in unsigned 64-bit arithmetic: every inner
// product is below 2^32 (each of its three terms below 2^31, so the signed terms of <w,d> fit an int32 and their sum an int64).
__device__ __forceinline__ bool brush_within(const BrushSegment& g, const BrushRule& rule, uint32_t x, uint32_t y, uint32_t z)
{
    const int32_t wx = static_cast<int32_t>(x - g.a[0]), wy = static_cast<int32_t>(y - g.a[1]), wz = static_cast<int32_t>(z - g.a[2]);
    const uint32_t ww = rule.weight[0] * static_cast<uint32_t>(wx * wx) + rule.weight[1] * static_cast<uint32_t>(wy * wy) + rule.weight[2] * static_cast<uint32_t>(wz * wz);
    if (g.dd == 0u) return ww <= rule.r2;                                // (wave-uniform)
    const int32_t dx = static_cast<int32_t>(g.b[0] - g.a[0]), dy = static_cast<int32_t>(g.b[1] - g.a[1]), dz = static_cast<int32_t>(g.b[2] - g.a[2]);
    const int64_t wd = static_cast<int64_t>(static_cast<int32_t>(rule.weight[0]) * dx * wx) + static_cast<int64_t>(static_cast<int32_t>(rule.weight[1]) * dy * wy) +
                       static_cast<int64_t>(static_cast<int32_t>(rule.weight[2]) * dz * wz);
    if (wd <= 0) return ww <= rule.r2;
    if (wd >= static_cast<int64_t>(g.dd)) {
        const int32_t ux = wx - dx, uy = wy - dy, uz = wz - dz;
        return rule.weight[0] * static_cast<uint32_t>(ux * ux) + rule.weight[1] * static_cast<uint32_t>(uy * uy) + rule.weight[2] * static_cast<uint32_t>(uz * uz) <= rule.r2;
    }
    const uint64_t p = static_cast<uint64_t>(wd), r2dd = g.r2dd_lo | (static_cast<uint64_t>(g.r2dd_hi) << 32);
    return static_cast<uint64_t>(ww) * g.dd - p * p <= r2dd;             // (>= 0 by Cauchy-Schwarz)
}

// One pass over the items of slab s (make_crop_slab over the request's box cut to the stroke's hull, s.box_lo/hi that box, no plane),
// in either layout, a wave at a time: the loop's trip count is the wave's, because the segment cull below talks across its lanes.
// Per chunk, geometry first -- it needs no memory:
//   1. crop_chunk and, linear, the one-owner test of the relabel kernel;
//   2. the 16-bit mask of the chunk's texels that lie within some segment.  The box of the wave's 64 chunks (wave_min / wave_max,
//      then scalar) is held against each segment's box first: a segment that misses it is skipped by a uniform branch.  Then the
//      lane's chunk box against the segment's, then each texel against it, and only then the 64-bit test;
//   3. only if that mask is non-zero, the 16 labels and to[l] != l;
//   4. only then the density, skipped by a uniform test when the window is 0..255;
//   5. tally_texel, the journal append and the plain 16-byte store exactly as relabel_pass does them.
// Every texel is decided once, by its chunk's owner, from the bytes before the edit: the mask is the union over the segments.
template <bool JOURNAL>
__device__ __forceinline__ void brush_pass(RelabelShared& sh, uint4* __restrict__ labels, const uint4* __restrict__ vol, const BrushSegment* __restrict__ segs,
                                           const RelabelOut& out, const LabelTable& to, const CropSlab& s, const BrushRule& rule, const LabelJournal& journal,
                                           uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    sh.to[threadIdx.x] = to.v[threadIdx.x];
    tally_init(sh);
    __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const bool windowed = rule.min_byte > 0u || rule.max_byte < 255u;   // (uniform)
    RelabelTally t;

    for (uint32_t base = blockIdx.x * 256u + wave * 64u; base < n_items; base += gridDim.x * 256u) {
        const uint32_t i = base + lane;
        uint64_t k = 0;
        uint32_t keep = 0, moved;
        bool live = i < n_items && crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved);
        if (live && !bricked && !relabel_owns_chunk(s, i, nx, ny, k)) live = false;
        if (!keep) live = false;
        // the chunk's texel box (hi inclusive): a brick's 4 x 4 patch of one z; linear, 16 texels that may wrap rows and slices, whose
        // box is then taken a little wide (whole rows, whole slices): it only culls
        uint32_t x0 = 0, y0 = 0, z0 = 0, cl[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, ch[3] = {0u, 0u, 0u};
        if (live) {
            label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);   // (k < 2^28: a layout has fewer than 2^32 bytes)
            cl[0] = x0; cl[1] = y0; cl[2] = ch[2] = z0;
            if (bricked) { ch[0] = x0 + 3u; ch[1] = y0 + 3u; }
            else if (x0 + 15u < nx) { ch[0] = x0 + 15u; ch[1] = y0; }
            else {
                const uint32_t rows = (x0 + 15u) / nx;
                cl[0] = 0u; ch[0] = nx - 1u; ch[1] = y0 + rows;
                if (ch[1] >= ny) { cl[1] = 0u; ch[1] = ny - 1u; ch[2] = z0 + (y0 + rows) / ny; }
            }
        }
        uint32_t wl[3], wh[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            wl[a] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_min(cl[a]))));
            wh[a] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_max(ch[a]))));
        }
        if (wl[0] > wh[0]) continue;                                     // (uniform: no lane of the wave has a chunk)
        uint32_t mask = 0;
        for (uint32_t g = 0; g < rule.n_segments; ++g) {
            const BrushSegment seg = segs[g];
            if (seg.lo[0] > wh[0] || seg.hi[0] < wl[0] || seg.lo[1] > wh[1] || seg.hi[1] < wl[1] || seg.lo[2] > wh[2] || seg.hi[2] < wl[2]) continue;   // (uniform)
            if (!live || seg.lo[0] > ch[0] || seg.hi[0] < cl[0] || seg.lo[1] > ch[1] || seg.hi[1] < cl[1] || seg.lo[2] > ch[2] || seg.hi[2] < cl[2]) continue;
            uint32_t x = x0, y = y0, z = z0;
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                if (bricked) { x = x0 + (j & 3u); y = y0 + (j >> 2); }
                if ((keep & ~mask & (1u << j)) && x >= seg.lo[0] && x <= seg.hi[0] && y >= seg.lo[1] && y <= seg.hi[1] && z >= seg.lo[2] && z <= seg.hi[2] &&
                    brush_within(seg, rule, x, y, z))
                    mask |= 1u << j;
                if (!bricked && ++x == nx) { x = 0u; if (++y == ny) { y = 0u; ++z; } }
            }
        }
        if (!mask) continue;                                             // before any load
        const uint4 lv = labels[k];
        uint32_t lb[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t cand = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t l = (lb[j >> 2] >> (8u * (j & 3u))) & 0xffu;
            if (sh.to[l] != l) cand |= 1u << j;
        }
        cand &= mask;
        if (!cand) continue;                                             // no density, no store
        if (windowed) {
            const uint4 dv = vol[k];
            const uint32_t d[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                const uint32_t b = (d[j >> 2] >> (8u * (j & 3u))) & 0xffu;
                if (b < rule.min_byte || b > rule.max_byte) cand &= ~(1u << j);
            }
            if (!cand) continue;
        }
        uint32_t x = x0, y = y0, z = z0;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            if (bricked) { x = x0 + (j & 3u); y = y0 + (j >> 2); }
            if (cand & (1u << j)) {
                const uint32_t shift = 8u * (j & 3u), l = (lb[j >> 2] >> shift) & 0xffu, becomes = sh.to[l];
                lb[j >> 2] = (lb[j >> 2] & ~(0xffu << shift)) | (becomes << shift);
                tally_texel(sh, t, l, becomes, x, y, z);
            }
            if (!bricked && ++x == nx) { x = 0u; if (++y == ny) { y = 0u; ++z; } }
        }
        if (rule.store) {
            if (JOURNAL) {
                const unsigned long long here = __ballot(1);             // the lanes that store a chunk in this step
                const uint32_t leader = static_cast<uint32_t>(__ffsll(here)) - 1u;
                uint32_t first = 0u;
                if (lane == leader) first = atomicAdd(journal.count, static_cast<uint32_t>(__popcll(here)));
                first = __shfl(first, static_cast<int>(leader), 64);
                const uint32_t at = first + static_cast<uint32_t>(__popcll(here & ((1ull << lane) - 1ull)));
                if (at < journal.capacity) { journal.index[at] = static_cast<uint32_t>(k); journal.old[at] = lv; }
            }
            labels[k] = make_uint4(lb[0], lb[1], lb[2], lb[3]);
        }
    }
    tally_reduce(sh, t, out);
}

__global__ __launch_bounds__(256) void volym_brush_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const BrushSegment* __restrict__ segs,
                                                          RelabelOut out, LabelTable to, CropSlab s, BrushRule rule, uint32_t nx, uint32_t ny, uint32_t nz,
                                                          uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    brush_pass<false>(sh, labels, vol, segs, out, to, s, rule, LabelJournal{}, nx, ny, nz, bricked, n_items);
}

// the same stroke while the history is on and the request is no DRY_RUN
__global__ __launch_bounds__(256) void volym_brush_journal_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const BrushSegment* __restrict__ segs,
                                                                  RelabelOut out, LabelTable to, CropSlab s, BrushRule rule, LabelJournal journal, uint32_t nx,
                                                                  uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    brush_pass<true>(sh, labels, vol, segs, out, to, s, rule, journal, nx, ny, nz, bricked, n_items);
}

}  // namespace volym
