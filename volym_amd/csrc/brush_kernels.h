// The kernel of the brush (volym_brush_labels): the label edit whose texels are decided by geometry, not by a snapshot.  Included by
// brush.hip alone.  Everything but the selection rule is edit_chunks.h's: the walk (wave_chunk_step), the tail (selected_chunk_tail), the
// prologue, the tally and the journal.  Here: the segment, the rule of one texel against it, and the mask of a chunk.
#pragma once

#include "edit_chunks.h"

namespace volym {

// One segment of the stroke as the host lays it out (brush.hip): its end points (a == b: a ball), the box of texels that can lie
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
// in either layout: the walk and the tail of edit_chunks.h (wave_chunk_step, selected_chunk_tail) around the brush's selection
// rule, the 16-bit mask of the chunk's texels that lie within some segment -- their union, so every texel is decided once.  Three
// levels of cull: the wave's box is held against each segment's box first, and a segment that misses it is skipped by a uniform
// branch; then the lane's chunk box against the segment's; then each texel against it, and only then the 64-bit test.
template <bool JOURNAL>
__device__ __forceinline__ void brush_pass(RelabelShared& sh, uint4* __restrict__ labels, const uint4* __restrict__ vol, const BrushSegment* __restrict__ segs,
                                           const RelabelOut& out, const LabelTable& to, const CropSlab& s, const BrushRule& rule, const LabelJournal& journal,
                                           uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    edit_prologue(sh, to);
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const bool windowed = rule.min_byte > 0u || rule.max_byte < 255u;   // (uniform)
    RelabelTally t;

    for (uint32_t base = blockIdx.x * 256u + wave * 64u; base < n_items; base += gridDim.x * 256u) {
        WaveChunk c;
        if (!wave_chunk_step(c, s, base, lane, n_items, nx, ny, n, bricked, bx, by)) continue;
        uint32_t mask = 0;
        for (uint32_t g = 0; g < rule.n_segments; ++g) {
            const BrushSegment seg = segs[g];
            if (seg.lo[0] > c.wh[0] || seg.hi[0] < c.wl[0] || seg.lo[1] > c.wh[1] || seg.hi[1] < c.wl[1] || seg.lo[2] > c.wh[2] || seg.hi[2] < c.wl[2]) continue;   // (uniform)
            if (!c.live || seg.lo[0] > c.ch[0] || seg.hi[0] < c.cl[0] || seg.lo[1] > c.ch[1] || seg.hi[1] < c.cl[1] || seg.lo[2] > c.ch[2] || seg.hi[2] < c.cl[2]) continue;
            // (stepped by hand, not by a ChunkCursor: with one here the compiler spills the segment's scalar registers inside the unrolled loop)
            uint32_t x = c.x0, y = c.y0, z = c.z0;
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                if (bricked) { x = c.x0 + (j & 3u); y = c.y0 + (j >> 2); }
                if ((c.keep & ~mask & (1u << j)) && x >= seg.lo[0] && x <= seg.hi[0] && y >= seg.lo[1] && y <= seg.hi[1] && z >= seg.lo[2] && z <= seg.hi[2] &&
                    brush_within(seg, rule, x, y, z))
                    mask |= 1u << j;
                if (!bricked && ++x == nx) { x = 0u; if (++y == ny) { y = 0u; ++z; } }
            }
        }
        if (!mask) continue;                                             // before any load
        selected_chunk_tail<JOURNAL>(sh, t, labels, vol, c.k, mask, windowed, rule.min_byte, rule.max_byte, rule.store, journal, nx, ny, bricked);
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
