// The kernels of the measure pass (volym_measure_pass): per-label statistics and grouped density histograms of the scene under its
// cuts.  Included by measure.hip alone; the chunk walk it reads (CropSlab, crop_chunk) is scene_chunks.h's.
#pragma once

#include "scene_chunks.h"

namespace volym {

// the result in device memory: struct volym_measurement, as the two arrays the kernels index
struct MeasureOut {
    volym_segment_stats* seg;           // [256]
    unsigned long long* hist;           // [VOLYM_MEASURE_GROUPS][256]
};

// the context's own result back to 256 empty records and zeroed histograms (one workgroup of 256 threads)
__global__ __launch_bounds__(256) void volym_measure_init_kernel(MeasureOut out)
{
    const uint32_t l = threadIdx.x;
    volym_segment_stats e = {};
    e.min = 255u; e.max = 0u;
    for (int i = 0; i < 6; ++i) e.box[i] = i < 3 ? INT32_MAX : -1;
    out.seg[l] = e;
    for (uint32_t g = 0; g < VOLYM_MEASURE_GROUPS; ++g) out.hist[g * 256u + l] = 0ull;
}

// `keep` of a linear item cut to the bytes of the item's own run.  chunks_per_run has a spare chunk and two runs may share a chunk;
// crop_chunk's keep covers all 16 bytes of the chunk, which the rewrite kernels do not mind (both lanes store the same bytes) and a
// counting kernel would count twice.  Every texel of a slab lies in exactly one run, so after this every texel is counted once.
__device__ __forceinline__ uint32_t measure_own_run(const CropSlab& s, uint32_t i, uint32_t nx, uint32_t ny, uint64_t k)
{
    const uint32_t r = i / s.chunks_per_run, ry = r % s.runs_y, rz = r / s.runs_y;
    const uint64_t start = s.lo[0] + static_cast<uint64_t>(nx) * ((s.lo[1] + ry) + static_cast<uint64_t>(ny) * (s.lo[2] + rz));
    const uint64_t o = k << 4, end = start + s.run_len;                // (crop_chunk returned true: o < end, and o + 16 > start)
    const uint32_t first = start > o ? static_cast<uint32_t>(start - o) : 0u;
    const uint32_t last = end - o < 16u ? static_cast<uint32_t>(end - o) : 16u;
    return ((1u << last) - 1u) & ~((1u << first) - 1u);
}

// One pass over the items of slab s (make_crop_slab over the request's box cut to the crop box; with UNCUT the request's box, no
// plane), 16 density bytes and, LABELS, 16 label bytes per lane and step, in either layout.  s.box_lo/hi is the slab itself: keep
// names exactly the texels that are in.  masked: a segment is hidden, and mask.v[l] bit 0 = label l is visible (as
// volym_visibility_kernel reads it).  group.v[l]: histogram group of label l, or VOLYM_MEASURE_NO_GROUP.
//
// A lane carries one run of equal labels and one run of equal (group, byte) through its texels and flushes each to LDS when it
// changes and once at the end: segments are contiguous and air is one byte, so the flushes are few and 64 lanes seldom meet in one
// LDS word.  After the barrier thread l adds the workgroup's record of label l and the bins b = l of every group to the global
// result.  All sums are integers: the result does not depend on arrival order.
//
// Widths.  The host launches at least ceil(n_items / (256 * MEASURE_ITEMS_PER_LANE)) workgroups (measure.hip), so a lane walks at
// most MEASURE_ITEMS_PER_LANE = 4096 items of at most 16 texels: 2^16 texels.
//   lane, u32:       count <= 2^16; sum <= 2^16 * 255 < 2^24; sum_sq <= 2^16 * 65025 = 4 261 478 400 < 2^32;
//                    coordinate sums <= 2^16 * 4095 < 2^28.
//   workgroup, LDS:  256 lanes, so at most 2^24 texels.  u32 is enough for count (2^24), sum (2^24 * 255 < 2^32) and a histogram
//                    bin (2^24); NOT for sum_sq (2^24 * 65025 ~ 2^40) nor for a coordinate sum (2^24 * 4095 ~ 2^36): those four
//                    are 64-bit in LDS.
//   global:          everything 64-bit but min, max and the box.
constexpr uint32_t MEASURE_ITEMS_PER_LANE = 4096u;

template <bool LABELS>
__global__ __launch_bounds__(256) void volym_measure_kernel(const uint4* __restrict__ vol, const uint4* __restrict__ labels, MeasureOut out,
                                                            LabelTable group, LabelTable mask, CropSlab s, uint32_t nx, uint32_t ny, uint32_t nz,
                                                            uint32_t bricked, uint32_t masked, uint32_t n_items)
{
    __shared__ uint32_t s_cnt[256], s_sum[256], s_min[256], s_max[256];           // (widths: see above)
    __shared__ unsigned long long s_sq[256], s_sx[256], s_sy[256], s_sz[256];
    __shared__ int s_box[256 * 6];
    __shared__ uint32_t s_hist[VOLYM_MEASURE_GROUPS * 256];
    __shared__ uint8_t s_group[256], s_mask[256];
    {
        const uint32_t l = threadIdx.x;
        s_cnt[l] = s_sum[l] = s_max[l] = 0u; s_min[l] = 255u;
        s_sq[l] = s_sx[l] = s_sy[l] = s_sz[l] = 0ull;
        for (int i = 0; i < 6; ++i) s_box[l * 6 + i] = i < 3 ? INT32_MAX : -1;
        for (uint32_t g = 0; g < VOLYM_MEASURE_GROUPS; ++g) s_hist[g * 256u + l] = 0u;
        s_group[l] = group.v[l];
        s_mask[l] = mask.v[l];
    }
    __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);

    // the run of equal labels (cur = 256: none yet) ...
    uint32_t cur = 256u, cur_group = VOLYM_MEASURE_NO_GROUP, cnt = 0, sum = 0, sq = 0, sx = 0, sy = 0, sz = 0, mn = 255u, mx = 0u;
    int bx0 = 0, by0 = 0, bz0 = 0, bx1 = 0, by1 = 0, bz1 = 0;
    // ... and the run of equal (group, byte): bin index g * 256 + b (>= 2048: none, or a label without a group)
    uint32_t hcur = 0xffffu, hcnt = 0;
    auto flush = [&]() {
        if (cur > 255u) return;
        atomicAdd(&s_cnt[cur], cnt); atomicAdd(&s_sum[cur], sum);
        atomicAdd(&s_sq[cur], static_cast<unsigned long long>(sq));
        atomicAdd(&s_sx[cur], static_cast<unsigned long long>(sx));
        atomicAdd(&s_sy[cur], static_cast<unsigned long long>(sy));
        atomicAdd(&s_sz[cur], static_cast<unsigned long long>(sz));
        atomicMin(&s_min[cur], mn); atomicMax(&s_max[cur], mx);
        int* b = &s_box[cur * 6];
        atomicMin(&b[0], bx0); atomicMin(&b[1], by0); atomicMin(&b[2], bz0);
        atomicMax(&b[3], bx1); atomicMax(&b[4], by1); atomicMax(&b[5], bz1);
    };
    auto flush_hist = [&]() {
        if (hcur < VOLYM_MEASURE_GROUPS * 256u) atomicAdd(&s_hist[hcur], hcnt);
    };

    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        if (!bricked) keep &= measure_own_run(s, i, nx, ny, k);
        if (!keep) continue;                                             // before any load
        const uint4 dv = vol[k];
        uint4 lv = make_uint4(0u, 0u, 0u, 0u);
        if (LABELS) lv = labels[k];
        const uint32_t d[4] = {dv.x, dv.y, dv.z, dv.w}, lb[4] = {lv.x, lv.y, lv.z, lv.w};
        if (LABELS && masked) {
            uint32_t visible = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) visible |= (s_mask[(lb[j >> 2] >> (8 * (j & 3))) & 0xffu] & 1u) << j;
            keep &= visible;
            if (!keep) continue;
        }
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);      // (k < 2^28: a layout has fewer than 2^32 bytes)
        int x = static_cast<int>(x0), y = static_cast<int>(y0);
        int z = static_cast<int>(z0);
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            if (bricked) { x = static_cast<int>(x0 + (j & 3u)); y = static_cast<int>(y0 + (j >> 2)); }
            if (keep & (1u << j)) {
                const uint32_t b = (d[j >> 2] >> (8u * (j & 3u))) & 0xffu;
                const uint32_t l = LABELS ? (lb[j >> 2] >> (8u * (j & 3u))) & 0xffu : 0u;
                if (l != cur) {
                    flush();
                    cur = l; cur_group = s_group[l];
                    cnt = sum = sq = sx = sy = sz = 0u; mn = 255u; mx = 0u;
                    bx0 = bx1 = x; by0 = by1 = y; bz0 = bz1 = z;
                }
                ++cnt; sum += b; sq += b * b;
                sx += static_cast<uint32_t>(x); sy += static_cast<uint32_t>(y); sz += static_cast<uint32_t>(z);
                mn = min(mn, b); mx = max(mx, b);
                bx0 = min(bx0, x); bx1 = max(bx1, x); by0 = min(by0, y); by1 = max(by1, y); bz0 = min(bz0, z); bz1 = max(bz1, z);
                const uint32_t bin = cur_group < VOLYM_MEASURE_GROUPS ? cur_group * 256u + b : 0xffffu;
                if (bin != hcur) { flush_hist(); hcur = bin; hcnt = 0u; }
                ++hcnt;
            }
            if (!bricked && ++x == static_cast<int>(nx)) { x = 0; if (++y == static_cast<int>(ny)) { y = 0; ++z; } }
        }
    }
    flush();
    flush_hist();
    __syncthreads();
    const uint32_t l = threadIdx.x;
    if (s_cnt[l] != 0u) {
        volym_segment_stats* g = &out.seg[l];
        atomicAdd(reinterpret_cast<unsigned long long*>(&g->count), static_cast<unsigned long long>(s_cnt[l]));
        atomicAdd(reinterpret_cast<unsigned long long*>(&g->sum), static_cast<unsigned long long>(s_sum[l]));
        atomicAdd(reinterpret_cast<unsigned long long*>(&g->sum_sq), s_sq[l]);
        atomicAdd(reinterpret_cast<unsigned long long*>(&g->sum_x), s_sx[l]);
        atomicAdd(reinterpret_cast<unsigned long long*>(&g->sum_y), s_sy[l]);
        atomicAdd(reinterpret_cast<unsigned long long*>(&g->sum_z), s_sz[l]);
        for (int i = 0; i < 3; ++i) atomicMin(&g->box[i], s_box[l * 6 + i]);
        for (int i = 3; i < 6; ++i) atomicMax(&g->box[i], s_box[l * 6 + i]);
        atomicMin(&g->min, s_min[l]); atomicMax(&g->max, s_max[l]);
    }
    for (uint32_t g = 0; g < VOLYM_MEASURE_GROUPS; ++g) {
        const uint32_t h = s_hist[g * 256u + l];
        if (h != 0u) atomicAdd(&out.hist[g * 256u + l], static_cast<unsigned long long>(h));
    }
}

}  // namespace volym
