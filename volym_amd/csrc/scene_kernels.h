// The kernels of the scene-byte set-up path (scene_bytes.hip, the only unit that includes this header: a non-template
// __global__ function is defined in exactly one unit): macro-cell maxima, the bricked layout, importances mapped from a
// label volume, label statistics, and the crop box, clip plane and segment visibility rewrites of density and importances.
// The chunk geometry and the slab walk they share with the measure pass and the label edits are scene_chunks.h.
#pragma once

#include "scene_chunks.h"

namespace volym {

// per-cell maxima of the density volume: cell (cx,cy,cz) of the mc_n^3 grid covers the voxels a
// nearest-filter sample with pos in [c/mc_n, (c+1)/mc_n) can select, i.e. floor(pos*n) for those pos.
// One workgroup per cell of the range of cells `cells` = {x0, y0, z0, nx, ny, nz} (the whole grid, or the cells a crop edit touched).
struct CellRange { uint32_t c0[3], cn[3]; };
// voxel range [lo, hi) of cell c on an axis of n voxels, one voxel of slack on both sides (float rounding of pos*n)
__host__ __device__ inline uint32_t mc_voxel_lo(uint32_t c, uint32_t n, uint32_t mc_n)
{
    const uint32_t v = static_cast<uint32_t>((static_cast<uint64_t>(c) * n) / mc_n);
    return v > 0u ? v - 1u : 0u;
}
__host__ __device__ inline uint32_t mc_voxel_hi(uint32_t c, uint32_t n, uint32_t mc_n)
{
    const uint32_t v = static_cast<uint32_t>((static_cast<uint64_t>(c + 1u) * n + mc_n - 1u) / mc_n) + 1u;
    return v < n ? v : n;
}

__global__ __launch_bounds__(256) void volym_macrocell_kernel(const uint8_t* __restrict__ vol, uint8_t* __restrict__ mc_max,
                                                              uint32_t nx, uint32_t ny, uint32_t nz, uint32_t mc_n, uint32_t bricked, CellRange cells)
{
    const uint32_t cx = cells.c0[0] + blockIdx.x % cells.cn[0], cy = cells.c0[1] + (blockIdx.x / cells.cn[0]) % cells.cn[1],
                   cz = cells.c0[2] + blockIdx.x / (cells.cn[0] * cells.cn[1]);
    const uint32_t cell = (cz * mc_n + cy) * mc_n + cx;
    const uint32_t x0 = mc_voxel_lo(cx, nx, mc_n), x1 = mc_voxel_hi(cx, nx, mc_n), y0 = mc_voxel_lo(cy, ny, mc_n), y1 = mc_voxel_hi(cy, ny, mc_n),
                   z0 = mc_voxel_lo(cz, nz, mc_n), z1 = mc_voxel_hi(cz, nz, mc_n);
    const uint32_t wx = x1 - x0, wy = y1 - y0, wz = z1 - z0;
    const uint32_t total = wx * wy * wz;
    uint32_t m = 0;
    for (uint32_t i = threadIdx.x; i < total; i += 256u) {
        const uint32_t x = x0 + i % wx, y = y0 + (i / wx) % wy, z = z0 + i / (wx * wy);
        const uint32_t v = vol[layout_offset(bricked != 0u, layout_bx(bricked != 0u, nx), layout_bxy(bricked != 0u, nx, ny), x, y, z)];
        m = v > m ? v : m;
    }
    for (int s = 32; s > 0; s >>= 1) { const uint32_t o = __shfl_xor(m, s, 64); m = o > m ? o : m; }
    __shared__ uint32_t s_m[4];
    if ((threadIdx.x & 63u) == 0u) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t r = s_m[0];
        for (int w = 1; w < 4; ++w) r = s_m[w] > r ? s_m[w] : r;
        mc_max[cell] = static_cast<uint8_t>(r);
    }
}

// The same maxima for the finer grid of the per-view tile mask and depth bounds (volym_ctx::d_mc_fine): a cell of the fine_n^3 grid
// is defined as a macro cell is, by mc_voxel_lo / mc_voxel_hi with fine_n.  Its voxel range is a few voxels per axis (2 + 2 of
// slack at 256^3 and 128 cells), so one thread per cell of the range `cells`, x fastest: neighbouring lanes read neighbouring
// runs of a row.  An axis shorter than fine_n gives cells that share voxels, never an empty range (the loops would leave 0).
__global__ __launch_bounds__(256) void volym_fine_cell_kernel(const uint8_t* __restrict__ vol, uint8_t* __restrict__ fine_max,
                                                              uint32_t nx, uint32_t ny, uint32_t nz, uint32_t fine_n, uint32_t bricked, CellRange cells)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cells.cn[0] * cells.cn[1] * cells.cn[2]) return;
    const uint32_t cx = cells.c0[0] + i % cells.cn[0], cy = cells.c0[1] + (i / cells.cn[0]) % cells.cn[1], cz = cells.c0[2] + i / (cells.cn[0] * cells.cn[1]);
    const uint32_t x0 = mc_voxel_lo(cx, nx, fine_n), x1 = mc_voxel_hi(cx, nx, fine_n), y0 = mc_voxel_lo(cy, ny, fine_n), y1 = mc_voxel_hi(cy, ny, fine_n),
                   z0 = mc_voxel_lo(cz, nz, fine_n), z1 = mc_voxel_hi(cz, nz, fine_n);
    const uint32_t bx = layout_bx(bricked != 0u, nx), bxy = layout_bxy(bricked != 0u, nx, ny);
    uint32_t m = 0;
    for (uint32_t z = z0; z < z1; ++z)
        for (uint32_t y = y0; y < y1; ++y)
            for (uint32_t x = x0; x < x1; ++x) {
                const uint32_t v = vol[layout_offset(bricked != 0u, bx, bxy, x, y, z)];
                m = v > m ? v : m;
            }
    fine_max[(cz * fine_n + cy) * fine_n + cx] = static_cast<uint8_t>(m);
}

// linear (x fastest) staging copy -> 4x4x4 bricks; one thread per voxel of the padded grid
__global__ __launch_bounds__(256) void volym_rebrick_kernel(const uint8_t* __restrict__ linear, uint8_t* __restrict__ bricked,
                                                            uint32_t nx, uint32_t ny, uint32_t nz)
{
    const uint32_t bx = brick_count(nx), by = brick_count(ny), bz = brick_count(nz);
    const uint64_t total = static_cast<uint64_t>(bx) * by * bz * 64u;
    const uint64_t o = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (o >= total) return;
    const uint32_t brick = static_cast<uint32_t>(o >> 6), in = static_cast<uint32_t>(o & 63u);
    const uint32_t x = (brick % bx) * 4u + (in & 3u), y = ((brick / bx) % by) * 4u + ((in >> 2) & 3u), z = (brick / (bx * by)) * 4u + (in >> 4);
    uint8_t v = 0;
    if (x < nx && y < ny && z < nz) v = linear[static_cast<size_t>(x) + static_cast<size_t>(nx) * (y + static_cast<size_t>(ny) * z)];
    bricked[o] = v;
}

// ---- segment importances from a label volume on the device (volym_set_labels / volym_set_segment_importances) ----
// Both kernels walk the device layout of the labels in the 16-byte chunks of scene_chunks.h, one chunk per lane and step.
//
// imp[i] = table[labels[i]] for the voxels, 0 for the padding (what volym_rebrick_kernel leaves there): 16 bytes in, 16 out per
// lane, the table in LDS.  n_chunks = ceil(layout bytes / 16); both buffers hold n_chunks * 16 bytes (the allocations end 16
// bytes past the layout).  Grid-stride, two chunks in flight per lane.
__global__ __launch_bounds__(256) void volym_segment_map_kernel(const uint4* __restrict__ labels, uint4* __restrict__ imp, LabelTable table,
                                                                uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_chunks)
{
    __shared__ uint8_t s_tab[256];
    s_tab[threadIdx.x] = table.v[threadIdx.x];
    __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t stride = gridDim.x * 256u;
    auto map = [&](uint4 v, uint32_t inside) {
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (inside & (1u << (4 * j + b))) o |= static_cast<uint32_t>(s_tab[(w[j] >> (8 * b)) & 0xffu]) << (8 * b);
            w[j] = o;
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    };
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n_chunks; k += 2u * stride) {
        const uint32_t k2 = k + stride;
        const uint4 a = labels[k];
        const uint4 b = k2 < n_chunks ? labels[k2] : make_uint4(0u, 0u, 0u, 0u);
        imp[k] = map(a, label_chunk_inside(bricked != 0u, k, nx, ny, nz, n));
        if (k2 < n_chunks) imp[k2] = map(b, label_chunk_inside(bricked != 0u, k2, nx, ny, nz, n));
    }
}

// Voxel count and texel AABB of every label value, in the coordinates of the volume (x fastest), whatever the layout.
// stats: 256 u64 counts, then 256 x {x0, y0, z0, x1, y1, z1} (the caller initialises lo = INT_MAX, hi = -1).
// A lane carries one run of equal labels through its voxels and flushes it to LDS when the label changes; most voxels carry
// one or two labels, so the flushes are few.  Each workgroup then adds its LDS totals to the global ones once per label.
__global__ __launch_bounds__(256) void volym_label_stats_kernel(const uint4* __restrict__ labels, unsigned long long* __restrict__ counts,
                                                                int* __restrict__ boxes, uint32_t nx, uint32_t ny, uint32_t nz,
                                                                uint32_t bricked, uint32_t n_chunks)
{
    __shared__ uint32_t s_cnt[256];
    __shared__ int s_box[256 * 6];
    s_cnt[threadIdx.x] = 0u;
    for (int i = 0; i < 6; ++i) s_box[threadIdx.x * 6 + i] = i < 3 ? INT32_MAX : -1;
    __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    uint32_t cur = 256u, cnt = 0;                 // 256: no run yet
    int bx0 = 0, by0 = 0, bz0 = 0, bx1 = 0, by1 = 0, bz1 = 0;
    auto flush = [&]() {
        if (cur > 255u) return;
        atomicAdd(&s_cnt[cur], cnt);
        int* b = &s_box[cur * 6];
        atomicMin(&b[0], bx0); atomicMin(&b[1], by0); atomicMin(&b[2], bz0);
        atomicMax(&b[3], bx1); atomicMax(&b[4], by1); atomicMax(&b[5], bz1);
    };
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n_chunks; k += gridDim.x * 256u) {
        const uint4 v = labels[k];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t inside = label_chunk_inside(bricked != 0u, k, nx, ny, nz, n);
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, k, nx, ny, x0, y0, z0);
        int x = static_cast<int>(x0), y = static_cast<int>(y0), z = static_cast<int>(z0);
        for (uint32_t i = 0; i < 16u; ++i) {
            if (bricked) { x = static_cast<int>(x0 + (i & 3u)); y = static_cast<int>(y0 + (i >> 2)); }
            if (inside & (1u << i)) {
                const uint32_t l = (w[i >> 2] >> (8u * (i & 3u))) & 0xffu;
                if (l != cur) {
                    flush();
                    cur = l; cnt = 0;
                    bx0 = bx1 = x; by0 = by1 = y; bz0 = bz1 = z;
                }
                ++cnt;
                bx0 = min(bx0, x); bx1 = max(bx1, x); by0 = min(by0, y); by1 = max(by1, y); bz0 = min(bz0, z); bz1 = max(bz1, z);
            }
            if (!bricked && ++x == static_cast<int>(nx)) { x = 0; if (++y == static_cast<int>(ny)) { y = 0; ++z; } }
        }
    }
    flush();
    __syncthreads();
    const uint32_t l = threadIdx.x;
    if (s_cnt[l] != 0u) {
        atomicAdd(&counts[l], static_cast<unsigned long long>(s_cnt[l]));
        for (int i = 0; i < 3; ++i) atomicMin(&boxes[l * 6 + i], s_box[l * 6 + i]);
        for (int i = 3; i < 6; ++i) atomicMax(&boxes[l * 6 + i], s_box[l * 6 + i]);
    }
}

// ---- crop box on the device (volym_set_crop_box) -------------------------------------------------------------------------
// dst = inside(box) ? value(src) : 0 over one slab of texels, where value is the byte itself (density, uploaded importances) or
// table[byte] (src = the label volume).  16 bytes in, 16 out per lane and step, in either layout; a chunk that sticks out of the
// slab rewrites its other bytes by the same rule, which leaves them as they are (the host only hands slabs that cover every
// texel whose side of the box changes).  Padding stays 0: the box lies inside the volume.  The walk is scene_chunks.h's (CropSlab,
// crop_chunk); two linear runs may share a chunk: both lanes store the same 16 bytes.
template <bool TABLE>
__global__ __launch_bounds__(256) void volym_crop_slab_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, LabelTable table, CropSlab s,
                                                              uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ uint8_t s_tab[TABLE ? 256 : 1];      // (only the instantiation that maps labels holds the table)
    if (TABLE) {
        s_tab[threadIdx.x] = table.v[threadIdx.x];
        __syncthreads();
    }
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        dst[k] = keep ? crop_chunk_value<TABLE>(src[k], keep, s_tab) : make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- segment visibility on the device (volym_set_segment_visibility) ------------------------------------------------------
// dst = (inside(box) && visible[label]) ? value(src) : 0 over one box of texels, walked as volym_crop_slab_kernel walks a slab (same
// CropSlab, same items, both layouts).  `labels` has the dimensions and layout of src and dst.  TABLE: the labels are the source
// themselves (value = table[label], src is not read).  mask.v[l]: bit 0 = label l is visible, bit 1 = its visibility flipped in
// this edit.  The label chunk is read first; a chunk with no texel of a flipped label is neither loaded from src nor stored:
// dst already holds there what the rule gives (the host keeps it so, context.hpp).  A chunk that is stored is stored whole by the
// new rule, which leaves its other bytes as they are.  A crop edit under a mask runs this kernel over its slabs with every
// label marked flipped.  Both tables are a byte per label in LDS: a lane indexes them with its own label, which a mask held as
// eight dwords of kernel arguments (SGPRs) cannot serve without a select chain per byte.
template <bool TABLE>
__global__ __launch_bounds__(256) void volym_visibility_kernel(const uint4* __restrict__ labels, const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                               LabelTable table, LabelTable mask, CropSlab s, uint32_t nx, uint32_t ny, uint32_t nz,
                                                               uint32_t bricked, uint32_t n_items)
{
    __shared__ uint8_t s_mask[256];
    __shared__ uint8_t s_tab[TABLE ? 256 : 1];
    s_mask[threadIdx.x] = mask.v[threadIdx.x];
    if (TABLE) s_tab[threadIdx.x] = table.v[threadIdx.x];
    __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        const uint4 lv = labels[k];
        const uint32_t l[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t flipped = 0, visible = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t m = s_mask[(l[j >> 2] >> (8 * (j & 3))) & 0xffu];
            flipped |= m;
            visible |= (m & 1u) << j;
        }
        if (!(flipped & 2u)) continue;
        keep &= visible;
        dst[k] = keep ? crop_chunk_value<TABLE>(TABLE ? lv : src[k], keep, s_tab) : make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- clip plane on the device (volym_set_clip_plane) ------------------------------------------------------------------------
// dst = (inside(box) && kept by plane p && visible[label]) ? value(src) : 0 over the box of texels that planes q (before) and p
// (now) classify differently (volym_clip_plane_box), walked as the two kernels above walk theirs.  A chunk in which no texel
// inside the box changes side is neither loaded nor stored: dst already holds there what the rule gives -- the analogue of the
// visibility kernel's chunk without a flipped label.  A chunk that is stored is stored whole by the new rule.  MASKED: a segment
// is hidden, and the labels are read as volym_visibility_kernel reads them (mask.v[l] bit 0 = label l is visible).  TABLE: the
// labels are the source themselves (src == labels, value = table[label]).
template <bool TABLE, bool MASKED>
__global__ __launch_bounds__(256) void volym_clip_plane_kernel(const uint4* __restrict__ labels, const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                               LabelTable table, LabelTable mask, CropSlab s, uint32_t nx, uint32_t ny, uint32_t nz,
                                                               uint32_t bricked, uint32_t n_items)
{
    __shared__ uint8_t s_mask[MASKED ? 256 : 1];
    __shared__ uint8_t s_tab[TABLE ? 256 : 1];
    if (MASKED) s_mask[threadIdx.x] = mask.v[threadIdx.x];
    if (TABLE) s_tab[threadIdx.x] = table.v[threadIdx.x];
    if (MASKED || TABLE) __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<true>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        if (!moved) continue;
        uint4 lv = make_uint4(0u, 0u, 0u, 0u);
        if (keep && (MASKED || TABLE)) lv = labels[k];
        if (MASKED) {
            const uint32_t l[4] = {lv.x, lv.y, lv.z, lv.w};
            uint32_t visible = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) visible |= (s_mask[(l[j >> 2] >> (8 * (j & 3))) & 0xffu] & 1u) << j;
            keep &= visible;
        }
        dst[k] = keep ? crop_chunk_value<TABLE>(TABLE ? lv : src[k], keep, s_tab) : make_uint4(0u, 0u, 0u, 0u);
    }
}

}  // namespace volym
