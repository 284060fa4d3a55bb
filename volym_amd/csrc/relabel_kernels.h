// The kernels of the label edit (volym_edit_labels, volym_read_labels).  Included by scene_bytes.hip alone, after scene_kernels.h,
// whose chunk walk (CropSlab, crop_chunk) and chunk geometry (label_chunk_origin) they read; nothing in that header changes.
#pragma once

#include "scene_kernels.h"

namespace volym {

// what the rule reads beside the table: the window, the id range and the distance band, and the boxes the id volume and the map
// are linear in (the request's box lies inside each that is read: the host checks it)
struct RelabelRule {
    uint32_t min_byte, max_byte;
    uint32_t id_lo, id_hi, ids_except;
    uint32_t d2_lo, d2_hi;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t ids_box[6], map_box[6];
};

// The working result in device memory: volym_relabel_result as the kernel accumulates it.  The caller sets lo = 0xffffffff and
// hi = 0 (the INCLUSIVE maxima) and zeroes the counts; the host turns the hull into the result's box.
struct RelabelOut {
    unsigned long long* changed;    // [1]
    unsigned long long* left;       // [256]
    unsigned long long* arrived;    // [256]
    uint32_t* box;                  // [6]
};

// Does linear item i own its chunk k?  Two runs may share a chunk (scene_kernels.h).  The rewrite kernels do not mind: both lanes
// store the same bytes.  Here a lane stores bytes it derived from the labels it read, and counts them: a chunk must be visited
// once.  Its owner is the first run that touches it, and the owner decides every byte of the chunk that lies in the box.  The runs'
// first bytes ascend with the run number, so do their last chunks: an earlier run touches k iff the run before this one does.
__device__ __forceinline__ bool relabel_owns_chunk(const CropSlab& s, uint32_t i, uint32_t nx, uint32_t ny, uint64_t k)
{
    const uint32_t r = i / s.chunks_per_run;
    if (r == 0u) return true;
    const uint32_t p = r - 1u, ry = p % s.runs_y, rz = p / s.runs_y;
    const uint64_t start = s.lo[0] + static_cast<uint64_t>(nx) * ((s.lo[1] + ry) + static_cast<uint64_t>(ny) * (s.lo[2] + rz));
    return k > ((start + s.run_len - 1u) >> 4);
}

// index of texel (x, y, z) in a volume that is linear in box b = {x0, y0, z0, x1, y1, z1} (the id volume, the distance map: fewer
// than 2^31 texels)
__device__ __forceinline__ uint32_t box_linear(const uint32_t b[6], uint32_t x, uint32_t y, uint32_t z)
{
    return (x - b[0]) + (b[3] - b[0]) * ((y - b[1]) + (b[4] - b[1]) * (z - b[2]));
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) { const uint32_t w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) { const uint32_t w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

// One pass over the items of slab s (make_crop_slab over the request's box, s.box_lo/hi the box itself, no plane: keep names the
// texels of the box), in either layout.  Per chunk: the 16 labels first; a chunk in which no texel of the box has to[l] != l loads
// nothing more and stores nothing.  Else the 16 density bytes (vol: the scene bytes, or the uncut copy), then -- IDS, DISTANCE --
// the id and the distance of the texels that are still candidates, from the box-linear snapshots.  The chunk is stored, by a
// plain vector store, only if a byte changed and rule.store says so.  Labels are read and written by the chunk's one owner and
// everything else is only read: every texel is decided from the bytes before the edit.
//
// The result.  A lane counts its changed texels and keeps their hull in registers, and carries one run of equal old labels whose
// length it flushes when the label changes and once at the end.  At the end the waves add up first: changed and the hull by
// shuffles, and the runs too where the whole wave carries the same label (a merge of one segment: every lane) -- one LDS atomic per
// wave and word instead of 64 on the same word.  After the barrier thread l adds the workgroup's left[l] and arrived[l] to the
// global result and thread 0 the count and the hull: one global atomic per non-zero word and workgroup.  All integer adds and
// min/max: the result does not depend on arrival order.  A workgroup holds fewer texels than a layout has bytes (< 2^32): u32 in LDS.
template <bool IDS, bool DISTANCE>
__global__ __launch_bounds__(256) void volym_relabel_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ ids,
                                                            const uint32_t* __restrict__ dmap, RelabelOut out, LabelTable to, CropSlab s, RelabelRule rule,
                                                            uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ uint8_t s_to[256];
    __shared__ uint32_t s_left[256], s_arrived[256];
    __shared__ uint32_t s_changed, s_box[6];
    {
        const uint32_t l = threadIdx.x;
        s_to[l] = to.v[l];
        s_left[l] = s_arrived[l] = 0u;
        if (l == 0u) s_changed = 0u;
        if (l < 6u) s_box[l] = l < 3u ? 0xffffffffu : 0u;
    }
    __syncthreads();
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);

    uint32_t changed = 0, lo_x = 0xffffffffu, lo_y = 0xffffffffu, lo_z = 0xffffffffu, hi_x = 0, hi_y = 0, hi_z = 0;
    uint32_t cur = 256u, cnt = 0;                    // the run of equal old labels (256: none yet)
    auto flush = [&]() {
        if (cur > 255u) return;
        atomicAdd(&s_left[cur], cnt);
        atomicAdd(&s_arrived[s_to[cur]], cnt);
    };

    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        if (!bricked && !relabel_owns_chunk(s, i, nx, ny, k)) continue;
        if (!keep) continue;                                             // before any load
        const uint4 lv = labels[k];
        uint32_t lb[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t cand = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t l = (lb[j >> 2] >> (8u * (j & 3u))) & 0xffu;
            if (s_to[l] != l) cand |= 1u << j;
        }
        cand &= keep;
        if (!cand) continue;                                             // no density, no ids, no store
        const uint4 dv = vol[k];
        const uint32_t d[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t b = (d[j >> 2] >> (8u * (j & 3u))) & 0xffu;
            if (b < rule.min_byte || b > rule.max_byte) cand &= ~(1u << j);
        }
        if (!cand) continue;
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);      // (k < 2^28: a layout has fewer than 2^32 bytes)
        uint32_t x = x0, y = y0, z = z0;
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            if (bricked) { x = x0 + (j & 3u); y = y0 + (j >> 2); }
            if (cand & (1u << j)) {
                bool in = true;
                if (IDS) {
                    const uint32_t id = ids[box_linear(rule.ids_box, x, y, z)];
                    const bool ranged = id >= rule.id_lo && id <= rule.id_hi;
                    in = id != VOLYM_COMPONENT_NONE && (rule.ids_except ? !ranged : ranged);
                }
                if (DISTANCE && in) {
                    const uint32_t dd = dmap[box_linear(rule.map_box, x, y, z)];
                    in = dd != VOLYM_DISTANCE_NONE && dd >= rule.d2_lo && dd <= rule.d2_hi;
                }
                if (in) {
                    const uint32_t sh = 8u * (j & 3u), l = (lb[j >> 2] >> sh) & 0xffu;
                    lb[j >> 2] = (lb[j >> 2] & ~(0xffu << sh)) | (static_cast<uint32_t>(s_to[l]) << sh);
                    if (l != cur) { flush(); cur = l; cnt = 0u; }
                    ++cnt; ++changed;
                    lo_x = min(lo_x, x); lo_y = min(lo_y, y); lo_z = min(lo_z, z);
                    hi_x = max(hi_x, x); hi_y = max(hi_y, y); hi_z = max(hi_z, z);
                } else {
                    cand &= ~(1u << j);
                }
            }
            if (!bricked && ++x == nx) { x = 0u; if (++y == ny) { y = 0u; ++z; } }
        }
        if (cand && rule.store) labels[k] = make_uint4(lb[0], lb[1], lb[2], lb[3]);
    }

    // per wave, before LDS (every lane of the workgroup is here: the loop has ended for all)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w_changed = wave_sum(changed);
    if (w_changed != 0u) {                                               // (wave-uniform)
        const uint32_t a = wave_min(lo_x), b = wave_min(lo_y), c = wave_min(lo_z), d = wave_max(hi_x), e = wave_max(hi_y), f = wave_max(hi_z);
        const unsigned long long have = __ballot(cur < 256u);
        const uint32_t first = static_cast<uint32_t>(__ffsll(have)) - 1u;
        const uint32_t ref = __shfl(cur, static_cast<int>(first), 64);
        if (__all(cur > 255u || cur == ref)) {
            const uint32_t total = wave_sum(cur < 256u ? cnt : 0u);
            if (lane == first) { atomicAdd(&s_left[ref], total); atomicAdd(&s_arrived[s_to[ref]], total); }
        } else {
            flush();
        }
        if (lane == 0u) {
            atomicAdd(&s_changed, w_changed);
            atomicMin(&s_box[0], a); atomicMin(&s_box[1], b); atomicMin(&s_box[2], c);
            atomicMax(&s_box[3], d); atomicMax(&s_box[4], e); atomicMax(&s_box[5], f);
        }
    }
    __syncthreads();
    const uint32_t l = threadIdx.x;
    if (s_left[l] != 0u) atomicAdd(&out.left[l], static_cast<unsigned long long>(s_left[l]));
    if (s_arrived[l] != 0u) atomicAdd(&out.arrived[l], static_cast<unsigned long long>(s_arrived[l]));
    if (l == 0u && s_changed != 0u) {
        atomicAdd(out.changed, static_cast<unsigned long long>(s_changed));
        for (int a = 0; a < 3; ++a) atomicMin(&out.box[a], s_box[a]);
        for (int a = 3; a < 6; ++a) atomicMax(&out.box[a], s_box[a]);
    }
}

// out (box-linear, x fastest) = the labels of box b = {x0, y0, z0, x1, y1, z1}, read from the device layout: one thread per texel
__global__ __launch_bounds__(256) void volym_read_labels_kernel(const uint8_t* __restrict__ labels, uint8_t* __restrict__ out, uint32_t nx, uint32_t ny,
                                                                uint32_t bricked, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t w, uint32_t h, uint64_t total)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t x = x0 + static_cast<uint32_t>(i % w), y = y0 + static_cast<uint32_t>((i / w) % h), z = z0 + static_cast<uint32_t>(i / (static_cast<uint64_t>(w) * h));
    out[i] = labels[layout_offset(bricked != 0u, layout_bx(bricked != 0u, nx), layout_bxy(bricked != 0u, nx, ny), x, y, z)];
}

}  // namespace volym
