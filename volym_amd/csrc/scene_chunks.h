// The 16-byte chunks of a volume in the device layout, and the walk over the chunks of a slab of texels: what the kernels of the
// scene-byte set-up path (scene_kernels.h), of the measure pass (measure_kernels.h) and of the label edits (edit_chunks.h and the
// headers built on it) share.  Device functions and the structs they read only: no __global__ function, so any unit may include it.
#pragma once

#include "raymarch_device.h"

namespace volym {

// ---- chunk geometry ---------------------------------------------------------------------------------------------------------
// The kernels that stream a label volume walk its device layout (linear, or the 4x4x4 bricks of volym_rebrick_kernel) in 16-byte
// chunks, one chunk per lane and step.  Byte b of chunk k is a voxel of the volume or padding: linear, bytes past the last voxel;
// bricked, the bytes of a brick outside nx x ny x nz.  In a bricked chunk z is fixed and (x, y) is a 4x4 patch.
struct LabelTable { uint8_t v[256]; };

__device__ __forceinline__ void label_chunk_origin(bool bricked, uint32_t k, uint32_t nx, uint32_t ny, uint32_t& x, uint32_t& y, uint32_t& z)
{
    if (bricked) {
        const uint32_t bx = brick_count(nx), by = brick_count(ny), brick = k >> 2;
        x = (brick % bx) * 4u; y = ((brick / bx) % by) * 4u; z = (brick / (bx * by)) * 4u + (k & 3u);
    } else {
        const uint32_t o = k * 16u, slab = nx * ny;
        z = o / slab; y = (o - z * slab) / nx; x = o - z * slab - y * nx;
    }
}

// bit b set: byte b of chunk k is a voxel of the volume
__device__ __forceinline__ uint32_t label_chunk_inside(bool bricked, uint32_t k, uint32_t nx, uint32_t ny, uint32_t nz, uint64_t n)
{
    if (!bricked) {
        const uint64_t o = static_cast<uint64_t>(k) * 16u;
        return o + 16u <= n ? 0xffffu : (1u << static_cast<uint32_t>(n - o)) - 1u;
    }
    uint32_t x, y, z;
    label_chunk_origin(true, k, nx, ny, x, y, z);
    if (z >= nz) return 0u;
    const uint32_t wx = nx - x < 4u ? nx - x : 4u, wy = ny - y < 4u ? ny - y : 4u;
    const uint32_t row = (1u << wx) - 1u;
    uint32_t m = 0;
    for (uint32_t r = 0; r < wy; ++r) m |= row << (4u * r);
    return m;
}

// ---- the walk over a slab ---------------------------------------------------------------------------------------------------
// One slab of texels as 16-byte chunks, 16 bytes per lane and step, in either layout; a chunk that sticks out of the slab carries
// its other bytes along (`keep` says which bytes are texels of the box).
//   bricked: the slab widened to whole bricks; item i is chunk (i & 3) of brick (i >> 2) of that brick range (chunks whose z is
//            outside the slab are skipped), so neighbouring lanes write neighbouring chunks;
//   linear:  the slab as runs of consecutive bytes (a row of the slab; whole rows merge into one run per z, whole slices into a
//            single run -- the host decides), each covered by the aligned chunks it touches.  Two runs may share a chunk.
struct CropSlab {
    uint32_t lo[3], hi[3];          // the slab, texels
    uint32_t box_lo[3], box_hi[3];  // the box the bytes are cropped to
    uint32_t run_len, runs_y, runs_z, chunks_per_run;   // linear walk: runs_y * runs_z runs of run_len bytes
    uint32_t b_lo[3], b_n[3];       // bricked walk: first brick and bricks per axis
    // clip plane: texel (x, y, z) is kept iff pn . (x, y, z) <= pd; n = (0, 0, 0), d = 0 keeps every texel.  |n| <= 4096 and
    // coordinates <= 4099 (a brick's padding; a linear chunk past the last voxel reaches z = nz <= 4096), so
    // |n . t| <= 3 * 4096 * 4099 < 2^31: the sum is exact in 32 bits.
    int32_t pn[3], pd;              // the plane the bytes are clipped to
    int32_t qn[3], qd;              // the plane they were clipped to before (volym_clip_plane_kernel only)
    uint32_t planes;                // 0: neither plane cuts, and the term is not evaluated
};

__device__ __forceinline__ int32_t plane_sum(const int32_t n[3], uint32_t x, uint32_t y, uint32_t z)
{
    return n[0] * static_cast<int32_t>(x) + n[1] * static_cast<int32_t>(y) + n[2] * static_cast<int32_t>(z);
}

// bit 4 * r + j: texel (x0 + j, y0 + r, z) is kept by plane (n, d)
__device__ __forceinline__ uint32_t plane_side_4x4(const int32_t n[3], int32_t d, uint32_t x0, uint32_t y0, uint32_t z)
{
    int32_t row = plane_sum(n, x0, y0, z);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        int32_t t = row;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) { if (t <= d) m |= 1u << (4u * r + j); t += n[0]; }
        row += n[1];
    }
    return m;
}

// Item i of the walk over slab s: its chunk k and `keep` (bit b: byte b of the chunk is a texel inside the box and on the kept
// side of plane p).  MOVED: also `moved` (bit b: byte b is a texel inside the box that planes p and q classify differently).
// False: the item has no chunk (a bricked chunk whose z is outside the slab, the spare chunk of a linear run).
template <bool MOVED>
__device__ inline bool crop_chunk(const CropSlab& s, uint32_t i, uint32_t nx, uint32_t ny, uint64_t n, uint32_t bricked, uint32_t bx, uint32_t by,
                                  uint64_t& k, uint32_t& keep, uint32_t& moved)
{
    uint32_t inbox = 0, side_p = 0xffffu, side_q = 0xffffu;
    keep = moved = 0;
    if (bricked) {
        const uint32_t zz = i & 3u, b = i >> 2;
        const uint32_t bxi = s.b_lo[0] + b % s.b_n[0], byi = s.b_lo[1] + (b / s.b_n[0]) % s.b_n[1], bzi = s.b_lo[2] + b / (s.b_n[0] * s.b_n[1]);
        const uint32_t z = bzi * 4u + zz;
        if (z < s.lo[2] || z >= s.hi[2]) return false;
        k = (static_cast<uint64_t>(bzi) * by + byi) * bx + bxi;
        k = k * 4u + zz;
        if (z >= s.box_lo[2] && z < s.box_hi[2]) {
            uint32_t row = 0;
            for (uint32_t j = 0; j < 4u; ++j) { const uint32_t x = bxi * 4u + j; if (x >= s.box_lo[0] && x < s.box_hi[0]) row |= 1u << j; }
            for (uint32_t r = 0; r < 4u; ++r) { const uint32_t y = byi * 4u + r; if (y >= s.box_lo[1] && y < s.box_hi[1]) inbox |= row << (4u * r); }
            if (s.planes && inbox) {
                side_p = plane_side_4x4(s.pn, s.pd, bxi * 4u, byi * 4u, z);
                if (MOVED) side_q = plane_side_4x4(s.qn, s.qd, bxi * 4u, byi * 4u, z);
            }
        }
    } else {
        const uint32_t ci = i % s.chunks_per_run, r = i / s.chunks_per_run;
        const uint32_t ry = r % s.runs_y, rz = r / s.runs_y;
        const uint64_t start = s.lo[0] + static_cast<uint64_t>(nx) * ((s.lo[1] + ry) + static_cast<uint64_t>(ny) * (s.lo[2] + rz));
        k = (start >> 4) + ci;
        if ((k << 4) >= start + s.run_len) return false;
        const uint64_t o = k << 4, slice = static_cast<uint64_t>(nx) * ny;
        uint32_t z = static_cast<uint32_t>(o / slice);
        const uint32_t rem = static_cast<uint32_t>(o - z * slice);
        uint32_t y = rem / nx, x = rem - y * nx;
        if (!s.planes) {
            for (uint32_t j = 0; j < 16u; ++j) {
                if (o + j < n && x >= s.box_lo[0] && x < s.box_hi[0] && y >= s.box_lo[1] && y < s.box_hi[1] && z >= s.box_lo[2] && z < s.box_hi[2]) inbox |= 1u << j;
                if (++x == nx) { x = 0; if (++y == ny) { y = 0; ++z; } }
            }
        } else {
            // the chunk may wrap a row (and a slice): the running sums step by n[0] with x and start over with the row
            int32_t tp = plane_sum(s.pn, x, y, z), tq = MOVED ? plane_sum(s.qn, x, y, z) : 0;
            side_p = side_q = 0;
            for (uint32_t j = 0; j < 16u; ++j) {
                if (o + j < n && x >= s.box_lo[0] && x < s.box_hi[0] && y >= s.box_lo[1] && y < s.box_hi[1] && z >= s.box_lo[2] && z < s.box_hi[2]) inbox |= 1u << j;
                if (tp <= s.pd) side_p |= 1u << j;
                if (MOVED && tq <= s.qd) side_q |= 1u << j;
                tp += s.pn[0];
                if (MOVED) tq += s.qn[0];
                if (++x == nx) {
                    x = 0;
                    if (++y == ny) { y = 0; ++z; }
                    tp = plane_sum(s.pn, x, y, z);
                    if (MOVED) tq = plane_sum(s.qn, x, y, z);
                }
            }
        }
    }
    keep = inbox & side_p;
    if (MOVED) moved = inbox & (side_p ^ side_q);
    return true;
}

// the bytes of chunk v that `keep` names, each through the table (TABLE) or as it is; the others 0
template <bool TABLE>
__device__ inline uint4 crop_chunk_value(uint4 v, uint32_t keep, const uint8_t* s_tab)
{
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t o = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (!(keep & (1u << (4 * j + b)))) continue;
            const uint32_t byte = (w[j] >> (8 * b)) & 0xffu;
            o |= (TABLE ? static_cast<uint32_t>(s_tab[byte & (TABLE ? 255u : 0u)]) : byte) << (8 * b);
        }
        w[j] = o;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace volym
