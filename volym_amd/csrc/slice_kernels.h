// Kernel of the slice pass (gfx950): a plane through the volume that shows the bytes of the scene themselves -- density, transfer
// function or importance -- with the segments as a colour overlay and the texels the cuts remove marked.  Integer only; the host
// twin is scene.slice_frame (volym_amd/scene.py) and agrees on every byte.  (slice.hip, the only unit that includes this header.)
//
// The launch shape is the pick kernel's: one 256-thread workgroup per 16x16 pixel block, one wave64 per 8x8 block, one lane per
// output pixel.  A slice is an affine map of pixels to texels, so the 8x8 pixels of a wave land on an 8x8 patch of a plane through
// the volume: for any orientation its byte gathers stay inside few 64-byte bricks (bricked) or few rows (linear), as a wave's rays
// do in the march.  Per pixel: an address, up to three byte loads (density or importance, label), two integer blends, one dword
// store.  Palette and transfer function arrive as kernel arguments (SliceArgs is about 2.3 KiB) and are staged in LDS, where a
// lane's data-dependent index costs one ds_read.
//
//   BRICK    layout of the density (GridT<BRICK>); labels and importances take their own layouts at run time, as the pick kernel's
//            label fetch does.  mode and flags are uniform, so every branch on them is.
#pragma once

#include "raymarch_device.h"

namespace volym {

enum : uint32_t { SLICE_LABELS = 2u, SLICE_MARK_CUT = 4u };      // VOLYM_SLICE_LABELS, VOLYM_SLICE_MARK_CUT (UNCUT chooses `vol` on the host)

struct SliceArgs {
    const uint8_t* vol;            // d_vol, or the uncut copy with VOLYM_SLICE_UNCUT
    const uint8_t* imp;            // mode IMPORTANCE: d_imp
    const uint8_t* labels;         // NULL: no labels with the volume's dimensions on the device (the host refuses LABELS then)
    uint32_t* out;                 // width * height rgba8, row-major
    uint32_t origin[3], du[3], dv[3];   // 16.16, two's complement
    uint32_t width, height;
    uint32_t tiles_x;              // 16x16 blocks per row of the output
    uint32_t nx, ny, nz;
    uint32_t mode, flags;
    uint32_t imp_bricked, labels_bricked;
    uint32_t tf_n;
    uint32_t background, cut;      // rgba8 as the output holds it: r in the low byte
    uint32_t crop_lo[3], crop_hi[3];
    int32_t clip_n[3], clip_d;     // (0, 0, 0), 0: no plane -- 0 > 0 removes nothing
    uint32_t hidden[8];            // seg_hidden[l] != 0 as bit l
    uint32_t palette[256];         // LABELS
    uint32_t lut[256];             // TF: the table volym_set_transfer_function received
};
static_assert(sizeof(SliceArgs) < 4096, "palette and table travel with the launch: kernel arguments stay below 4 KiB");

// the outline's blend (include/volym_hip.h at volym_outline): out[c] = (src[c] * (255 - A) + col[c] * A + 127) / 255 for r, g, b, and
// 255 for col in the alpha byte
__device__ __forceinline__ uint32_t slice_blend(uint32_t src, uint32_t col)
{
    const uint32_t A = col >> 24, B = 255u - A;
    uint32_t out = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        const uint32_t s = (src >> (8u * c)) & 0xffu, v = c == 3u ? 255u : (col >> (8u * c)) & 0xffu;
        out |= ((s * B + v * A + 127u) / 255u) << (8u * c);
    }
    return out;
}

template <bool BRICK>
__global__ __launch_bounds__(256) void volym_slice_kernel(const SliceArgs a)
{
    __shared__ uint32_t s_pal[256];
    __shared__ uint32_t s_lut[256];
    __shared__ uint32_t s_hidden[8];

    const bool tf = a.mode == 1u, importance = a.mode == 2u;
    const bool overlay = (a.flags & SLICE_LABELS) != 0u, mark = (a.flags & SLICE_MARK_CUT) != 0u;
    {
        const uint32_t i = threadIdx.x;
        if (overlay) s_pal[i] = a.palette[i];
        if (tf) s_lut[i] = a.lut[i];
        if (mark && i < 8u) s_hidden[i] = a.hidden[i];
    }
    __syncthreads();

    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t i = tx * 16u + (((wave & 1u) << 3) | (lane & 7u));
    const uint32_t j = ty * 16u + (((wave >> 1) << 3) | (lane >> 3));
    if (i >= a.width || j >= a.height) return;

    // p = origin + i * du + j * dv in 32-bit unsigned arithmetic with wrap-around, read as int32.  The host admits a slice only if
    // its four corners lie in [-2^30, 2^30) on every axis (volym_slice_check); p is affine, so every pixel's position does, and
    // the wrapped sum is congruent to the integer value modulo 2^32 with that value inside int32: they are equal, even where a
    // product wraps.  floor(p / 65536) is the arithmetic shift.
    const int x = static_cast<int32_t>(a.origin[0] + i * a.du[0] + j * a.dv[0]) >> 16;
    const int y = static_cast<int32_t>(a.origin[1] + i * a.du[1] + j * a.dv[1]) >> 16;
    const int z = static_cast<int32_t>(a.origin[2] + i * a.du[2] + j * a.dv[2]) >> 16;
    const uint32_t ux = static_cast<uint32_t>(x), uy = static_cast<uint32_t>(y), uz = static_cast<uint32_t>(z);

    uint32_t out = a.background;
    if (ux < a.nx && uy < a.ny && uz < a.nz) {         // inside: 0 <= t < n on every axis (a negative t is a large unsigned one)
        uint32_t label = 0u;
        if (a.labels != nullptr && (overlay || mark)) {
            const bool lb = a.labels_bricked != 0u;
            label = a.labels[layout_offset(lb, layout_bx(lb, a.nx), layout_bxy(lb, a.nx, a.ny), ux, uy, uz)];
        }
        uint32_t b;
        if (importance) {
            const bool ib = a.imp_bricked != 0u;
            b = a.imp[layout_offset(ib, layout_bx(ib, a.nx), layout_bxy(ib, a.nx, a.ny), ux, uy, uz)];
        } else {
            GridT<BRICK> g;
            grid_init(g, a.vol, nullptr, a.nx, a.ny, a.nz);
            b = a.vol[voxel_offset(g, x, y, z)];
        }
        out = tf ? (s_lut[(b * a.tf_n) >> 8] | 0xff000000u) : (b * 0x010101u) | 0xff000000u;
        if (overlay) out = slice_blend(out, s_pal[label]);
        if (mark) {
            bool removed = ux < a.crop_lo[0] || ux >= a.crop_hi[0] || uy < a.crop_lo[1] || uy >= a.crop_hi[1] || uz < a.crop_lo[2] || uz >= a.crop_hi[2];
            removed = removed || a.clip_n[0] * x + a.clip_n[1] * y + a.clip_n[2] * z > a.clip_d;      // |n . t| < 2^31 (volym_set_clip_plane)
            removed = removed || ((s_hidden[label >> 5] >> (label & 31u)) & 1u) != 0u;                 // label 0 and hidden all 0 without labels
            if (removed) out = slice_blend(out, a.cut);
        }
    }
    a.out[static_cast<size_t>(j) * a.width + i] = out;
}

}  // namespace volym
