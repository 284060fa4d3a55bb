// Kernels of the outline pass (gfx950): which pixels of the frame show a selected segment, as a bit plane, then the ring round them
// and the blend.  Integer only; the host twin is scene.outline_frame (volym_amd/scene.py) and agrees on every byte.
//
// The bit plane: one bit per frame pixel at its frame-absolute position, bit i of word k of row y is pixel (64k + i, y).  A row is
// `stride` = ceil(W / 64) + 2 words, the first and the last a guard; there are 8 guard rows above row 0 and 8 below row H - 1.
// The guards are zeroed when the plane is allocated and never written, so that the dilation reads through the frame's edges
// without a bounds branch (the radius is at most 8).  Pack rewrites every word that is not a guard, each pass.
//
// Two launches: the words the second reads were written by an earlier launch, never by its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace volym {

constexpr uint32_t OUTLINE_GUARD_ROWS = 8;      // the largest radius
constexpr uint32_t OUTLINE_PACK_ROWS = 4;       // rows of one wave of the pack kernel
constexpr uint32_t OUTLINE_STRIP_ROWS = 8;      // rows of one wave of the blend kernel

struct OutlineArgs {
    const uint2* tails;        // the records, viewed as 8-byte halves: half 2i + 1 holds bytes 8..15 of record i
    uint64_t* plane;
    const uint32_t* src;       // the frame
    uint32_t* dst;             // the target; may be src (a pixel reads only its own texel)
    uint64_t sel[4];           // selected[l] != 0 as bit l
    uint32_t W, H, stride;     // stride: words per plane row, guards included
    uint32_t x0, y0, w, h;     // the rect the records cover
    uint32_t ring, fill;       // rgba8 as the frame holds it: r in the low byte
};

__device__ __forceinline__ uint64_t* outline_plane_word(uint64_t* plane, uint32_t stride, uint32_t y, uint32_t k)
{
    return plane + static_cast<size_t>(y + OUTLINE_GUARD_ROWS) * stride + (k + 1u);
}

// One wave per 64 consecutive pixels of OUTLINE_PACK_ROWS rows: a lane loads bytes 8..15 of its pixel's record (z, label, density,
// status, ...), tests status == 2 && selected[label], and the ballot is the word.  Block (64, 4).
__global__ __launch_bounds__(256) void volym_outline_pack_kernel(OutlineArgs a)
{
    const uint32_t k = blockIdx.x;
    const uint32_t x = k * 64u + threadIdx.x;
    const uint32_t row0 = (blockIdx.y * 4u + threadIdx.y) * OUTLINE_PACK_ROWS;
    const bool in_x = x >= a.x0 && x - a.x0 < a.w;
    uint2 tail[OUTLINE_PACK_ROWS];
#pragma unroll
    for (uint32_t j = 0; j < OUTLINE_PACK_ROWS; ++j) {
        const uint32_t y = row0 + j;
        tail[j] = make_uint2(0u, 0u);                                       // status 0: not selected
        if (in_x && y >= a.y0 && y - a.y0 < a.h)
            tail[j] = a.tails[(static_cast<size_t>(y - a.y0) * a.w + (x - a.x0)) * 2u + 1u];
    }
#pragma unroll
    for (uint32_t j = 0; j < OUTLINE_PACK_ROWS; ++j) {
        const uint32_t y = row0 + j;
        const uint32_t label = (tail[j].x >> 16) & 0xffu, status = tail[j].y & 0xffu;
        const uint64_t w01 = (label & 64u) ? a.sel[1] : a.sel[0], w23 = (label & 64u) ? a.sel[3] : a.sel[2];
        const uint64_t word = (label & 128u) ? w23 : w01;
        const bool selected = status == 2u && ((word >> (label & 63u)) & 1u) != 0u;
        const uint64_t bits = __ballot(selected);
        if (threadIdx.x == 0u && y < a.H) *outline_plane_word(a.plane, a.stride, y, k) = bits;
    }
}

// rgba8 blend of the rule: out[c] = (src[c] * (255 - A) + col[c] * A + 127) / 255 for r, g, b, and 255 for col in the alpha byte
__device__ __forceinline__ uint32_t outline_blend(uint32_t src, uint32_t col)
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

// x | x << 1 | ... | x << r (up) or the same with >> (down), by doubling: r is wave-uniform, 1..8
__device__ __forceinline__ uint64_t outline_smear(uint64_t x, uint32_t r, bool up)
{
    for (uint32_t done = 0; done < r;) {
        const uint32_t s = (done + 1u < r - done) ? done + 1u : r - done;
        x |= up ? x << s : x >> s;
        done += s;
    }
    return x;
}

// the 64-bit value lane `l` holds, in every lane (l: a constant)
__device__ __forceinline__ uint64_t outline_from_lane(uint64_t v, int l)
{
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), l), hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(v >> 32), l);
    return static_cast<uint64_t>(hi) << 32 | lo;
}

// One wave per strip of 64 x OUTLINE_STRIP_ROWS pixels, rows y0 .. y1 - 1.  The strip needs the plane rows y0 - r .. y1 - 1 + r, at
// most 24 of them: lane l takes row y0 - r + l and its three words (left neighbour, centre, right neighbour), so the dilation
// runs bit-parallel across the lanes.  Sideways first: with the top r bits of the left word moved below the centre's bit 0 and
// the low r bits of the right word above its bit 63 folded in, d = up(c | right << (64 - r)) | down(c | left >> (64 - r)), where up
// and down smear by 0..r places.  Then down the lanes: lane j ORs the lanes j .. j + 2r, again by doubling, and holds the dilated
// word of row y0 + j; the centre word of that row comes from lane j + r.  Each row's two words are then broadcast and every lane
// takes its bit of them.  The frame texels of the strip are loaded before anything is stored: the target may be the frame.
// Block (64, 4).
__global__ __launch_bounds__(256) void volym_outline_blend_kernel(OutlineArgs a, uint32_t r)
{
    constexpr int R = static_cast<int>(OUTLINE_STRIP_ROWS);
    const uint32_t k = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t x = k * 64u + lane;
    const int y0 = static_cast<int>((blockIdx.y * 4u + threadIdx.y) * OUTLINE_STRIP_ROWS);
    const int H = static_cast<int>(a.H);
    if (y0 >= H) return;                                                        // the whole wave: y0 is the same in all its lanes
    const int y1 = y0 + R < H ? y0 + R : H;
    const bool in_x = x < a.W;

    uint32_t texel[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        texel[j] = 0u;
        if (in_x && y0 + j < y1) texel[j] = a.src[static_cast<size_t>(y0 + j) * a.W + x];
    }

    // plane row of this lane: >= -8 and, where it is read, <= H - 1 + 8 -- a guard row at the least and at the most
    const int yy = y0 - static_cast<int>(r) + static_cast<int>(lane);
    uint64_t left = 0u, centre = 0u, right = 0u;
    if (yy < y1 + static_cast<int>(r)) {
        const uint64_t* row = a.plane + static_cast<size_t>(yy + static_cast<int>(OUTLINE_GUARD_ROWS)) * a.stride + k;
        left = row[0]; centre = row[1]; right = row[2];
    }
    uint64_t near = outline_smear(centre | (right << (64u - r)), r, true) | outline_smear(centre | (left >> (64u - r)), r, false);
    for (uint32_t done = 0; done < 2u * r;) {                                   // lane j: OR of the lanes j .. j + 2r
        const uint32_t s = (done + 1u < 2u * r - done) ? done + 1u : 2u * r - done;
        near |= __shfl_down(near, s);
        done += s;
    }
    const uint64_t own = __shfl_down(centre, r);                                // lane j: the centre word of row y0 + j

#pragma unroll
    for (int j = 0; j < R; ++j) {
        const uint64_t m = outline_from_lane(own, j), d = outline_from_lane(near, j);
        const int y = y0 + j;
        if (y < y1 && in_x) {
            uint32_t out = texel[j];
            if ((m >> lane) & 1u) out = outline_blend(out, a.fill);
            else if ((d >> lane) & 1u) out = outline_blend(out, a.ring);
            a.dst[static_cast<size_t>(y) * a.W + x] = out;
        }
    }
}

}  // namespace volym
