// Kernel of the projection pass (gfx950): maximum and mean intensity along the view rays.  The host twin is scene.project_frame
// (volym_amd/scene.py) and agrees on every byte.  (project.hip, the only unit that includes this header.)
//
// The launch shape is the pick kernel's: one 256-thread workgroup per 16x16 pixel block of the rect, one wave64 per 8x8 block, one
// lane per ray; the ray set-up (make_ray), the texel arithmetic (texel_nearest, voxel_offset) and the one label fetch of a ray are
// the march's.  The loop is not: sample k lies at t_entry + (float)k * step, a function of k alone, so there is no step state, no
// alpha chain and nothing to replay when samples are left out.  Per sample: one multiply and one add for t, three multiply-adds
// for the position (unfused, as the march computes it), the address, one byte load, an integer add and a compare.
//
// Skipping (default; VOLYM_PROJECT_NO_SKIP reads every sample).  After a run of PROJECT_ZERO_RUN zero bytes a lane looks the macro
// cell of its next sample up in d_mc before it reads the sample.  When the cell's maximum is 0 and the position lies inside the
// cell shrunk by eps on every face, that sample and every later one in front of the ray's exit from the shrunken cell read 0: they
// add nothing to the sum and cannot exceed the running maximum, and none of them is fetched.  The exit is rounded down (the pick
// kernel's slack), the index of the last such sample is estimated and accepted only by the rule's own comparison (t_kk < t_stop;
// else the index below it, else none), and the next sample is at least k + 1 in every case, so each iteration advances.  A leap
// keeps the run, so a row of empty cells is crossed at one look each.  A look that does not leap -- an occupied cell, a position
// within eps of a face (a ray that runs in the plane between two cells never leaves it), outside the grid -- ends the run: zeros
// scattered through occupied cells (noise) and rays along cell faces pay one look per PROJECT_ZERO_RUN + 1 samples at most.
// When to look is a matter of cost alone: whatever is left out was proven to read 0.  Only samples in cells of maximum 0 are left
// out: a record holds max and mean of the same ray, and a cell that cannot raise the maximum still feeds the sum.  A ray through
// dense texels never looks.
// (Measured on the device, profiles/projection.txt and DESIGN.md 4.10: on the scenes timed so far the default path does not beat
// NO_SKIP, also not under a crop box, where the leaps happen; the cause is not established.  An earlier form that looked after
// every zero byte was slower still -- a wave takes the branch when any of its 64 lanes does, and the synthetic bonsai's air is
// noise of 0..5 -- which is why a run of zeros is asked for; that comparison was not recorded.)
//
// n_samples is the rule's count on both paths: the loop of a lane ends at the first k with !(t_k < t_exit), leaps stop in front of
// min(cell exit, t_exit), so that k is the count.
//
//   BRICK    layout of the density (GridT<BRICK>); the labels take their own layout at run time.  mode and flags are uniform.
#pragma once

#include "raymarch_device.h"

namespace volym {

constexpr uint32_t PROJECT_ZERO_RUN = 4u;      // consecutive zero bytes before a lane looks its macro cell up

enum : uint32_t { PROJECT_TF = 1u, PROJECT_LABELS = 2u, PROJECT_NO_SKIP = 4u };      // VOLYM_PROJECT_TF, _LABELS, _NO_SKIP

struct ProjectArgs {
    const uint8_t* vol;
    const uint8_t* labels;         // NULL: no labels with the volume's dimensions on the device
    const uint8_t* mc;             // mc_n^3 macro-cell maxima of vol (volym_ctx::d_mc)
    uint4* out;                    // w * h records, row-major within the rect
    uint32_t* image;               // w * h rgba8, row-major within the rect; NULL: no image
    uint32_t x0, y0, w, h;         // the rect, pixels of the frame
    uint32_t tiles_x;              // 16x16 blocks per row of the rect
    uint32_t mc_n;
    uint32_t labels_bricked;
    uint32_t mode, flags;
    uint32_t tf_n;
    uint32_t background;           // rgba8 as the image holds it: r in the low byte
    float step;
    uint32_t palette[256];         // LABELS
    uint32_t lut[256];             // TF: the table volym_set_transfer_function received
};

// the outline's blend (include/volym_hip.h at volym_outline): out[c] = (src[c] * (255 - A) + col[c] * A + 127) / 255 for r, g, b, and
// 255 for col in the alpha byte
__device__ __forceinline__ uint32_t project_blend(uint32_t src, uint32_t col)
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
__global__ __launch_bounds__(256) void volym_project_kernel(const ProjectArgs a, const FrameParams fp)
{
    __shared__ uint32_t s_pal[256];
    __shared__ uint32_t s_lut[256];

    const bool image = a.image != nullptr;
    const bool tf = image && (a.flags & PROJECT_TF) != 0u, overlay = image && (a.flags & PROJECT_LABELS) != 0u;
    const bool skip = (a.flags & PROJECT_NO_SKIP) == 0u;
    if (tf) s_lut[threadIdx.x] = a.lut[threadIdx.x];
    if (overlay) s_pal[threadIdx.x] = a.palette[threadIdx.x];
    __syncthreads();

    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t rx = tx * 16u + (((wave & 1u) << 3) | (lane & 7u));
    const uint32_t ry = ty * 16u + (((wave >> 1) << 3) | (lane >> 3));
    const bool in_rect = rx < a.w && ry < a.h;         // the host keeps the rect inside the frame

    GridT<BRICK> g;
    grid_init(g, a.vol, nullptr, fp.nx, fp.ny, fp.nz);

    Ray ray;
    ray.o = ray.d = v3(0.0f, 0.0f, 0.0f);
    ray.t_entry = ray.t_exit = 0.0f;
    ray.hit = false;
    if (in_rect) ray = make_ray(fp, a.x0 + rx, a.y0 + ry);
    bool live = in_rect && ray.hit;

    const float step = a.step, inv_step = 1.0f / step;
    const float mcf = static_cast<float>(a.mc_n), inv_mc = 1.0f / mcf;
    const float idx_ = 1.0f / ray.d.x, idy_ = 1.0f / ray.d.y, idz_ = 1.0f / ray.d.z;
    const float nox = -ray.o.x * idx_, noy = -ray.o.y * idy_, noz = -ray.o.z * idz_;

    uint32_t k = 0u, best = 0u, best_k = 0u, sum = 0u, zeros = 0u;

    // a lane is done at the first k whose sample does not exist; the wave ends when no lane is live
    while (__ballot(live) != 0ull) {
        if (!live) continue;
        const float t = ray.t_entry + static_cast<float>(k) * step;          // the rule: a multiply, an add (-ffp-contract=off)
        if (!(t < ray.t_exit) || k >= 65535u) { live = false; continue; }     // (the bound is never reached: include/volym_hip.h)
        const V3 pos = ray.o + ray.d * t;
        if (skip && zeros >= PROJECT_ZERO_RUN) {
            // ---- is sample k inside an empty macro cell?  Conservative arithmetic only: it never decides what a sample reads ----
            const float cxf = __builtin_floorf(pos.x * mcf), cyf = __builtin_floorf(pos.y * mcf), czf = __builtin_floorf(pos.z * mcf);
            const int cx = static_cast<int>(cxf), cy = static_cast<int>(cyf), cz = static_cast<int>(czf);
            zeros = 0u;                                   // a look that ends without a leap: sample on, and look again after the next run
            if (static_cast<uint32_t>(cx | cy | cz) < a.mc_n) {
                if (a.mc[static_cast<uint32_t>(cx) + a.mc_n * (static_cast<uint32_t>(cy) + a.mc_n * static_cast<uint32_t>(cz))] == 0u) {
                    // the cell [c, c + 1] / mc_n shrunk by eps on every face
                    const float eps = 4.0e-5f;
                    const float lx = __builtin_fmaf(cxf, inv_mc, eps), hx = __builtin_fmaf(cxf, inv_mc, inv_mc - eps);
                    const float ly = __builtin_fmaf(cyf, inv_mc, eps), hy = __builtin_fmaf(cyf, inv_mc, inv_mc - eps);
                    const float lz = __builtin_fmaf(czf, inv_mc, eps), hz = __builtin_fmaf(czf, inv_mc, inv_mc - eps);
                    if (pos.x > lx && pos.x < hx && pos.y > ly && pos.y < hy && pos.z > lz && pos.z < hz) {
                        // sample k reads 0, and so does every later one in front of the ray's exit from the shrunken cell
                        const float ex = __builtin_fmaxf(__builtin_fmaf(lx, idx_, nox), __builtin_fmaf(hx, idx_, nox));
                        const float ey = __builtin_fmaxf(__builtin_fmaf(ly, idy_, noy), __builtin_fmaf(hy, idy_, noy));
                        const float ez = __builtin_fmaxf(__builtin_fmaf(lz, idz_, noz), __builtin_fmaf(hz, idz_, noz));
                        float te = __builtin_fminf(__builtin_fminf(ex, ey), ez);      // NaN (0 * inf) drops out
                        te = te - 2.0e-5f * __builtin_fabsf(te);                      // rounding slack
                        const float t_stop = __builtin_fminf(te, ray.t_exit);
                        // the last sample in front of t_stop: an estimate, accepted only by the rule's own comparison, else the one below it
                        const float est = __builtin_floorf((t_stop - ray.t_entry) * inv_step);
                        uint32_t next = k + 1u;                                       // sample k itself is left out in every case
                        if (est > static_cast<float>(k)) {                            // (false for a NaN)
                            const uint32_t kk = static_cast<uint32_t>(est);           // k < kk < 2^24: exact
                            if (ray.t_entry + est * step < t_stop) next = kk + 1u;    // samples k .. kk read 0
                            else if (ray.t_entry + (est - 1.0f) * step < t_stop) next = kk;
                        }
                        k = next;
                        zeros = PROJECT_ZERO_RUN;                                     // a leap keeps the run: the next cell is looked up at once
                        continue;
                    }
                }
            }
        }
        const uint32_t b = a.vol[voxel_offset(g, texel_nearest(pos.x, g.fnx, g.hix), texel_nearest(pos.y, g.fny, g.hiy), texel_nearest(pos.z, g.fnz, g.hiz))];
        sum += b;
        if (b > best) { best = b; best_k = k; }
        ++k;
        zeros = b != 0u ? 0u : zeros + 1u;
    }

    if (!in_rect) return;
    k = k < 65535u ? k : 65535u;                                                // (n_samples is 16 bits; never reached)
    const size_t at = static_cast<size_t>(ry) * a.w + rx;
    uint32_t status = 0u, mean = 0u, label = 0u, ux = 0u, uy = 0u, uz = 0u;
    float t_best = -1.0f;
    if (ray.hit) {
        status = best != 0u ? 2u : 1u;
        mean = (2u * sum + k) / (2u * k);                                      // k >= 1: sample 0 of a hit ray exists
        if (best != 0u) {
            t_best = ray.t_entry + static_cast<float>(best_k) * step;
            const V3 pos = ray.o + ray.d * t_best;
            ux = static_cast<uint32_t>(texel_nearest(pos.x, g.fnx, g.hix));
            uy = static_cast<uint32_t>(texel_nearest(pos.y, g.fny, g.hiy));
            uz = static_cast<uint32_t>(texel_nearest(pos.z, g.fnz, g.hiz));
            if (a.labels != nullptr) {
                const bool lb = a.labels_bricked != 0u;
                label = a.labels[layout_offset(lb, layout_bx(lb, fp.nx), layout_bxy(lb, fp.nx, fp.ny), ux, uy, uz)];
            }
        }
    }
    // struct volym_projection as the four dwords of its one store; a tile row is 128 contiguous bytes
    a.out[at] = make_uint4(__float_as_uint(t_best), ux | (uy << 16), uz | (best << 16) | (mean << 24), label | (status << 8) | (k << 16));
    if (image) {
        uint32_t px = a.background;
        if (ray.hit) {
            const uint32_t v = a.mode == 1u ? mean : best;
            px = tf ? (s_lut[(v * a.tf_n) >> 8] | 0xff000000u) : (v * 0x010101u) | 0xff000000u;
            if (overlay && status == 2u) px = project_blend(px, s_pal[label]);
        }
        a.image[at] = px;
    }
}

}  // namespace volym
