// The pick march (gfx950): which sample of a pixel's ray does the picture show?  (pick.hip, the only unit that includes this header.)
//
// The launch shape and the march are those of volym_raymarch_kernel<1, ...> (raymarch_kernels.h): one 256-thread workgroup per 16x16
// pixel block, one wave64 per 8x8 block, one lane per ray; the same ray set-up, texel arithmetic, step state machine, threshold test,
// look-ahead suppression and, in table mode, the same distance-field leaps (conservative arithmetic, replayed step sizes: they never
// decide a sample).  What a frame needs beyond that does not exist here: no gradient taps, no shading, no colour.  alpha is a plain
// f32 register updated in the shader's order (wgsl:313-318: w = (1 - alpha) * a; alpha += w) -- EXACT arithmetic, because here alpha
// decides: the pick is the first composited sample after whose compositing alpha >= alpha_min, and the march of the lane ends there.
//
//   BRICK    layout of density and importances (GridT<BRICK>); the one label fetch of a ray takes the labels' own layout
//   GENERAL  false: table mode (nearest filter, no smoothing) without importance rendering or colouring -- the common frame;
//            true:  everything else (look-ahead, smoothing, trilinear, colouring), decided at run time from the flags
#pragma once

#include "raymarch_device.h"

namespace volym {

struct PickArgs {
    const uint8_t* vol;
    const uint8_t* imp;
    const uint8_t* labels;         // NULL: no labels with the volume's dimensions on the device
    const FrameTables* tables;
    const uint8_t* df4;            // packed distance field of the frame's threshold (mc_n <= 32), NULL: march directly
    uint4* out;                    // w * h records, row-major within the rect
    uint32_t x0, y0, w, h;         // the rect, pixels of the frame
    uint32_t tiles_x;              // 16x16 blocks per row of the rect
    uint32_t labels_bricked;
    float alpha_min;
};

// volym_pick (include/volym_hip.h) as the four dwords of its one store
__device__ __forceinline__ uint4 pick_record(float t, uint32_t x, uint32_t y, uint32_t z, uint32_t label, uint32_t density, uint32_t status,
                                             uint32_t alpha8, uint32_t has_labels)
{
    return make_uint4(__float_as_uint(t), x | (y << 16), z | (label << 16) | (density << 24), status | (alpha8 << 8) | (has_labels << 16));
}

template <bool BRICK, bool GENERAL>
__global__ __launch_bounds__(256) void volym_pick_kernel(const PickArgs a, const FrameParams fp)
{
    __shared__ float s_alpha[256];      // tf_tab[b].w: the opacity of a table-mode sample
    __shared__ float s_rho[256];
    __shared__ float4 s_lut[GENERAL ? 256 : 1];
    __shared__ float s_ic_alpha[GENERAL ? 256 : 1];
    __shared__ __attribute__((aligned(16))) uint8_t s_df[VOLYM_DF_LDS_BYTES];

    const uint32_t flags = fp.flags;
    const bool linear = GENERAL && (flags & F_LINEAR) != 0u;
    const bool gauss = GENERAL && (flags & F_GAUSSIAN) != 0u;
    const bool table_mode = !linear && !gauss;
    const bool use_df = table_mode && a.df4 != nullptr;
    const bool colouring = GENERAL && (flags & F_IMP_COLORING) != 0u;
    const bool imp_rendering = GENERAL && !colouring && (flags & F_IMP_RENDERING) != 0u;
    const bool use_alpha = colouring || (flags & F_OPACITY) != 0u;

    {
        const uint32_t i = threadIdx.x;
        s_alpha[i] = a.tables->tf_tab[i].w;
        s_rho[i] = a.tables->rho[i];
        if (GENERAL) {
            if (!table_mode) s_lut[i] = a.tables->lut_f[i];
            if (colouring) s_ic_alpha[i] = a.tables->ic_alpha[i];
        }
        if (use_df) {
            const uint32_t n16 = (fp.mc_n * fp.mc_n * fp.mc_n / 2u + 15u) / 16u;     // <= VOLYM_DF_LDS_BYTES / 16: the host passes df4 for mc_n <= 32 only
            const uint4* src = reinterpret_cast<const uint4*>(a.df4);
            uint4* dst = reinterpret_cast<uint4*>(s_df);
            for (uint32_t k = i; k < n16; k += 256u) dst[k] = src[k];
        }
    }
    __syncthreads();

    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t rx = tx * 16u + (((wave & 1u) << 3) | (lane & 7u));
    const uint32_t ry = ty * 16u + (((wave >> 1) << 3) | (lane >> 3));
    const bool in_rect = rx < a.w && ry < a.h;         // the host keeps the rect inside the frame
    const uint32_t has_labels = a.labels != nullptr ? 1u : 0u;

    GridT<BRICK> g;
    grid_init(g, a.vol, a.imp, fp.nx, fp.ny, fp.nz);

    Ray ray;
    ray.hit = false;
    if (in_rect) ray = make_ray(fp, a.x0 + rx, a.y0 + ry);
    bool live = in_rect && ray.hit;

    const float base = fp.base_step, min_step = fp.min_step, thr = fp.thr;
    float t = ray.t_entry, cur = base;
    float acc_a = 0.0f;
    bool picked = false;
    int pix = 0, piy = 0, piz = 0;
    uint32_t dummy = 0;

    // distance-field leaps: conservative arithmetic only (never decides a sample), as volym_raymarch_kernel<1>
    const float mcf = static_cast<float>(fp.mc_n), inv_mc = 1.0f / mcf;
    const float idx_ = 1.0f / ray.d.x, idy_ = 1.0f / ray.d.y, idz_ = 1.0f / ray.d.z;
    const float nox = -ray.o.x * idx_, noy = -ray.o.y * idy_, noz = -ray.o.z * idz_;

    // a lane is done at its pick, at loop exit or on a miss; the wave ends when no lane is live
    while (__ballot(live) != 0ull) {
        if (!live) continue;
        if (!(t < ray.t_exit && acc_a < 0.95f)) { live = false; continue; }     // wgsl:250
        const V3 pos = ray.o + ray.d * t;                                     // wgsl:251
        if (use_df) {
            const float cxf = __builtin_floorf(pos.x * mcf), cyf = __builtin_floorf(pos.y * mcf), czf = __builtin_floorf(pos.z * mcf);
            const int cx = static_cast<int>(cxf), cy = static_cast<int>(cyf), cz = static_cast<int>(czf);
            uint32_t D = 0;
            if (static_cast<uint32_t>(cx | cy | cz) < fp.mc_n) {
                const uint32_t ci = static_cast<uint32_t>(cx) + fp.mc_n * (static_cast<uint32_t>(cy) + fp.mc_n * static_cast<uint32_t>(cz));
                D = (static_cast<uint32_t>(s_df[ci >> 1]) >> ((ci & 1u) * 4u)) & 15u;
            }
            if (D != 0u) {
                // box of empty cells [c-R, c+R+1]/mc_n shrunk by eps on every face, R = D-1
                const float eps = 4.0e-5f;
                const float r = static_cast<float>(D - 1u) * inv_mc - eps;
                const float lx = __builtin_fmaf(cxf, inv_mc, -r), hx = __builtin_fmaf(cxf, inv_mc, r + inv_mc);
                const float ly = __builtin_fmaf(cyf, inv_mc, -r), hy = __builtin_fmaf(cyf, inv_mc, r + inv_mc);
                const float lz = __builtin_fmaf(czf, inv_mc, -r), hz = __builtin_fmaf(czf, inv_mc, r + inv_mc);
                const float ex = __builtin_fmaxf(__builtin_fmaf(lx, idx_, nox), __builtin_fmaf(hx, idx_, nox));
                const float ey = __builtin_fmaxf(__builtin_fmaf(ly, idy_, noy), __builtin_fmaf(hy, idy_, noy));
                const float ez = __builtin_fmaxf(__builtin_fmaf(lz, idz_, noz), __builtin_fmaf(hz, idz_, noz));
                float te = __builtin_fminf(__builtin_fminf(ex, ey), ez);   // NaN (0*inf) drops out
                te = te - 2.0e-5f * __builtin_fabsf(te);                    // rounding slack
                const bool inside = pos.x > lx && pos.x < hx && pos.y > ly && pos.y < hy && pos.z > lz && pos.z < hz;
                const float t_stop = __builtin_fminf(te, ray.t_exit);
                if (inside && t < t_stop) {
                    do {                                                    // wgsl:263-274 of a sample below the threshold
                        cur = __builtin_fminf(base, cur * 1.5f);
                        t += cur;
                    } while (t < t_stop);
                    continue;
                }
            }
        }

        // ---- density (wgsl:253-259) and the step state machine (wgsl:263-274) ----
        const int ix = texel_nearest(pos.x, g.fnx, g.hix), iy = texel_nearest(pos.y, g.fny, g.hiy), iz = texel_nearest(pos.z, g.fnz, g.hiz);
        const uint32_t off = voxel_offset(g, ix, iy, iz);
        uint32_t b = 0;
        float rho = 0.0f;
        bool dense;
        if (table_mode) {
            b = a.vol[off];
            dense = b >= fp.thr_byte;                                       // <=> b/255 >= thr
        } else {
            if (gauss) rho = sample_density_smoothed<false>(g, s_rho, linear, fp, pos, ray.d, dummy);
            else rho = sample_density(g, s_rho, linear, pos);
            dense = rho >= thr;
        }
        cur = dense ? min_step : __builtin_fminf(base, cur * 1.5f);
        if (!dense) { t += cur; continue; }

        // ---- classification (wgsl:276-304): what the sample's opacity is, or that it is suppressed ----
        float alpha_step;
        if (colouring) {                                                    // wgsl:83-92
            alpha_step = s_ic_alpha[g.imp[off]];
        } else {
            if (imp_rendering) {                                            // wgsl:283-295
                const uint32_t ib = g.imp[off];
                const bool ahead = (flags & F_CONE) ? ahead_cone<false>(g, fp, pos, ray.d, ray.t_exit, dummy)
                                                    : ahead_straight<false>(g, fp, pos, ray.d, ray.t_exit, dummy);
                if (ib < 255u && ahead) { t += cur; continue; }             // importance < 1.0 && ahead
            }
            if (table_mode) alpha_step = s_alpha[b];
            else alpha_step = 1.0f - wgsl_pow(1.0f - sample_tf(s_lut, fp.tf_n, rho).w, fp.alpha_y);   // wgsl:297-303, :314
        }

        // ---- compositing (wgsl:313-325), alpha alone ----
        if (use_alpha) {
            const float w = (1.0f - acc_a) * alpha_step;
            acc_a += w;
        } else {
            acc_a = 1.0f;                                                   // first hit (wgsl:319-323)
        }
        if (acc_a >= a.alpha_min || !use_alpha) {
            picked = true; live = false;
            pix = ix; piy = iy; piz = iz;
            continue;                                                       // t stays the picked sample's
        }
        t += cur;                                                           // wgsl:325
    }

    if (!in_rect) return;
    uint4 rec;
    if (picked) {
        const uint32_t x = static_cast<uint32_t>(pix), y = static_cast<uint32_t>(piy), z = static_cast<uint32_t>(piz);
        const uint32_t density = a.vol[voxel_offset(g, pix, piy, piz)];
        uint32_t label = 0;
        if (has_labels) {
            const bool lb = a.labels_bricked != 0u;
            label = a.labels[layout_offset(lb, layout_bx(lb, fp.nx), layout_bxy(lb, fp.nx, fp.ny), x, y, z)];
        }
        rec = pick_record(t, x, y, z, label, density, 2u, to_unorm8(acc_a), has_labels);
    } else {
        rec = pick_record(-1.0f, 0u, 0u, 0u, 0u, 0u, ray.hit ? 1u : 0u, ray.hit ? to_unorm8(acc_a) : 255u, has_labels);
    }
    a.out[static_cast<size_t>(ry) * a.w + rx] = rec;                        // one 16-byte store; a tile row is 128 contiguous bytes
}

}  // namespace volym
