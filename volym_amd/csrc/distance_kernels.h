// The kernels of the distance pass (volym_distance_pass): the exact squared Euclidean distance, weighted per axis, from every texel
// of a request's box to the nearest SEED of the box -- a solid texel, or with INSIDE a texel that is not solid.  Included by
// distance.hip alone.
//
// The transform is separable: D(x, y, z) = min over z' of wz (z - z')^2 + [min over y' of wy (y - y')^2 + [min over x' of
// wx (x - x')^2 over the seeds of row (y', z')]].  Three sweeps over the map, box-linear (i = (x - x0) + w * ((y - y0) + h * (z - z0))):
//   rows     one wave per row of the box, 64-texel chunks through layout_offset (the walk and the predicate of box_walk.h); the nearest seed
//            on either side from one ballot per chunk and two carries; no atomic but the two counters.
//   columns  along y, then along z, in place: f(i) = min_j g(j) + w (i - j)^2 over the entries with g(j) != NONE, as the lower
//            envelope of the parabolas (Meijster's two scans).  One lane per column, adjacent lanes on adjacent x, so every load and
//            store of the map and of the stacks is coalesced.  The stacks lie entry-major beside the map: entry k of the column that
//            starts at `base` is word base + k * stride of each of the two work arrays, (site | first index it wins from << 16) and
//            the site's g.  The site's g is kept because the evaluation runs in place: a site can lie on either side of the stretch it
//            wins, so its own word of the map may be overwritten before the stretch is evaluated.
//   finish   one wave per row again: the INSIDE border, the final store, and the summary through LDS.
// Widths.  A box has at most 2^31 - 2 texels: every box-linear index fits 31 bits.  An axis has at most 4096 texels and a weight is at
// most 64, so after the rows g <= 64 * 4095^2 < 2^30.01, and every f the column sweeps compare or store is at most 3 * 64 * 4095^2 =
// 3219655200 < 2^32: all of it is exact in uint32_t.  Every load and store is of a texel of the request's box, which
// volym_distance_check puts inside the volume, or of a word of the map or the work arrays with an index below the box's texel count.
#pragma once

#include "box_walk.h"

namespace volym {

struct DistanceArgs : BoxWalkArgs {     // w * n_rows <= 2^31 - 2 (volym_distance_check)
    uint32_t weight[3];
    uint32_t inside;                    // the seeds are the texels that are not solid
};

constexpr uint32_t DISTANCE_NONE = VOLYM_DISTANCE_NONE;
// the working summary as 64-bit words: three counters, the key of the maximum (D << 32 | ~index; 0: none), the keys of the nearest
// present texel per label (D << 32 | index; all ones: none) and the histogram
enum { DK_N_SOLID = 0, DK_N_PRESENT = 1, DK_N_FINITE = 2, DK_MAX = 3, DK_NEAR = 4, DK_HIST = 4 + 256, DISTANCE_KEY_WORDS = 4 + 256 + 256 };
// struct volym_distance_summary as 32-bit words
enum { DS_MAX_D2 = 6, DS_MAX_AT = 7, DS_NEAR_D2 = 10, DS_NEAR_AT = 10 + 256, DS_HIST = 10 + 256 + 768, DISTANCE_SUMMARY_WORDS = 10 + 256 + 768 + 512 };

// The working summary at rest, and the public summary of a box without texels (what an empty box leaves: the pack kernel, which
// overwrites it, does not run then).  One workgroup.
__global__ __launch_bounds__(256) void volym_distance_init_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ summary)
{
    const uint32_t t = threadIdx.x;
    if (t < 4u) keys[t] = 0ull;
    keys[DK_NEAR + t] = ~0ull;
    keys[DK_HIST + t] = 0ull;
    for (uint32_t i = t; i < DISTANCE_SUMMARY_WORDS; i += 256u)
        summary[i] = (i == DS_MAX_D2 || (i >= DS_NEAR_D2 && i < DS_NEAR_AT)) ? DISTANCE_NONE : 0u;
}

// ---- 1. rows: along x, wx * (distance to the nearest seed of the row)^2, or NONE for a row without seeds ---------------------------
// Left to right the map gets dl, the distance to the nearest seed at or left of the texel (NONE: none); dl == 0 marks the seeds, so
// the sweep back from the right needs no second look at the scene's bytes.
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_distance_rows_kernel(DistanceArgs a, BoxSelect select, uint32_t* __restrict__ map,
                                                                  unsigned long long* __restrict__ keys)
{
    __shared__ uint8_t s_select[256];
    s_select[threadIdx.x] = select.v[threadIdx.x];
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);        // bits 0..lane
    const uint64_t from = ~0ull << lane;                                        // bits lane..63
    const bool inside = a.inside != 0u;
    unsigned long long wave_solid = 0ull, wave_present = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t y = a.lo[1] + row % a.h, z = a.lo[2] + row / a.h;
        const uint32_t base = row * a.w;
        uint32_t carry = DISTANCE_NONE;                             // x of the last seed of the chunks before (wave-uniform)
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < a.w;
            bool present = false, solid = false;
            if (in) {
                uint32_t label;
                present = box_present<LABELS>(a, layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z), label);
                solid = present && box_selected(s_select, label);
            }
            const uint64_t sol = __ballot(solid);
            const uint64_t s = inside ? __ballot(in && !solid) : sol;
            const uint64_t left = s & upto;
            const uint32_t at = left ? x0 + (63u - static_cast<uint32_t>(__clzll(left))) : carry;
            if (in) map[base + xi] = at == DISTANCE_NONE ? DISTANCE_NONE : xi - at;
            if (s) carry = x0 + (63u - static_cast<uint32_t>(__clzll(s)));
            wave_solid += static_cast<uint32_t>(__popcll(sol));
            wave_present += static_cast<uint32_t>(__popcll(__ballot(present)));
        }
        // back from the right (each lane reads the words it stored itself); chunk k starts at 64 * k
        carry = DISTANCE_NONE;
        for (uint32_t k = (a.w + 63u) / 64u; k-- > 0u;) {
            const uint32_t x0 = k * 64u, xi = x0 + lane;
            const bool in = xi < a.w;
            const uint32_t dl = in ? map[base + xi] : DISTANCE_NONE;
            const uint64_t s = __ballot(in && dl == 0u);
            const uint64_t right = s & from;
            const uint32_t at = right ? x0 + static_cast<uint32_t>(__builtin_ctzll(right)) : carry;
            const uint32_t dr = at == DISTANCE_NONE ? DISTANCE_NONE : at - xi;
            const uint32_t m = min(dl, dr);                         // at most 4095, or NONE
            if (in) map[base + xi] = m == DISTANCE_NONE ? DISTANCE_NONE : a.weight[0] * m * m;
            if (s) carry = x0 + static_cast<uint32_t>(__builtin_ctzll(s));
        }
    }
    if (lane == 0u && wave_solid) atomicAdd(&keys[DK_N_SOLID], wave_solid);
    if (lane == 0u && wave_present) atomicAdd(&keys[DK_N_PRESENT], wave_present);
}

// ---- 2. columns: in place, f(i) = min_j g(j) + w * (i - j)^2 over the finite g(j) ----------------------------------------------------
// floor(num / den) for 0 <= num < 2^34, 0 < den < 2^20.  The f64 quotient only proposes: the two loops settle it in integers, so the
// result is exact whatever the rounding of the division (with a correctly rounded one neither loop turns: a quotient that is no
// integer lies at least 2^-20 from one, and the spacing of f64 at 2^14 is 2^-38).  An emulated 64-bit integer division would be many
// times the instructions.
__device__ __forceinline__ uint32_t distance_floor_div(uint64_t num, uint32_t den)
{
    uint32_t q = static_cast<uint32_t>(static_cast<double>(num) / static_cast<double>(den));
    while (static_cast<uint64_t>(q) * den > num) --q;
    while (static_cast<uint64_t>(q + 1u) * den <= num) ++q;
    return q;
}

struct DistanceColumns {
    uint32_t n;                         // entries of a column (the box's extent along the axis), 2..4096
    uint32_t stride;                    // words between two entries of a column
    uint32_t n_cols;                    // columns: the texels of the box / n
    uint32_t inner, outer;              // column c starts at word c % inner + (c / inner) * outer
    uint32_t weight;
};

__global__ __launch_bounds__(64) void volym_distance_columns_kernel(DistanceColumns a, uint32_t* __restrict__ map, uint32_t* __restrict__ stack,
                                                                    uint32_t* __restrict__ stack_g)
{
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.n_cols) return;
    const uint32_t base = c % a.inner + (c / a.inner) * a.outer;
    const uint32_t w = a.weight;
    // the stack's top in registers: site, the first index it wins from, the site's g
    int q = -1;
    uint32_t top_s = 0u, top_t = 0u, top_g = 0u;
    for (uint32_t u = 0u; u < a.n; ++u) {
        const uint32_t g = map[base + u * a.stride];
        if (g == DISTANCE_NONE) continue;                           // no parabola
        // pop while the new parabola is lower where the top's stretch starts (two f values: no division)
        while (q >= 0) {
            const uint32_t ds = top_t > top_s ? top_t - top_s : top_s - top_t, du = u - top_t;
            if (w * ds * ds + top_g <= w * du * du + g) break;
            if (--q >= 0) {
                const uint32_t e = stack[base + static_cast<uint32_t>(q) * a.stride];
                top_s = e & 0xffffu; top_t = e >> 16;
                top_g = stack_g[base + static_cast<uint32_t>(q) * a.stride];
            }
        }
        uint32_t first = 0u;
        if (q >= 0) {
            // the first index the new parabola wins from: 1 + floor of where it meets the top's.  The pop test left the top at or below
            // it at top_t >= 0, so they meet at or right of 0 and the numerator is no less than 0; it is below 64 * 4096^2 + 2^31 < 2^34.
            const uint64_t num = static_cast<uint64_t>(w) * (u * u - top_s * top_s) + g - top_g;      // (unsigned wrap-around of + g - top_g cancels: the sum is >= 0)
            first = distance_floor_div(num, 2u * w * (u - top_s)) + 1u;
            if (first >= a.n) continue;                             // it wins nowhere in the column
        }
        ++q;
        top_s = u; top_t = first; top_g = g;
        stack[base + static_cast<uint32_t>(q) * a.stride] = u | (first << 16);    // (both below 4096)
        stack_g[base + static_cast<uint32_t>(q) * a.stride] = g;
    }
    if (q < 0) return;                                              // an all-NONE column stays NONE
    for (uint32_t u = a.n; u-- > 0u;) {
        const uint32_t d = u > top_s ? u - top_s : top_s - u;
        map[base + u * a.stride] = w * d * d + top_g;
        if (u == top_t && q > 0) {
            --q;
            const uint32_t e = stack[base + static_cast<uint32_t>(q) * a.stride];
            top_s = e & 0xffffu; top_t = e >> 16;
            top_g = stack_g[base + static_cast<uint32_t>(q) * a.stride];
        }
    }
}

// ---- 3. finish: the INSIDE border, the final D, and the summary ------------------------------------------------------------------------
// the smallest c with c * c >= v, for v <= 254^2 (larger values go to bin 255 unrooted): the f32 root proposes, integers settle
__device__ __forceinline__ uint32_t distance_ceil_sqrt(uint32_t v)
{
    uint32_t c = static_cast<uint32_t>(sqrtf(static_cast<float>(v)));
    while (c * c < v) ++c;
    while (c > 0u && (c - 1u) * (c - 1u) >= v) --c;
    return c;
}

__device__ __forceinline__ unsigned long long distance_shfl_xor(unsigned long long v, int off)
{
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), off), hi = __shfl_xor(static_cast<uint32_t>(v >> 32), off);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

template <bool LABELS>
__global__ __launch_bounds__(256) void volym_distance_finish_kernel(DistanceArgs a, uint32_t* __restrict__ map, unsigned long long* __restrict__ keys)
{
    __shared__ unsigned long long s_near[256], s_hist[256], s_max, s_finite;
    s_near[threadIdx.x] = ~0ull;
    s_hist[threadIdx.x] = 0ull;
    if (threadIdx.x == 0u) { s_max = 0ull; s_finite = 0ull; }
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const bool inside = a.inside != 0u;
    unsigned long long wave_finite = 0ull, lane_max = 0ull;
    // a lane carries the nearest present texel of one run of equal labels and flushes it when the label changes, and at the end
    uint32_t cur = 256u;
    unsigned long long cur_key = ~0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        const uint32_t y = a.lo[1] + ry, z = a.lo[2] + rz;
        const uint32_t base = row * a.w;
        uint32_t border = DISTANCE_NONE;                            // INSIDE: the nearest texel outside the box along y and z (wave-uniform)
        if (inside) {
            const uint32_t by = min(ry + 1u, a.hi[1] - y), bz = min(rz + 1u, a.hi[2] - z);
            border = min(a.weight[1] * by * by, a.weight[2] * bz * bz);
        }
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane, i = base + xi;
            const bool in = xi < a.w;
            uint32_t d = DISTANCE_NONE, bin = 0u;
            if (in) {
                d = map[i];
                if (inside) {
                    const uint32_t b = min(xi + 1u, a.w - xi);
                    d = min(d, min(border, a.weight[0] * b * b));
                    map[i] = d;
                }
            }
            const bool finite = d != DISTANCE_NONE;
            if (finite) {
                const unsigned long long hi = static_cast<unsigned long long>(d) << 32;
                lane_max = max(lane_max, hi | static_cast<uint32_t>(~i));
                uint32_t label;
                if (box_present<LABELS>(a, layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z), label)) {
                    if (label != cur) {
                        if (cur < 256u) atomicMin(&s_near[cur], cur_key);
                        cur = label; cur_key = ~0ull;
                    }
                    cur_key = min(cur_key, hi | i);
                }
                bin = d > 254u * 254u ? 255u : distance_ceil_sqrt(d);
            }
            // the histogram: where the chunk's finite texels share one bin -- the inside of a segment, the far field -- one lane adds them
            const uint64_t f = __ballot(finite);
            if (f) {
                const uint32_t lead = __shfl(bin, static_cast<int>(__ffsll(static_cast<unsigned long long>(f))) - 1);
                if (__ballot(finite && bin != lead) == 0ull) {
                    if (lane == 0u) atomicAdd(&s_hist[lead], static_cast<unsigned long long>(__popcll(f)));
                } else if (finite) {
                    atomicAdd(&s_hist[bin], 1ull);
                }
                wave_finite += static_cast<uint32_t>(__popcll(f));
            }
        }
    }
    // The last flush of the runs.  Where the lanes that carry one all carry the same label -- one segment, or no labels -- the wave
    // takes the minimum with shuffles and one lane touches LDS (the components pass measured what per-lane flushes onto one word cost).
    const uint64_t have = __ballot(cur < 256u);
    if (have) {
        const uint32_t lead = __shfl(cur, static_cast<int>(__ffsll(static_cast<unsigned long long>(have))) - 1);
        if (__ballot(cur < 256u && cur != lead) != 0ull) {
            if (cur < 256u) atomicMin(&s_near[cur], cur_key);
        } else {
            for (int off = 32; off > 0; off >>= 1) cur_key = min(cur_key, distance_shfl_xor(cur_key, off));      // (no run: all ones, the neutral element)
            if (lane == 0u) atomicMin(&s_near[lead], cur_key);
        }
    }
    for (int off = 32; off > 0; off >>= 1) lane_max = max(lane_max, distance_shfl_xor(lane_max, off));
    if (lane == 0u && lane_max) atomicMax(&s_max, lane_max);
    if (lane == 0u && wave_finite) atomicAdd(&s_finite, wave_finite);
    __syncthreads();
    // only the entries this workgroup touched go to memory
    const unsigned long long near = s_near[threadIdx.x], count = s_hist[threadIdx.x];
    if (near != ~0ull) atomicMin(&keys[DK_NEAR + threadIdx.x], near);
    if (count) atomicAdd(&keys[DK_HIST + threadIdx.x], count);
    if (threadIdx.x == 0u && s_max) atomicMax(&keys[DK_MAX], s_max);
    if (threadIdx.x == 0u && s_finite) atomicAdd(&keys[DK_N_FINITE], s_finite);
}

// the working summary into struct volym_distance_summary, whole 32-bit words; one workgroup
__global__ __launch_bounds__(256) void volym_distance_pack_kernel(DistanceArgs a, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ summary)
{
    const uint32_t t = threadIdx.x;
    auto at = [&](uint32_t i, uint32_t* out) {                      // box-linear index -> volume coordinates
        out[0] = a.lo[0] + i % a.w;
        out[1] = a.lo[1] + (i / a.w) % a.h;
        out[2] = a.lo[2] + i / (a.w * a.h);
    };
    if (t < 3u) {
        summary[2u * t] = static_cast<uint32_t>(keys[t]);
        summary[2u * t + 1u] = static_cast<uint32_t>(keys[t] >> 32);
    }
    if (t == 0u) {
        const unsigned long long k = keys[DK_MAX];
        summary[DS_MAX_D2] = k ? static_cast<uint32_t>(k >> 32) : DISTANCE_NONE;
        uint32_t p[3] = {0u, 0u, 0u};
        if (k) at(~static_cast<uint32_t>(k), p);
        for (int j = 0; j < 3; ++j) summary[DS_MAX_AT + j] = p[j];
    }
    const unsigned long long k = keys[DK_NEAR + t];
    uint32_t p[3] = {0u, 0u, 0u};
    if (k != ~0ull) at(static_cast<uint32_t>(k), p);
    summary[DS_NEAR_D2 + t] = static_cast<uint32_t>(k >> 32);       // (all ones: NONE)
    for (int j = 0; j < 3; ++j) summary[DS_NEAR_AT + 3u * t + j] = p[j];
    summary[DS_HIST + 2u * t] = static_cast<uint32_t>(keys[DK_HIST + t]);
    summary[DS_HIST + 2u * t + 1u] = static_cast<uint32_t>(keys[DK_HIST + t] >> 32);
}

}  // namespace volym
