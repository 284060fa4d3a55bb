// The kernels of the interpolate pass (volym_interpolate_pass: fill between slices) and of the edit by it (volym_interpolate_labels).
// Included by interpolate.hip alone.
//
// The pass (include/volym_hip.h states the rule): the SLICES of a request's box are its planes perpendicular to `axis`; on every KEY
// slice the planar distance transform of SHAPE, outside (Dout: to the nearest SHAPE texel of the slice) and inside (Din: to the nearest
// texel of the slice that is not SHAPE, the box's border included); on every slice of a fillable gap the comparison of the two keys
// about it.  It is the distance pass's separable transform (distance_kernels.h) run per plane and twice:
//   init     zeroes the summary and the SHAPE counts per slice.
//   rows     one wave per x-row of the box, one ballot per 64-texel chunk: the SHAPE bit of the state byte, the row distances of both
//            maps (axis y or z) or 0 / NONE (axis x, where a row crosses the slices), and the SHAPE texels per slice -- one atomic per
//            row and wave, or through an LDS histogram when every x is another slice.
//   keys     one workgroup: which slices are keys (the counts, or the request's bits), the two keys about every other slice, the kind of
//            every slice and the gap counts, straight into the public summary.
//   columns  the distance pass's lower-envelope sweep, one lane per column and adjacent lanes on adjacent x, along the in-plane axes the
//            rows have not covered: y (axis z), z (axis y), y and then z (axis x); once per map.  A column whose plane is no key returns
//            at once.  The sweep exists a third time here because the distance pass's header is pinned to its unit.
//   resolve  one wave per row: the signed word and the state byte of every texel; for a texel of a fillable gap the four words at its
//            in-plane position in the two keys and the 64-bit comparison.  Counts per wave, then per workgroup.
// The signed map is stored over the first stack of the column sweeps, which is free by then: resolve reads Dout and Din only, so no
// wave reads a word another wave of the same launch writes.
// Widths.  A box has at most 2^31 - 2 texels: every box-linear index fits 31 bits.  An axis has at most 4096 texels and a weight is at
// most 64, so every D the sweeps compare or store is at most 2 * 64 * 4095^2 = 2146435200 < 2^31: exact in uint32_t, and D << 1 | 1
// fits.  a, b < 4096, so a^2 D < 2^24 * 2^31: exact in uint64_t.  A slice has at most 4096^2 = 2^24 texels: a count fits uint32_t.
// Every load and store is of a texel of the request's box, which volym_interpolate_check puts inside the volume, or of an element of
// the maps and work arrays with an index below the box's texel count: a gap texel's key positions differ from its own only along
// `axis`, by key_lo and key_hi, which the keys kernel takes from the slices of the box.
//
// The edit: an edit kernel built from the pieces of edit_chunks.h, in place, whose new label comes from one of two tables by the
// snapshot's state byte.
#pragma once

#include "box_walk.h"
#include "edit_chunks.h"

namespace volym {

struct InterpolateArgs : BoxWalkArgs {  // w * n_rows <= 2^31 - 2 (volym_interpolate_check)
    uint32_t weight[3];
    uint32_t axis;                      // 0, 1, 2
    uint32_t max_gap, use_keys;
};

// the request's key bits, passed by value
struct InterpolateKeys { uint32_t v[VOLYM_INTERPOLATE_SLICES / 32]; };

constexpr uint32_t INTERPOLATE_NONE = VOLYM_INTERPOLATE_NONE;
constexpr uint32_t INTERPOLATE_SLICES = VOLYM_INTERPOLATE_SLICES;
// struct volym_interpolate_summary as 32-bit words (the 64-bit counters at even words), a slice record as four
enum { IS_N_SLICES = 0, IS_N_KEYS = 1, IS_N_GAPS = 2, IS_N_GAP_SLICES = 3, IS_N_REFUSED = 4, IS_N_SHAPE = 6, IS_N_INSIDE = 8, IS_N_NEW = 10, IS_N_STALE = 12,
       IS_SLICE = 14, INTERPOLATE_SUMMARY_WORDS = 14 + 4 * VOLYM_INTERPOLATE_SLICES };
enum { ISL_KIND = 0, ISL_KEY_LO = 1, ISL_KEY_HI = 2, ISL_COUNT = 3 };

// the extent of the box along the request's axis, and the stride of a step along it in a box-linear map
__device__ __forceinline__ uint32_t interpolate_slices(const InterpolateArgs& a)
{
    return a.axis == 0u ? a.w : a.axis == 1u ? a.h : a.hi[2] - a.lo[2];
}

// The summary and the counts at rest (what an empty box leaves).  One workgroup.
__global__ __launch_bounds__(256) void volym_interpolate_init_kernel(uint32_t* __restrict__ summary, uint32_t* __restrict__ counts)
{
    for (uint32_t i = threadIdx.x; i < INTERPOLATE_SUMMARY_WORDS; i += 256u) summary[i] = 0u;
    for (uint32_t i = threadIdx.x; i < INTERPOLATE_SLICES; i += 256u) counts[i] = 0u;
}

// ---- 1. rows ----------------------------------------------------------------------------------------------------------------------------
// The distance pass's row sweep for two seed sets at once: Dout's seeds are the SHAPE texels, Din's the texels of the row that are not
// (the border along x is the resolve kernel's).  Left to right both maps get dl, the distance to the nearest seed at or left of the texel
// (NONE: none); dl == 0 marks the seeds, so the sweep back from the right needs no second look at the scene's bytes.  AXIS_X: every
// texel of a row lies in another slice, so there is no distance along the row: 0 on a seed, NONE elsewhere.
template <bool LABELS, bool AXIS_X>
__global__ __launch_bounds__(256) void volym_interpolate_rows_kernel(InterpolateArgs a, BoxSelect select, uint32_t* __restrict__ dout, uint32_t* __restrict__ din,
                                                                     uint8_t* __restrict__ state, uint32_t* __restrict__ counts)
{
    __shared__ uint8_t s_select[256];
    __shared__ uint32_t s_count[AXIS_X ? INTERPOLATE_SLICES : 1u];
    s_select[threadIdx.x] = select.v[threadIdx.x];
    if (AXIS_X)
        for (uint32_t i = threadIdx.x; i < INTERPOLATE_SLICES; i += 256u) s_count[i] = 0u;
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);        // bits 0..lane
    const uint64_t from = ~0ull << lane;                                        // bits lane..63
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        const uint32_t y = a.lo[1] + ry, z = a.lo[2] + rz;
        const uint32_t base = row * a.w;
        uint32_t carry_out = INTERPOLATE_NONE, carry_in = INTERPOLATE_NONE;     // x of the last seed of the chunks before (wave-uniform)
        uint32_t row_shape = 0u;
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < a.w;
            bool shape = false;
            if (in) {
                uint32_t label;
                shape = box_solid<LABELS>(a, s_select, layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z), label);
                state[base + xi] = shape ? static_cast<uint8_t>(VOLYM_INTERPOLATE_SHAPE) : static_cast<uint8_t>(0u);
            }
            const uint64_t so = __ballot(shape), si = __ballot(in && !shape);
            if (AXIS_X) {
                if (in) {
                    dout[base + xi] = shape ? 0u : INTERPOLATE_NONE;
                    din[base + xi] = shape ? INTERPOLATE_NONE : 0u;
                }
                if (shape) atomicAdd(&s_count[xi], 1u);                         // (64 lanes, 64 words)
            } else {
                const uint64_t lo_ = so & upto, li = si & upto;
                const uint32_t at_o = lo_ ? x0 + (63u - static_cast<uint32_t>(__clzll(lo_))) : carry_out;
                const uint32_t at_i = li ? x0 + (63u - static_cast<uint32_t>(__clzll(li))) : carry_in;
                if (in) {
                    dout[base + xi] = at_o == INTERPOLATE_NONE ? INTERPOLATE_NONE : xi - at_o;
                    din[base + xi] = at_i == INTERPOLATE_NONE ? INTERPOLATE_NONE : xi - at_i;
                }
                if (so) carry_out = x0 + (63u - static_cast<uint32_t>(__clzll(so)));
                if (si) carry_in = x0 + (63u - static_cast<uint32_t>(__clzll(si)));
                row_shape += static_cast<uint32_t>(__popcll(so));
            }
        }
        if (AXIS_X) continue;
        // back from the right (each lane reads the words it stored itself); chunk k starts at 64 * k
        carry_out = carry_in = INTERPOLATE_NONE;
        for (uint32_t k = (a.w + 63u) / 64u; k-- > 0u;) {
            const uint32_t x0 = k * 64u, xi = x0 + lane;
            const bool in = xi < a.w;
            const uint32_t dl_o = in ? dout[base + xi] : INTERPOLATE_NONE, dl_i = in ? din[base + xi] : INTERPOLATE_NONE;
            const uint64_t so = __ballot(in && dl_o == 0u), si = __ballot(in && dl_i == 0u);
            const uint64_t ro = so & from, ri = si & from;
            const uint32_t at_o = ro ? x0 + static_cast<uint32_t>(__builtin_ctzll(ro)) : carry_out;
            const uint32_t at_i = ri ? x0 + static_cast<uint32_t>(__builtin_ctzll(ri)) : carry_in;
            const uint32_t mo = min(dl_o, at_o == INTERPOLATE_NONE ? INTERPOLATE_NONE : at_o - xi);      // at most 4095, or NONE
            const uint32_t mi = min(dl_i, at_i == INTERPOLATE_NONE ? INTERPOLATE_NONE : at_i - xi);
            if (in) {
                dout[base + xi] = mo == INTERPOLATE_NONE ? INTERPOLATE_NONE : a.weight[0] * mo * mo;
                din[base + xi] = mi == INTERPOLATE_NONE ? INTERPOLATE_NONE : a.weight[0] * mi * mi;
            }
            if (so) carry_out = x0 + static_cast<uint32_t>(__builtin_ctzll(so));
            if (si) carry_in = x0 + static_cast<uint32_t>(__builtin_ctzll(si));
        }
        if (lane == 0u && row_shape) atomicAdd(&counts[a.axis == 2u ? rz : ry], row_shape);
    }
    if (AXIS_X) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < a.w; i += 256u)                      // only the slices this workgroup touched go to memory
            if (s_count[i]) atomicAdd(&counts[i], s_count[i]);
    }
}

// ---- 2. keys: the kind of every slice and the two keys about it -----------------------------------------------------------------------
// One workgroup.  Thread 0 walks the slices once up and once down through LDS (at most 8192 steps); everything else is per slice.
__global__ __launch_bounds__(256) void volym_interpolate_keys_kernel(InterpolateArgs a, InterpolateKeys keys, const uint32_t* __restrict__ counts,
                                                                     uint32_t* __restrict__ summary)
{
    __shared__ uint8_t s_key[INTERPOLATE_SLICES];
    __shared__ uint16_t s_lo[INTERPOLATE_SLICES], s_hi[INTERPOLATE_SLICES];     // the key at or below, at or above (0xffff: none)
    __shared__ uint32_t s_tot[5];                                               // keys, gaps, gap slices, refused gaps, SHAPE texels
    const uint32_t n = interpolate_slices(a), first = a.lo[a.axis];
    if (threadIdx.x < 5u) s_tot[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t shape = 0u;                                                        // (the box has fewer than 2^31 texels)
    for (uint32_t k = threadIdx.x; k < n; k += 256u) {
        const uint32_t cnt = counts[k], at = first + k;
        shape += cnt;
        s_key[k] = (a.use_keys ? ((keys.v[at >> 5] >> (at & 31u)) & 1u) != 0u : cnt != 0u) ? 1u : 0u;
    }
    if (shape) atomicAdd(&s_tot[4], shape);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t last = 0xffffu;
        for (uint32_t k = 0u; k < n; ++k) { if (s_key[k]) last = k; s_lo[k] = static_cast<uint16_t>(last); }
        last = 0xffffu;
        for (uint32_t k = n; k-- > 0u;) { if (s_key[k]) last = k; s_hi[k] = static_cast<uint16_t>(last); }
    }
    __syncthreads();
    uint32_t n_keys = 0u, n_gaps = 0u, n_gap_slices = 0u, n_refused = 0u;
    for (uint32_t k = threadIdx.x; k < n; k += 256u) {
        const uint32_t lo = s_lo[k], hi = s_hi[k];
        uint32_t kind = VOLYM_INTERPOLATE_SLICE_OUTSIDE, key_lo = INTERPOLATE_NONE, key_hi = INTERPOLATE_NONE, count = 0u;
        if (s_key[k]) {
            kind = VOLYM_INTERPOLATE_SLICE_KEY; key_lo = key_hi = first + k; count = counts[k];
            ++n_keys;
        } else if (lo != 0xffffu && hi != 0xffffu) {
            const bool refused = a.max_gap != 0u && hi - lo - 1u > a.max_gap;
            kind = refused ? VOLYM_INTERPOLATE_SLICE_REFUSED : VOLYM_INTERPOLATE_SLICE_GAP;
            key_lo = first + lo; key_hi = first + hi;
            if (!refused) ++n_gap_slices;
            if (k == lo + 1u) { if (refused) ++n_refused; else ++n_gaps; }     // the first slice of its run
        }
        uint32_t* const rec = summary + IS_SLICE + 4u * k;
        rec[ISL_KIND] = kind; rec[ISL_KEY_LO] = key_lo; rec[ISL_KEY_HI] = key_hi; rec[ISL_COUNT] = count;
    }
    if (n_keys) atomicAdd(&s_tot[0], n_keys);
    if (n_gaps) atomicAdd(&s_tot[1], n_gaps);
    if (n_gap_slices) atomicAdd(&s_tot[2], n_gap_slices);
    if (n_refused) atomicAdd(&s_tot[3], n_refused);
    __syncthreads();
    if (threadIdx.x == 0u) {
        summary[IS_N_SLICES] = n;
        summary[IS_N_KEYS] = s_tot[0]; summary[IS_N_GAPS] = s_tot[1]; summary[IS_N_GAP_SLICES] = s_tot[2]; summary[IS_N_REFUSED] = s_tot[3];
        summary[IS_N_SHAPE] = s_tot[4];                                         // (the high word stays 0)
    }
}

// ---- 3. columns: in place, f(i) = min_j g(j) + w * (i - j)^2 over the finite g(j), in the planes of the key slices -------------------
// floor(num / den) for 0 <= num < 2^34, 0 < den < 2^20, as the distance pass takes it: the f64 quotient only proposes, the two loops
// settle it in integers.
__device__ __forceinline__ uint32_t interpolate_floor_div(uint64_t num, uint32_t den)
{
    uint32_t q = static_cast<uint32_t>(static_cast<double>(num) / static_cast<double>(den));
    while (static_cast<uint64_t>(q) * den > num) --q;
    while (static_cast<uint64_t>(q + 1u) * den <= num) ++q;
    return q;
}

struct InterpolateColumns {
    uint32_t n;                         // entries of a column (the box's extent along the swept axis), 2..4096
    uint32_t stride;                    // words between two entries of a column
    uint32_t n_cols;                    // columns: the texels of the box / n
    uint32_t inner, outer;              // column c starts at word c % inner + (c / inner) * outer
    uint32_t weight;
    uint32_t slice_div, slice_mod;      // column c lies in slice (c / slice_div) % slice_mod of the box
};

// The stacks lie entry-major beside the map, as in the distance pass: entry k of the column that starts at `base` is word
// base + k * stride of each of the two work arrays, (site | first index it wins from << 16) and the site's g.
__global__ __launch_bounds__(64) void volym_interpolate_columns_kernel(InterpolateColumns a, const uint32_t* __restrict__ summary, uint32_t* __restrict__ map,
                                                                       uint32_t* __restrict__ stack, uint32_t* __restrict__ stack_g)
{
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.n_cols) return;
    if (summary[IS_SLICE + 4u * ((c / a.slice_div) % a.slice_mod) + ISL_KIND] != VOLYM_INTERPOLATE_SLICE_KEY) return;
    const uint32_t base = c % a.inner + (c / a.inner) * a.outer;
    const uint32_t w = a.weight;
    // the stack's top in registers: site, the first index it wins from, the site's g
    int q = -1;
    uint32_t top_s = 0u, top_t = 0u, top_g = 0u;
    for (uint32_t u = 0u; u < a.n; ++u) {
        const uint32_t g = map[base + u * a.stride];
        if (g == INTERPOLATE_NONE) continue;                        // no parabola
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
            first = interpolate_floor_div(num, 2u * w * (u - top_s)) + 1u;
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

// ---- 4. resolve: the signed word and the state byte of every texel ---------------------------------------------------------------------
// A texel is SHAPE iff its Dout is 0.  Din gets the border here: texels outside the box count as not SHAPE, and the nearest of them
// lies straight across the nearer side of each in-plane axis.  A gap texel and its two key positions share their in-plane
// coordinates, so one border serves the three.
template <bool AXIS_X>
__global__ __launch_bounds__(256) void volym_interpolate_resolve_kernel(InterpolateArgs a, const uint32_t* __restrict__ dout, const uint32_t* __restrict__ din,
                                                                        uint32_t* __restrict__ map, uint8_t* __restrict__ state, uint32_t* __restrict__ summary)
{
    __shared__ uint32_t s_count[AXIS_X ? INTERPOLATE_SLICES : 1u];
    __shared__ unsigned long long s_tot[3];                                     // inside, new, stale
    if (AXIS_X)
        for (uint32_t i = threadIdx.x; i < INTERPOLATE_SLICES; i += 256u) s_count[i] = 0u;
    if (threadIdx.x < 3u) s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = a.hi[2] - a.lo[2];
    const uint32_t stride = a.axis == 0u ? 1u : a.axis == 1u ? a.w : a.w * a.h;
    const uint32_t first = a.lo[a.axis];
    uint32_t wave_inside = 0u, wave_new = 0u, wave_stale = 0u;                   // (a wave walks at most 4096 rows of 4096 texels)
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        const uint32_t base = row * a.w;
        const uint32_t by = min(ry + 1u, a.h - ry), bz = min(rz + 1u, d - rz);
        const uint32_t border_y = a.weight[1] * by * by, border_z = a.weight[2] * bz * bz;
        uint32_t row_inside = 0u;
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane, i = base + xi;
            const bool in = xi < a.w;
            const uint32_t s = AXIS_X ? xi : (a.axis == 2u ? rz : ry);
            bool gap = false, inside = false, shape = false;
            if (in) {
                const uint32_t* const rec = summary + IS_SLICE + 4u * s;
                const uint32_t kind = rec[ISL_KIND];
                const uint32_t b = min(xi + 1u, a.w - xi), border_x = a.weight[0] * b * b;
                const uint32_t border = a.axis == 0u ? min(border_y, border_z) : a.axis == 1u ? min(border_x, border_z) : min(border_x, border_y);
                uint32_t word = INTERPOLATE_NONE;
                uint32_t st = state[i] & static_cast<uint32_t>(VOLYM_INTERPOLATE_SHAPE);
                shape = st != 0u;
                if (kind == VOLYM_INTERPOLATE_SLICE_KEY) {
                    const uint32_t o = dout[i];
                    if (o == 0u) { word = (min(din[i], border) << 1) | 1u; st |= VOLYM_INTERPOLATE_INSIDE; }
                    else if (o != INTERPOLATE_NONE) word = o << 1;
                } else if (kind == VOLYM_INTERPOLATE_SLICE_GAP) {
                    gap = true;
                    const uint32_t z0 = rec[ISL_KEY_LO] - first, z1 = rec[ISL_KEY_HI] - first;      // z0 < s < z1 < the slices of the box
                    const uint32_t i0 = i - (s - z0) * stride, i1 = i + (z1 - s) * stride;
                    const uint32_t o0 = dout[i0], o1 = dout[i1];
                    const uint64_t a2 = static_cast<uint64_t>(z1 - s) * (z1 - s), b2 = static_cast<uint64_t>(s - z0) * (s - z0);
                    if (o0 == 0u && o1 == 0u) inside = true;
                    else if (o0 == 0u && o1 != INTERPOLATE_NONE) inside = a2 * min(din[i0], border) > b2 * o1;
                    else if (o1 == 0u && o0 != INTERPOLATE_NONE) inside = b2 * min(din[i1], border) > a2 * o0;
                    st |= VOLYM_INTERPOLATE_GAP | (inside ? static_cast<uint32_t>(VOLYM_INTERPOLATE_INSIDE) : 0u);
                }
                map[i] = word;
                state[i] = static_cast<uint8_t>(st);
            }
            const uint64_t bi = __ballot(inside);
            if (AXIS_X) { if (inside) atomicAdd(&s_count[xi], 1u); }
            else row_inside += static_cast<uint32_t>(__popcll(bi));
            wave_inside += static_cast<uint32_t>(__popcll(bi));
            wave_new += static_cast<uint32_t>(__popcll(__ballot(inside && !shape)));
            wave_stale += static_cast<uint32_t>(__popcll(__ballot(gap && !inside && shape)));
        }
        if (!AXIS_X && lane == 0u && row_inside) atomicAdd(&summary[IS_SLICE + 4u * (a.axis == 2u ? rz : ry) + ISL_COUNT], row_inside);
    }
    if (lane == 0u) {
        if (wave_inside) atomicAdd(&s_tot[0], static_cast<unsigned long long>(wave_inside));
        if (wave_new) atomicAdd(&s_tot[1], static_cast<unsigned long long>(wave_new));
        if (wave_stale) atomicAdd(&s_tot[2], static_cast<unsigned long long>(wave_stale));
    }
    __syncthreads();
    if (AXIS_X)
        for (uint32_t i = threadIdx.x; i < a.w; i += 256u)
            if (s_count[i]) atomicAdd(&summary[IS_SLICE + 4u * i + ISL_COUNT], s_count[i]);
    if (threadIdx.x < 3u && s_tot[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(summary + IS_N_INSIDE) + threadIdx.x, s_tot[threadIdx.x]);
}

// out (box-linear in the sub-box, x fastest) = the bytes of a box-linear byte volume of width w and height h, from element `first`
// on: one thread per byte (volym_read_interpolate_state of a sub-box that is no run of whole slices)
__global__ __launch_bounds__(256) void volym_interpolate_gather_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, uint32_t w, uint32_t h,
                                                                       uint32_t first, uint32_t sw, uint32_t sh, uint32_t total)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    out[i] = src[first + i % sw + w * ((i / sw) % sh + h * (i / (sw * sh)))];
}

// ---- the edit (volym_interpolate_labels) -------------------------------------------------------------------------------------------------
// what the rule reads beside the marks: the window, the two tables, and the pass's box
struct InterpolateRule {
    uint32_t min_byte, max_byte;
    uint32_t store;                 // 0: DRY_RUN
    uint32_t box[6];                // the box of the interpolate pass: the state map is linear in it, and the request's box lies inside it
    uint8_t to[256], out[256];
};

// One pass over the items of the request's slab, as the fill walks it (nearest_kernels.h): a lane at a time, the 16 labels first.  The
// table `marks` only marks the labels either table moves (marks[l] != l iff to[l] != l or out[l] != l), for chunk_candidates; a chunk
// without such a texel in the box loads nothing more.  Else the density, then per candidate its state byte from the snapshot: with GAP
// it becomes to[l] where INSIDE is set and out[l] where it is not.  The chunk is stored only if a byte changed and rule.store says so;
// every texel is decided from the snapshot and the bytes before the edit.
template <bool JOURNAL>
__device__ __forceinline__ void interpolate_edit_pass(RelabelShared& sh, uint8_t* s_to, uint8_t* s_out, uint4* __restrict__ labels, const uint4* __restrict__ vol,
                                                      const uint8_t* __restrict__ state, const RelabelOut& out, const LabelTable& marks, const CropSlab& s,
                                                      const InterpolateRule& rule, const LabelJournal& journal, uint32_t nx, uint32_t ny, uint32_t nz,
                                                      uint32_t bricked, uint32_t n_items)
{
    s_to[threadIdx.x] = rule.to[threadIdx.x];
    s_out[threadIdx.x] = rule.out[threadIdx.x];
    edit_prologue(sh, marks);
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint32_t bx = brick_count(nx), by = brick_count(ny);
    RelabelTally t;

    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_items; i += gridDim.x * 256u) {
        uint64_t k;
        uint32_t keep, moved;
        if (!crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, keep, moved)) continue;
        if (!bricked && !relabel_owns_chunk(s, i, nx, ny, k)) continue;
        if (!keep) continue;                                             // before any load
        const uint4 lv = labels[k];
        uint32_t lb[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t cand = chunk_candidates(sh, lb, keep);
        if (!cand) continue;                                             // no density, no snapshot, no store
        cand = chunk_in_window(vol[k], rule.min_byte, rule.max_byte, cand);
        if (!cand) continue;
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);      // (k < 2^28: a layout has fewer than 2^32 bytes)
        bool stored = false;
        ChunkCursor c = {x0, y0, z0};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            c.at(bricked, j, x0, y0);
            if (cand & (1u << j)) {
                const uint32_t st = state[box_linear(rule.box, c.x, c.y, c.z)];
                if (st & VOLYM_INTERPOLATE_GAP) {
                    const uint32_t shift = 8u * (j & 3u), l = (lb[j >> 2] >> shift) & 0xffu;
                    const uint32_t becomes = (st & VOLYM_INTERPOLATE_INSIDE) ? s_to[l] : s_out[l];
                    if (becomes != l) {
                        lb[j >> 2] = (lb[j >> 2] & ~(0xffu << shift)) | (becomes << shift);
                        tally_texel(sh, t, l, becomes, c.x, c.y, c.z);
                        stored = true;
                    }
                }
            }
            c.next(bricked, nx, ny);
        }
        if (stored && rule.store) chunk_store<JOURNAL>(labels, k, lv, lb, journal);
    }
    tally_reduce(sh, t, out);
}

__global__ __launch_bounds__(256) void volym_interpolate_edit_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint8_t* __restrict__ state,
                                                                     RelabelOut out, LabelTable marks, CropSlab s, InterpolateRule rule, uint32_t nx, uint32_t ny,
                                                                     uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ uint8_t s_to[256], s_out[256];
    interpolate_edit_pass<false>(sh, s_to, s_out, labels, vol, state, out, marks, s, rule, LabelJournal{}, nx, ny, nz, bricked, n_items);
}

// the same edit while the history is on and the request is no DRY_RUN
__global__ __launch_bounds__(256) void volym_interpolate_edit_journal_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol,
                                                                             const uint8_t* __restrict__ state, RelabelOut out, LabelTable marks, CropSlab s,
                                                                             InterpolateRule rule, LabelJournal journal, uint32_t nx, uint32_t ny, uint32_t nz,
                                                                             uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    __shared__ uint8_t s_to[256], s_out[256];
    interpolate_edit_pass<true>(sh, s_to, s_out, labels, vol, state, out, marks, s, rule, journal, nx, ny, nz, bricked, n_items);
}

}  // namespace volym
