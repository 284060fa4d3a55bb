// The kernels of the components pass (volym_components_pass): the 6-connected components of the solid texels of a request, numbered
// in the order of their first texels, as one id per texel of the request's box and one record per component.  Included by
// components.hip alone.
//
// The work array is the id volume itself, parent[], indexed box-linear: i = (x - x0) + w * row, row = (y - y0) + h * (z - z0).  It is
// a union-find forest over texels, and the five steps below turn it into the ids in place: no second array of the volume's size.
//   The rows are walked as box_walk.h says, and a texel is solid by its predicate.  Every load and store is
// of a texel of the request's box, which volym_components_check puts inside the volume, or of parent[i] with i below the box's
// texel count.
//
// Invariants of parent[] from the end of the rows kernel to the end of the flatten kernel (a NONE word never changes):
//   (1) parent[i] <= i, always;
//   (2) every value ever stored in parent[i] is a member of i's final component;
//   (3) every store of the merge kernel is an atomicMin: a word only ever decreases, and there is no plain path-compression store.
// A load may be stale -- a CU's L1 is never refreshed by other CUs' stores -- and by (1) to (3) a stale value is only an older, larger
// ancestor of the same component: following it costs extra hops and never a wrong answer.  What decides is the RETURN VALUE of the
// atomic, which is the word's true content at that moment; no fence and no freshness of a load is relied on.  The merge is visible to
// the flatten kernel because that is a later launch.
#pragma once

#include "box_walk.h"

namespace volym {

struct ComponentsArgs : BoxWalkArgs {   // w * n_rows <= 2^31 - 2 (volym_components_check)
    uint32_t capacity;                  // records kept: components numbered below it
};

// Widths.  The box has at most 2^31 - 2 texels, so a box-linear index, a component's number, its count and every count of roots
// (a row's, a workgroup's per label, a row offset) is below 2^31 and fits a u32 with bit 31 to spare: the number kernel tags a
// root's word with that bit.  n_solid and the summary's counters are 64-bit where they are summed across workgroups.
constexpr uint32_t COMPONENT_NONE = VOLYM_COMPONENT_NONE;
constexpr uint32_t COMPONENT_TAG = 0x80000000u;     // a root's word between the number and the relabel kernel: TAG | number (never NONE: number <= 2^31 - 3)
// the working table: per kept component ten 32-bit words
enum { CW_ROOT_XY = 0, CW_ROOT_ZL = 1, CW_COUNT = 2, CW_FLAGS = 3, CW_MIN = 4, CW_MAX = 7, COMPONENT_WORK_WORDS = 10 };

// summary: struct volym_components_summary as 64-bit words
enum { CS_N_COMPONENTS = 0, CS_N_SOLID = 1, CS_RECORDED = 2, CS_PER_LABEL = 3, COMPONENT_SUMMARY_WORDS = 3 + 256 };

// zero summary (block 0) and an empty working table: counts and flags 0, the box inside out
__global__ __launch_bounds__(256) void volym_components_init_kernel(unsigned long long* summary, uint32_t* __restrict__ work, uint32_t n_records)
{
    if (blockIdx.x == 0u)
        for (uint32_t i = threadIdx.x; i < COMPONENT_SUMMARY_WORDS; i += 256u) summary[i] = 0ull;
    const uint32_t n_words = n_records * COMPONENT_WORK_WORDS;     // (n_records <= 2^24)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_words; i += gridDim.x * 256u) {
        const uint32_t f = i % COMPONENT_WORK_WORDS;
        work[i] = (f >= CW_MIN && f < CW_MAX) ? 0xffffffffu : 0u;
    }
}

// ---- 1. rows: every x-run of solid (and, SPLIT, equally labelled) texels points at its first texel; no atomic ---------------------
template <bool LABELS, bool SPLIT>
__global__ __launch_bounds__(256) void volym_components_rows_kernel(ComponentsArgs a, BoxSelect select, uint32_t* __restrict__ parent,
                                                                    unsigned long long* __restrict__ summary)
{
    __shared__ uint8_t s_select[256];
    s_select[threadIdx.x] = select.v[threadIdx.x];
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);        // bits 0..lane
    unsigned long long wave_solid = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t y = a.lo[1] + row % a.h, z = a.lo[2] + row / a.h;
        const uint32_t base = row * a.w;
        uint64_t carry = 0ull;                                     // bit 0: the last texel of the chunk before is solid
        uint32_t carry_label = 0u, carry_start = 0u;               // ... its label, and the first texel of its run
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < a.w;
            uint32_t label = 0u;
            bool solid = false;
            if (in) {
                solid = box_solid<LABELS>(a, s_select, layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z), label);
            }
            const uint64_t s = __ballot(solid);
            uint64_t link = s & ((s << 1) | carry);                // linked to the texel on the left
            if (SPLIT) {
                const uint32_t left = __shfl_up(label, 1);
                link &= __ballot(label == (lane == 0u ? carry_label : left));
            }
            // the run's first texel: the highest clear bit of the link mask at or below the lane; none: the run came in from the left
            const uint64_t clear = ~link & upto;
            const uint32_t start = clear ? base + x0 + (63u - static_cast<uint32_t>(__clzll(clear))) : carry_start;
            if (in) parent[base + xi] = solid ? start : COMPONENT_NONE;
            carry = s >> 63;
            carry_label = __shfl(label, 63);
            carry_start = __shfl(start, 63);
            wave_solid += static_cast<uint32_t>(__popcll(s));
        }
    }
    if (lane == 0u && wave_solid) atomicAdd(&summary[CS_N_SOLID], wave_solid);
}

// ---- 2. merge: the lock-free union over the y and z links ---------------------------------------------------------------------------
// Follows parent[] to a word that points at itself.  Each hop strictly decreases x (invariant 1), so it ends; the word may be stale and
// x no longer a root: the caller's atomic finds that out.
__device__ __forceinline__ uint32_t components_find(const uint32_t* parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = parent[x];
        if (p == x) return x;
        x = p;
    }
}

// Unites the trees of a and b.  The larger root is hooked under the smaller by atomicMin.  Its return value `old` is the word's true
// content: old == larger: it was a root and now points at `smaller` -- done.  Otherwise `larger` had a parent `old` already, and the
// word is now min(old, smaller): whichever of the two it does not hold any more must still be united with the other, so the loop
// goes on with `old` in place of `larger` -- the pair this call owes is (old, smaller), both members of the component (invariant 2).
// Every turn replaces the larger of the two indices by a strictly smaller one, so the loop ends; it waits for nobody.
__device__ __forceinline__ void components_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = components_find(parent, a);
        b = components_find(parent, b);
        if (a == b) return;
        const uint32_t larger = max(a, b), smaller = min(a, b);
        const uint32_t old = atomicMin(&parent[larger], smaller);
        if (old == larger) return;
        a = old;
        b = smaller;
    }
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void volym_components_merge_kernel(ComponentsArgs a, uint32_t* parent)
{
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slice = a.w * a.h;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        if (ry == 0u && rz == 0u) continue;                        // links never cross the request's box
        const uint32_t y = a.lo[1] + ry, z = a.lo[2] + rz;
        const uint32_t base = row * a.w;
        for (uint32_t xi = lane; xi < a.w; xi += 64u) {
            const uint32_t i = base + xi;
            if (parent[i] == COMPONENT_NONE) continue;             // (solidity never changes: a NONE word stays NONE)
            const uint32_t x = a.lo[0] + xi;
            const uint32_t label = SPLIT ? a.labels[layout_offset(a.bricked != 0u, bx, bxy, x, y, z)] : 0u;
            if (ry != 0u && parent[i - a.w] != COMPONENT_NONE &&
                (!SPLIT || a.labels[layout_offset(a.bricked != 0u, bx, bxy, x, y - 1u, z)] == label))
                components_unite(parent, i, i - a.w);
            if (rz != 0u && parent[i - slice] != COMPONENT_NONE &&
                (!SPLIT || a.labels[layout_offset(a.bricked != 0u, bx, bxy, x, y, z - 1u)] == label))
                components_unite(parent, i, i - slice);
        }
    }
}

// ---- 3. flatten: parent[i] = its root, the smallest index of i's component; and the roots of every row, counted --------------------
// A later launch than the merge, so the forest is complete and visible.  The stores here are plain: a word goes from an ancestor to the
// root, a root's word is never written, and a reader that meets either value reaches the same root.
__global__ __launch_bounds__(256) void volym_components_flatten_kernel(ComponentsArgs a, uint32_t* parent, uint32_t* __restrict__ rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t base = row * a.w;
        uint32_t n_roots = 0u;                                     // (wave-uniform; below 2^31)
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane, i = base + xi;
            bool root = false;
            if (xi < a.w) {
                const uint32_t p = parent[i];
                if (p != COMPONENT_NONE) {
                    const uint32_t r = components_find(parent, p);
                    if (r != p) parent[i] = r;
                    root = r == i;
                }
            }
            n_roots += static_cast<uint32_t>(__popcll(__ballot(root)));
        }
        if (lane == 0u) rows[row] = n_roots;
    }
}

// ---- 4. number: a root's number is its row's offset plus the roots before it in the row; no atomic decides a number -----------------
// Between the flatten and this kernel the host scans rows[] from counts into offsets (scan_row_offsets, box_pass.hip): rows[row] is now
// the number of the row's first root.  A root's word becomes TAG | number, and the root texel of a kept component goes
// into the working table.  Only the counters of the summary are atomics (integers: arrival order cannot show).
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_components_number_kernel(ComponentsArgs a, uint32_t* parent, const uint32_t* __restrict__ rows,
                                                                      uint32_t* __restrict__ work, unsigned long long* __restrict__ summary)
{
    __shared__ uint32_t s_per_label[256], s_roots;                 // a workgroup's roots: below 2^31
    s_per_label[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) s_roots = 0u;
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t wave_roots = 0u;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t y = a.lo[1] + row % a.h, z = a.lo[2] + row / a.h;
        const uint32_t base = row * a.w;
        uint32_t at = rows[row];                                   // wave-uniform
        const uint32_t first = at;
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane, i = base + xi;
            const bool root = xi < a.w && parent[i] == i;          // (NONE is no index of the box)
            const uint64_t r = __ballot(root);
            if (root) {
                const uint32_t number = at + static_cast<uint32_t>(__popcll(r & below));
                const uint32_t x = a.lo[0] + xi;
                const uint32_t label = LABELS ? a.labels[layout_offset(a.bricked != 0u, bx, bxy, x, y, z)] : 0u;
                parent[i] = COMPONENT_TAG | number;
                atomicAdd(&s_per_label[label], 1u);
                if (number < a.capacity) {
                    work[number * COMPONENT_WORK_WORDS + CW_ROOT_XY] = x | (y << 16);
                    work[number * COMPONENT_WORK_WORDS + CW_ROOT_ZL] = z | (label << 16);
                }
            }
            at += static_cast<uint32_t>(__popcll(r));
        }
        wave_roots += at - first;
    }
    if (lane == 0u && wave_roots) atomicAdd(&s_roots, wave_roots);
    __syncthreads();
    const uint32_t v = s_per_label[threadIdx.x];
    if (v) atomicAdd(&summary[CS_PER_LABEL + threadIdx.x], static_cast<unsigned long long>(v));
    if (threadIdx.x == 0u && s_roots) atomicAdd(&summary[CS_N_COMPONENTS], static_cast<unsigned long long>(s_roots));
}

// ---- 5. relabel and records ---------------------------------------------------------------------------------------------------------
// After the flatten every word of a solid texel that is no root holds its root's index, and since the number kernel a root's word is
// TAG | number.  Here a root stores its number, every other solid texel the number it reads in its root's word: that word is
// TAG | number or, once the root's own lane has stored, number -- the same 31 bits either way, so no order between the two matters
// and no last pass strips the tag.  Nobody reads a word of a texel that is no root but its own lane.
//   The records accumulate in the working table with integer atomics, as the measure pass accumulates: a lane carries one run of equal
// component and flushes it when the component changes and at the end.
__global__ __launch_bounds__(256) void volym_components_relabel_kernel(ComponentsArgs a, uint32_t* parent, uint32_t* __restrict__ work)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t cur = COMPONENT_NONE, count = 0u, flags = 0u, mn[3] = {0u, 0u, 0u}, mx[3] = {0u, 0u, 0u};
    auto flush = [&]() {
        if (cur == COMPONENT_NONE) return;
        uint32_t* rec = work + cur * COMPONENT_WORK_WORDS;          // (cur < capacity <= 2^24)
        atomicAdd(&rec[CW_COUNT], count);
        if (flags) atomicMax(&rec[CW_FLAGS], flags);
#pragma unroll
        for (int k = 0; k < 3; ++k) { atomicMin(&rec[CW_MIN + k], mn[k]); atomicMax(&rec[CW_MAX + k], mx[k]); }
    };
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t y = a.lo[1] + row % a.h, z = a.lo[2] + row / a.h;
        const uint32_t base = row * a.w;
        const bool edge_yz = y == a.lo[1] || y + 1u == a.hi[1] || z == a.lo[2] || z + 1u == a.hi[2];
        for (uint32_t xi = lane; xi < a.w; xi += 64u) {
            const uint32_t i = base + xi;
            const uint32_t v = parent[i];
            if (v == COMPONENT_NONE) continue;
            const uint32_t number = ((v & COMPONENT_TAG) ? v : parent[v]) & ~COMPONENT_TAG;
            parent[i] = number;
            if (number >= a.capacity) continue;                     // counted in the summary, no record
            const uint32_t t[3] = {a.lo[0] + xi, y, z};
            if (number != cur) {
                flush();
                cur = number; count = 0u; flags = 0u;
#pragma unroll
                for (int k = 0; k < 3; ++k) mn[k] = mx[k] = t[k];
            }
            ++count;
            flags |= (edge_yz || xi == 0u || xi + 1u == a.w) ? 1u : 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], t[k]); mx[k] = max(mx[k], t[k]); }
        }
    }
    // The last flush, which every lane reaches.  A large piece ends in the runs of most lanes of most waves, and so many atomics on the
    // eight words of one record queue up behind one another (measured: 96 % of the pass on a single piece at 256^3).  So where the lanes
    // of the wave that carry a run all carry the same component, the wave adds its runs up first and one lane flushes them.
    const uint64_t have = __ballot(cur != COMPONENT_NONE);
    if (have == 0ull) return;
    const uint32_t lead = __shfl(cur, static_cast<int>(__ffsll(static_cast<unsigned long long>(have))) - 1);      // wave-uniform
    if (__ballot(cur != COMPONENT_NONE && cur != lead) != 0ull) { flush(); return; }
    if (cur != lead) { count = 0u; flags = 0u; mn[0] = mn[1] = mn[2] = 0xffffffffu; mx[0] = mx[1] = mx[2] = 0u; }      // no run: the neutral elements
    for (int off = 32; off > 0; off >>= 1) {
        count += __shfl_xor(count, off);                            // (a wave's texels: below 2^31)
        flags |= __shfl_xor(flags, off);
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = min(mn[k], __shfl_xor(mn[k], off)); mx[k] = max(mx[k], __shfl_xor(mx[k], off)); }
    }
    cur = lane == 0u ? lead : COMPONENT_NONE;
    flush();
}

// the working table into the 24-byte records, six whole words each; and recorded = min(n_components, capacity)
__global__ __launch_bounds__(256) void volym_components_pack_kernel(const uint32_t* __restrict__ work, uint32_t* __restrict__ table,
                                                                    unsigned long long* __restrict__ summary, uint32_t capacity)
{
    const unsigned long long n = summary[CS_N_COMPONENTS];          // complete: the number kernel was an earlier launch
    const uint32_t recorded = n < capacity ? static_cast<uint32_t>(n) : capacity;
    if (blockIdx.x == 0u && threadIdx.x == 0u) summary[CS_RECORDED] = recorded;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < recorded; k += gridDim.x * 256u) {
        const uint32_t* w = work + k * COMPONENT_WORK_WORDS;
        uint32_t* out = table + k * 6u;
        out[0] = w[CW_ROOT_XY];
        out[1] = w[CW_ROOT_ZL] | (w[CW_FLAGS] << 24);               // z, label << 16, flags << 24
        out[2] = w[CW_COUNT];
        out[3] = w[CW_MIN] | (w[CW_MIN + 1] << 16);
        out[4] = w[CW_MIN + 2] | (w[CW_MAX] << 16);
        out[5] = w[CW_MAX + 1] | (w[CW_MAX + 2] << 16);
    }
}

}  // namespace volym
