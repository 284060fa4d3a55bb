// What every label-edit kernel is made of, here once for the relabel (relabel_kernels.h), the brush (brush_kernels.h), the lasso
// (lasso_kernels.h), the smoothing's vote (smooth_kernels.h), the fill (nearest_kernels.h) and the flood (geodesic_kernels.h): the result's tally, the journal, the pieces of a chunk's edit
// (edit_prologue, ChunkCursor, chunk_candidates, chunk_in_window, chunk_apply, chunk_store) and the wave-at-a-time walk and tail of
// the passes that select by geometry (wave_chunk_step, selected_chunk_tail), over the chunk walk of scene_chunks.h.  Device functions
// and the structs they read only: no __global__ function, so every edit's unit includes it.
#pragma once

#include "scene_chunks.h"

namespace volym {

// The working result in device memory: volym_relabel_result as the kernel accumulates it.  The caller sets lo = 0xffffffff and
// hi = 0 (the INCLUSIVE maxima) and zeroes the counts; the host turns the hull into the result's box.
struct RelabelOut {
    unsigned long long* changed;    // [1]
    unsigned long long* left;       // [256]
    unsigned long long* arrived;    // [256]
    uint32_t* box;                  // [6]
};

// Does linear item i own its chunk k?  Two runs may share a chunk (scene_chunks.h). The rewrite kernels do not mind: both lanes
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

// What a workgroup of the relabel and swap kernels keeps in LDS: the table (relabel only) and its share of the result.
struct RelabelShared {
    uint8_t to[256];
    uint32_t left[256], arrived[256];
    uint32_t changed, box[6];
};

// What a lane keeps in registers: its changed texels, their hull, and one run of equal (old label, new label) pairs, keyed
// old | new << 8, whose length it flushes when the pair changes and once at the end (TALLY_NONE: no run yet).
constexpr uint32_t TALLY_NONE = 0x10000u;
struct RelabelTally {
    uint32_t changed = 0, lo_x = 0xffffffffu, lo_y = 0xffffffffu, lo_z = 0xffffffffu, hi_x = 0, hi_y = 0, hi_z = 0;
    uint32_t cur = TALLY_NONE, cnt = 0;
};

__device__ __forceinline__ void tally_init(RelabelShared& sh)
{
    const uint32_t l = threadIdx.x;
    sh.left[l] = sh.arrived[l] = 0u;
    if (l == 0u) sh.changed = 0u;
    if (l < 6u) sh.box[l] = l < 3u ? 0xffffffffu : 0u;
}

__device__ __forceinline__ void tally_flush(RelabelShared& sh, const RelabelTally& t)
{
    if (t.cur >= TALLY_NONE) return;
    atomicAdd(&sh.left[t.cur & 0xffu], t.cnt);
    atomicAdd(&sh.arrived[t.cur >> 8], t.cnt);
}

// texel (x, y, z) went from label `from` to label `to`
__device__ __forceinline__ void tally_texel(RelabelShared& sh, RelabelTally& t, uint32_t from, uint32_t to, uint32_t x, uint32_t y, uint32_t z)
{
    const uint32_t key = from | (to << 8);
    if (key != t.cur) { tally_flush(sh, t); t.cur = key; t.cnt = 0u; }
    ++t.cnt; ++t.changed;
    t.lo_x = min(t.lo_x, x); t.lo_y = min(t.lo_y, y); t.lo_z = min(t.lo_z, z);
    t.hi_x = max(t.hi_x, x); t.hi_y = max(t.hi_y, y); t.hi_z = max(t.hi_z, z);
}

// The epilogue of both kernels; every lane of the workgroup calls it, after its loop has ended.  The waves add up first: changed
// and the hull by shuffles, and the runs too where the whole wave carries the same pair (a merge of one segment: every lane) -- one
// LDS atomic per wave and word instead of 64 on the same word.  After the barrier thread l adds the workgroup's left[l] and
// arrived[l] to the global result and thread 0 the count and the hull: one global atomic per non-zero word and workgroup.  All
// integer adds and min/max: the result does not depend on arrival order.  A workgroup holds fewer texels than a layout has bytes
// (< 2^32): u32 in LDS.
__device__ __forceinline__ void tally_reduce(RelabelShared& sh, const RelabelTally& t, const RelabelOut& out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w_changed = wave_sum(t.changed);
    if (w_changed != 0u) {                                               // (wave-uniform)
        const uint32_t a = wave_min(t.lo_x), b = wave_min(t.lo_y), c = wave_min(t.lo_z), d = wave_max(t.hi_x), e = wave_max(t.hi_y), f = wave_max(t.hi_z);
        const unsigned long long have = __ballot(t.cur < TALLY_NONE);
        const uint32_t first = static_cast<uint32_t>(__ffsll(have)) - 1u;
        const uint32_t ref = __shfl(t.cur, static_cast<int>(first), 64);
        if (__all(t.cur >= TALLY_NONE || t.cur == ref)) {
            const uint32_t total = wave_sum(t.cur < TALLY_NONE ? t.cnt : 0u);
            if (lane == first) { atomicAdd(&sh.left[ref & 0xffu], total); atomicAdd(&sh.arrived[ref >> 8], total); }
        } else {
            tally_flush(sh, t);
        }
        if (lane == 0u) {
            atomicAdd(&sh.changed, w_changed);
            atomicMin(&sh.box[0], a); atomicMin(&sh.box[1], b); atomicMin(&sh.box[2], c);
            atomicMax(&sh.box[3], d); atomicMax(&sh.box[4], e); atomicMax(&sh.box[5], f);
        }
    }
    __syncthreads();
    const uint32_t l = threadIdx.x;
    if (sh.left[l] != 0u) atomicAdd(&out.left[l], static_cast<unsigned long long>(sh.left[l]));
    if (sh.arrived[l] != 0u) atomicAdd(&out.arrived[l], static_cast<unsigned long long>(sh.arrived[l]));
    if (l == 0u && sh.changed != 0u) {
        atomicAdd(out.changed, static_cast<unsigned long long>(sh.changed));
        for (int a = 0; a < 3; ++a) atomicMin(&out.box[a], sh.box[a]);
        for (int a = 3; a < 6; ++a) atomicMax(&out.box[a], sh.box[a]);
    }
}

// The journal an edit appends to while the history is on (volym_label_history): per stored chunk its index and its 16 bytes before
// the edit, as two arrays.  *count runs past capacity when the journal is too small; a record at or past capacity is not written.
struct LabelJournal {
    uint32_t* index;
    uint4* old;
    uint32_t* count;
    uint32_t capacity;
};

// ---- what the edit passes share: relabel_pass below, brush_pass (brush_kernels.h), lasso_pass (lasso_kernels.h) ------------------------

// every pass begins so: the table and an empty tally in LDS
__device__ __forceinline__ void edit_prologue(RelabelShared& sh, const LabelTable& to)
{
    sh.to[threadIdx.x] = to.v[threadIdx.x];
    tally_init(sh);
    __syncthreads();
}

// The texel of byte j of a chunk whose first texel is (x0, y0, z0), in either layout: built at that texel, put at byte j before the
// byte is looked at (a brick is a 4 x 4 patch of one z) and moved on after it (a linear chunk runs along x and wraps rows and slices).
struct ChunkCursor {
    uint32_t x, y, z;
    __device__ __forceinline__ void at(uint32_t bricked, uint32_t j, uint32_t x0, uint32_t y0) { if (bricked) { x = x0 + (j & 3u); y = y0 + (j >> 2); } }
    __device__ __forceinline__ void next(uint32_t bricked, uint32_t nx, uint32_t ny) { if (!bricked && ++x == nx) { x = 0u; if (++y == ny) { y = 0u; ++z; } } }
};

// the texels of `mask` whose label the table moves: bit j for byte j of the 16 labels lb
__device__ __forceinline__ uint32_t chunk_candidates(const RelabelShared& sh, const uint32_t lb[4], uint32_t mask)
{
    uint32_t cand = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t l = (lb[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        if (sh.to[l] != l) cand |= 1u << j;
    }
    return cand & mask;
}

// ... and of those, the ones whose density byte lies in the window
__device__ __forceinline__ uint32_t chunk_in_window(const uint4& dv, uint32_t min_byte, uint32_t max_byte, uint32_t cand)
{
    const uint32_t d[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t b = (d[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        if (b < min_byte || b > max_byte) cand &= ~(1u << j);
    }
    return cand;
}

// Apply and tally: each candidate texel gets its new label in lb and is counted.  The chunk's first texel is (x0, y0, z0).
__device__ __forceinline__ void chunk_apply(RelabelShared& sh, RelabelTally& t, uint32_t lb[4], uint32_t cand, uint32_t bricked, uint32_t x0, uint32_t y0, uint32_t z0,
                                            uint32_t nx, uint32_t ny)
{
    ChunkCursor c = {x0, y0, z0};
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        c.at(bricked, j, x0, y0);
        if (cand & (1u << j)) {
            const uint32_t shift = 8u * (j & 3u), l = (lb[j >> 2] >> shift) & 0xffu, becomes = sh.to[l];
            lb[j >> 2] = (lb[j >> 2] & ~(0xffu << shift)) | (becomes << shift);
            tally_texel(sh, t, l, becomes, c.x, c.y, c.z);
        }
        c.next(bricked, nx, ny);
    }
}

// One record, chunk k with the 16 bytes `bytes`, appended to the journal: the lanes of a wave that arrive together take one atomicAdd
// for their number and rank themselves below it.  The callers' loops are divergent here, so the ballot is taken among the lanes that
// are there.  (The smoothing's vote, smooth_kernels.h, appends the bytes a chunk WILL hold by the same counter.)
__device__ __forceinline__ void journal_append(const LabelJournal& journal, uint64_t k, const uint4& bytes)
{
    const unsigned long long here = __ballot(1);                         // the lanes that store a chunk in this step
    const uint32_t lane = threadIdx.x & 63u, leader = static_cast<uint32_t>(__ffsll(here)) - 1u;
    uint32_t first = 0u;
    if (lane == leader) first = atomicAdd(journal.count, static_cast<uint32_t>(__popcll(here)));
    first = __shfl(first, static_cast<int>(leader), 64);
    const uint32_t at = first + static_cast<uint32_t>(__popcll(here & ((1ull << lane) - 1ull)));
    if (at < journal.capacity) { journal.index[at] = static_cast<uint32_t>(k); journal.old[at] = bytes; }
}

// Store chunk k, whose bytes were lv and are lb now, by a plain vector store.  JOURNAL: the chunk is appended to the journal first,
// once (its owner is the only lane that gets here), by journal_append.
template <bool JOURNAL>
__device__ __forceinline__ void chunk_store(uint4* __restrict__ labels, uint64_t k, const uint4& lv, const uint32_t lb[4], const LabelJournal& journal)
{
    if (JOURNAL) journal_append(journal, k, lv);
    labels[k] = make_uint4(lb[0], lb[1], lb[2], lb[3]);
}

// ---- the walk and the tail of the passes whose texels are selected by geometry (the brush, the lasso) -------------------------------
// Such a pass goes over its slab a wave at a time -- the loop's trip count is the wave's, because its cull talks across the lanes --
// and decides per chunk, geometry first: the 16-bit mask of the chunk's selected texels needs no memory.

// One step of that walk: the lane's chunk and the boxes the selection rules cull with.
struct WaveChunk {
    uint32_t k, keep;               // the lane's chunk (k < 2^28: a layout has fewer than 2^32 bytes) and the texels of it the slab keeps
                                    // (live: it has a chunk, owns it, and keeps some)
    bool live;
    uint32_t x0, y0, z0;            // the chunk's first texel
    uint32_t cl[3], ch[3];          // the chunk's texel box, hi INCLUSIVE (no chunk: lo > hi)
    uint32_t wl[3], wh[3];          // the box of the wave's 64 chunks, in scalar registers
};

// Item base + lane of slab s: crop_chunk and, linear, the one-owner test.  The chunk's box is a brick's 4 x 4 patch of one z; linear,
// 16 texels that may wrap rows and slices, whose box is then taken a little wide (whole rows, whole slices): it only culls.  False:
// no lane of the wave has a chunk (uniform).
__device__ __forceinline__ bool wave_chunk_step(WaveChunk& c, const CropSlab& s, uint32_t base, uint32_t lane, uint32_t n_items, uint32_t nx, uint32_t ny, uint64_t n,
                                                uint32_t bricked, uint32_t bx, uint32_t by)
{
    const uint32_t i = base + lane;
    uint64_t k = 0;
    uint32_t moved;
    c.keep = 0;
    c.live = i < n_items && crop_chunk<false>(s, i, nx, ny, n, bricked, bx, by, k, c.keep, moved);
    if (c.live && !bricked && !relabel_owns_chunk(s, i, nx, ny, k)) c.live = false;
    if (!c.keep) c.live = false;
    c.k = static_cast<uint32_t>(k);
    c.x0 = c.y0 = c.z0 = 0u;
    for (int a = 0; a < 3; ++a) { c.cl[a] = 0xffffffffu; c.ch[a] = 0u; }
    if (c.live) {
        label_chunk_origin(bricked != 0u, c.k, nx, ny, c.x0, c.y0, c.z0);
        c.cl[0] = c.x0; c.cl[1] = c.y0; c.cl[2] = c.ch[2] = c.z0;
        if (bricked) { c.ch[0] = c.x0 + 3u; c.ch[1] = c.y0 + 3u; }
        else if (c.x0 + 15u < nx) { c.ch[0] = c.x0 + 15u; c.ch[1] = c.y0; }
        else {
            const uint32_t rows = (c.x0 + 15u) / nx;
            c.cl[0] = 0u; c.ch[0] = nx - 1u; c.ch[1] = c.y0 + rows;
            if (c.ch[1] >= ny) { c.cl[1] = 0u; c.ch[1] = ny - 1u; c.ch[2] = c.z0 + (c.y0 + rows) / ny; }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c.wl[a] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_min(c.cl[a]))));
        c.wh[a] = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(wave_max(c.ch[a]))));
    }
    return c.wl[0] <= c.wh[0];
}

// The tail of a chunk whose mask is not 0: only now the 16 labels and to[l] != l; only if a candidate is left the density, skipped by
// a uniform test when the window is 0..255; then apply and tally, and the store of chunk_store unless DRY_RUN.  Every texel is decided
// once, by its chunk's owner, from the bytes before the edit.
template <bool JOURNAL>
__device__ __forceinline__ void selected_chunk_tail(RelabelShared& sh, RelabelTally& t, uint4* __restrict__ labels, const uint4* __restrict__ vol, uint64_t k,
                                                    uint32_t mask, bool windowed, uint32_t min_byte, uint32_t max_byte, uint32_t store, const LabelJournal& journal,
                                                    uint32_t nx, uint32_t ny, uint32_t bricked)
{
    const uint4 lv = labels[k];
    uint32_t lb[4] = {lv.x, lv.y, lv.z, lv.w};
    uint32_t cand = chunk_candidates(sh, lb, mask);
    if (!cand) return;                                                   // no density, no store
    if (windowed) {                                                      // (uniform)
        cand = chunk_in_window(vol[k], min_byte, max_byte, cand);
        if (!cand) return;
    }
    uint32_t x0, y0, z0;
    label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);
    chunk_apply(sh, t, lb, cand, bricked, x0, y0, z0, nx, ny);
    if (store) chunk_store<JOURNAL>(labels, k, lv, lb, journal);
}

}  // namespace volym
