// The kernels of the label edit (volym_edit_labels, volym_read_labels) and of its history (volym_label_history: the journalling form
// of the edit, and the swap of volym_undo_labels and volym_redo_labels, which is also the second phase of the smoothing).  Included by
// relabel.hip alone (volym_label_swap_kernel and volym_read_labels_kernel are no templates).  The parts of an edit pass are
// edit_chunks.h's; here the pass that selects by table, window, piece and distance.
#pragma once

#include "edit_chunks.h"

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

// ---- the edit by table, window, piece and distance ------------------------------------------------------------------------------------
// One pass over the items of slab s (make_crop_slab over the request's box, s.box_lo/hi the box itself, no plane: keep names the
// texels of the box), in either layout, a lane at a time: the trip count is the item's, and a lane goes on before any load.  Per
// chunk: the 16 labels first; a chunk in which no texel of the box has to[l] != l loads nothing more and stores nothing.  Else the 16
// density bytes (vol: the scene bytes, or the uncut copy), then -- IDS, DISTANCE -- the id and the distance of the texels that are
// still candidates, from the box-linear snapshots.  The chunk is stored only if a byte changed and rule.store says so.  Labels are
// read and written by the chunk's one owner and everything else is only read: every texel is decided from the bytes before the edit.
//
// The result: tally_texel per changed texel, tally_reduce at the end.
template <bool IDS, bool DISTANCE, bool JOURNAL>
__device__ __forceinline__ void relabel_pass(RelabelShared& sh, uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ ids,
                                             const uint32_t* __restrict__ dmap, const RelabelOut& out, const LabelTable& to, const CropSlab& s,
                                             const RelabelRule& rule, const LabelJournal& journal, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked,
                                             uint32_t n_items)
{
    edit_prologue(sh, to);
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
        if (!cand) continue;                                             // no density, no ids, no store
        cand = chunk_in_window(vol[k], rule.min_byte, rule.max_byte, cand);
        if (!cand) continue;
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, static_cast<uint32_t>(k), nx, ny, x0, y0, z0);      // (k < 2^28: a layout has fewer than 2^32 bytes)
        if (IDS || DISTANCE) {                                           // the snapshots, between window and apply
            ChunkCursor c = {x0, y0, z0};
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                c.at(bricked, j, x0, y0);
                if (cand & (1u << j)) {
                    bool in = true;
                    if (IDS) {
                        const uint32_t id = ids[box_linear(rule.ids_box, c.x, c.y, c.z)];
                        const bool ranged = id >= rule.id_lo && id <= rule.id_hi;
                        in = id != VOLYM_COMPONENT_NONE && (rule.ids_except ? !ranged : ranged);
                    }
                    if (DISTANCE && in) {
                        const uint32_t dd = dmap[box_linear(rule.map_box, c.x, c.y, c.z)];
                        in = dd != VOLYM_DISTANCE_NONE && dd >= rule.d2_lo && dd <= rule.d2_hi;
                    }
                    if (!in) cand &= ~(1u << j);
                }
                c.next(bricked, nx, ny);
            }
            if (!cand) continue;
        }
        chunk_apply(sh, t, lb, cand, bricked, x0, y0, z0, nx, ny);
        if (rule.store) chunk_store<JOURNAL>(labels, k, lv, lb, journal);
    }
    tally_reduce(sh, t, out);
}

template <bool IDS, bool DISTANCE>
__global__ __launch_bounds__(256) void volym_relabel_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ ids,
                                                            const uint32_t* __restrict__ dmap, RelabelOut out, LabelTable to, CropSlab s, RelabelRule rule,
                                                            uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    relabel_pass<IDS, DISTANCE, false>(sh, labels, vol, ids, dmap, out, to, s, rule, LabelJournal{}, nx, ny, nz, bricked, n_items);
}

// the same edit while the history is on and the request is no DRY_RUN
template <bool IDS, bool DISTANCE>
__global__ __launch_bounds__(256) void volym_relabel_journal_kernel(uint4* __restrict__ labels, const uint4* __restrict__ vol, const uint32_t* __restrict__ ids,
                                                                    const uint32_t* __restrict__ dmap, RelabelOut out, LabelTable to, CropSlab s, RelabelRule rule,
                                                                    LabelJournal journal, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t bricked, uint32_t n_items)
{
    __shared__ RelabelShared sh;
    relabel_pass<IDS, DISTANCE, true>(sh, labels, vol, ids, dmap, out, to, s, rule, journal, nx, ny, nz, bricked, n_items);
}

// Undo and redo (volym_undo_labels, volym_redo_labels): swap the records of one journal step with the labels, one record per lane and
// step of the grid.  Chunk index[i] gets the bytes old[i] and old[i] the bytes the chunk held, so that the same launch takes the swap
// back.  The chunks of a step are distinct: no two lanes touch the same one.  For the bytes that differ (texels of the volume: an edit
// changes no padding) the lane tallies the label that is there now as left and the one it restores as arrived, and their hull, with
// coordinates stepped by the edit's ChunkCursor: a linear chunk wraps rows and slices.
__global__ __launch_bounds__(256) void volym_label_swap_kernel(uint4* __restrict__ labels, const uint32_t* __restrict__ index, uint4* __restrict__ old,
                                                               RelabelOut out, uint32_t nx, uint32_t ny, uint32_t bricked, uint32_t n_records)
{
    __shared__ RelabelShared sh;
    tally_init(sh);
    __syncthreads();
    RelabelTally t;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_records; i += gridDim.x * 256u) {
        const uint32_t k = index[i];
        const uint4 now = labels[k], rec = old[i];
        labels[k] = rec;
        old[i] = now;
        const uint32_t a[4] = {now.x, now.y, now.z, now.w}, b[4] = {rec.x, rec.y, rec.z, rec.w};
        uint32_t x0, y0, z0;
        label_chunk_origin(bricked != 0u, k, nx, ny, x0, y0, z0);
        ChunkCursor c = {x0, y0, z0};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            c.at(bricked, j, x0, y0);
            const uint32_t shift = 8u * (j & 3u), from = (a[j >> 2] >> shift) & 0xffu, to = (b[j >> 2] >> shift) & 0xffu;
            if (from != to) tally_texel(sh, t, from, to, c.x, c.y, c.z);
            c.next(bricked, nx, ny);
        }
    }
    tally_reduce(sh, t, out);
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
