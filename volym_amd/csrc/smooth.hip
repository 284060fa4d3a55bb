// libvolym_hip.so: the smoothing (volym_smooth_labels, volym_smooth_check) beside the kernel it launches (smooth_kernels.h).  The
// first edit whose kernel cannot run in place, so it has a transition of its own, built from the pieces of label_edit.hpp.  Two phases:
// the vote leaves the chunks that change, as they will be, in the journal's staging area; volym_label_swap_kernel (launch_label_swap)
// exchanges them with the labels and leaves there what record_step expects.  A blocking set-up call.
#include <hip/hip_runtime.h>

#include <cassert>
#include <cstddef>

#include "label_edit.hpp"
#include "smooth_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_smooth) == 560 && offsetof(volym_smooth, flags) == 24 && offsetof(volym_smooth, min_byte) == 28 && offsetof(volym_smooth, radius) == 36 &&
              offsetof(volym_smooth, give) == 48 && offsetof(volym_smooth, take) == 304, "volym_smooth has no padding");
static_assert(VOLYM_SMOOTH_UNCUT == VOLYM_RELABEL_UNCUT && VOLYM_SMOOTH_DRY_RUN == VOLYM_RELABEL_DRY_RUN, "the smoothing's flags carry the edit's values");

// The staging area's optimistic share of the slab's items: a smoothing pass changes surfaces, not volumes, so one
// record per 16 items, and never fewer than 4096 records (80 KiB) nor more than the slab has items.
static const uint64_t SMOOTH_SHARE = 16u, SMOOTH_LEAST_RECORDS = 4096u;

// One launch of the vote over the slab, with room for `capacity` records, and its result and record count read back.
static hipError_t smooth_vote(volym_ctx* c, DeviceResult& d, const volym_smooth* r, const CropSlab& s, const SmoothRule& rule, uint64_t items, uint64_t capacity,
                              DeviceRelabelResult& back)
{
    hipError_t e = d.seed<DeviceRelabelResult>();
    if (e != hipSuccess) return e;
    const RelabelOut out = d.out();
    const LabelJournal journal = d.journal(c, capacity);
    SmoothTables tables;
    std::memcpy(tables.give, r->give, 256);
    std::memcpy(tables.take, r->take, 256);
    const uint32_t* labels = reinterpret_cast<const uint32_t*>(c->d_labels);
    const uint32_t* vol = reinterpret_cast<const uint32_t*>(edit_density(c, (r->flags & VOLYM_SMOOTH_UNCUT) != 0u));
    const uint32_t rows = (2u * r->radius[1] + 1u) * (2u * r->radius[2] + 1u), bricked = c->bricked ? 1u : 0u;
    // the tile follows the rows: up to 9 of them (radius <= 1 across the rows) or up to 49
    const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(rule.n_units, static_cast<uint64_t>(c->n_cus) * (rows <= 9u ? 8u : 2u))));
    if (rows <= 9u)
        hipLaunchKernelGGL(volym_smooth_vote_kernel<9u>, grid, dim3(256), 0, d.stream, labels, vol, out, tables, s, rule, journal, c->nx, c->ny, c->nz, bricked,
                           static_cast<uint32_t>(items));
    else
        hipLaunchKernelGGL(volym_smooth_vote_kernel<49u>, grid, dim3(256), 0, d.stream, labels, vol, out, tables, s, rule, journal, c->nx, c->ny, c->nz, bricked,
                           static_cast<uint32_t>(items));
    e = hipGetLastError();
    return e == hipSuccess ? d.fetch(back) : e;
}

// The smoothing's own transition, the counterpart of edit_labels for an edit in two phases.
static int smooth_labels(volym_ctx* c, const volym_smooth* r, volym_relabel_result& res)
{
    const char* const who = "volym_smooth_labels";
    const bool dry = (r->flags & VOLYM_SMOOTH_DRY_RUN) != 0u;
    const bool journalled = c->history_budget != 0u && !dry;
    std::memset(&res, 0, sizeof res);
    for (int a = 0; a < 3; ++a) if (r->box[a] == r->box[3 + a]) return VOLYM_OK;          // an empty box: nothing to walk

    // every label that gives or takes can be on either side
    uint8_t receives[256];
    for (int l = 0; l < 256; ++l) receives[l] = r->give[l] || r->take[l];
    int rc = begin_edit(c, receives);
    if (rc != VOLYM_OK) return rc;

    const hipStream_t stream = c->slot0().stream;
    CropSlab s;
    const uint64_t items = edit_slab(c, r->box, s);
    SmoothRule rule = {};
    rule.min_byte = r->min_byte; rule.max_byte = r->max_byte;
    rule.store = dry ? 0u : 1u;
    for (int a = 0; a < 3; ++a) rule.radius[a] = r->radius[a];
    uint64_t lines;
    if (c->bricked) { lines = static_cast<uint64_t>(s.b_n[1]) * s.b_n[2]; rule.blocks = (s.b_n[0] + SMOOTH_BRICKS - 1u) / SMOOTH_BRICKS; }
    else { lines = static_cast<uint64_t>(s.runs_y) * s.runs_z; rule.blocks = (s.chunks_per_run + SMOOTH_LINEAR_CHUNKS - 1u) / SMOOTH_LINEAR_CHUNKS; }
    rule.n_units = static_cast<uint32_t>(lines * rule.blocks);           // (no more than the slab has items: < 2^32)
    rule.alloc_dwords = static_cast<uint32_t>((static_cast<uint64_t>(c->nx) * c->ny * c->nz + 15u) / 16u * 4u);

    // the staging area: the optimistic share; the vote only counts past it, and is launched once more with room for what it counted
    uint64_t capacity = dry ? 0u : std::min(items, std::max(SMOOTH_LEAST_RECORDS, items / SMOOTH_SHARE));
    if (!dry) rc = reserve_journal(c, stream, capacity);
    if (rc != VOLYM_OK) return rc;
    DeviceRelabelResult back = {}, applied = {};
    bool apply = false;
    {
        DeviceResult d;
        rc = d.alloc(c, stream);
        if (rc != VOLYM_OK) return rc;
        hipError_t e = smooth_vote(c, d, r, s, rule, items, capacity, back);
        if (e == hipSuccess && !dry && back.records > capacity) {        // no label is written yet: the second launch sees the same bytes
            capacity = back.records;
            rc = reserve_journal(c, stream, capacity);
            if (rc != VOLYM_OK) return rc;
            e = smooth_vote(c, d, r, s, rule, items, capacity, back);
        }
        apply = e == hipSuccess && !dry && back.result.changed != 0u;
        if (apply) {
            // phase two: the records and the labels change places; the staging area then holds the bytes before the edit
            e = d.seed<DeviceRelabelResult>();
            if (e == hipSuccess) e = launch_label_swap(c, stream, c->journal_index.ptr, c->journal_old.ptr, back.records, d.out());
            if (e == hipSuccess) e = d.fetch(applied);
        }
        if (e != hipSuccess) {
            if (apply) c->have_vol = c->have_frame = false;               // (the swap may have stored)
            return fail(c, VOLYM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
        }
    }
    res = back.result;
#if VOLYM_DEV_SWITCHES
    // the swap's own tally is the vote's (hulls still INCLUSIVE in both)
    if (apply) assert(std::memcmp(&applied.result, &back.result, sizeof back.result) == 0);
#endif
    // one step of the history by the rule every edit has; with the history off the staging area stays, as the journal's does, until
    // volym_label_history(0) or volym_destroy
    return finish_edit(c, res, dry, journalled, back.records, std::min<uint64_t>(items, c->history_budget / JOURNAL_RECORD_BYTES), who);
}

extern "C" {

int volym_smooth_check(const volym_smooth* r, const uint32_t dims[3])
{
    if (!r || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(r->box, dims)) return VOLYM_E_INVALID;
    if (r->flags & ~static_cast<uint32_t>(VOLYM_SMOOTH_UNCUT | VOLYM_SMOOTH_DRY_RUN)) return VOLYM_E_INVALID;
    if (r->min_byte > r->max_byte || r->max_byte > 255u) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a) if (r->radius[a] > VOLYM_SMOOTH_MAX_RADIUS) return VOLYM_E_INVALID;
    if (r->radius[0] == 0u && r->radius[1] == 0u && r->radius[2] == 0u) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_smooth_labels(volym_ctx* c, const volym_smooth* r, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!r) return fail(c, VOLYM_E_INVALID, "volym_smooth_labels: NULL request");
    const int ok = editable_state(c, "volym_smooth_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_smooth_check(r, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_smooth_labels: need lo <= hi <= volume size on every axis, known flags, min_byte <= max_byte <= 255 and radii in 0..3, "
                                        "not all 0");
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = smooth_labels(c, r, res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

}  // extern "C"
