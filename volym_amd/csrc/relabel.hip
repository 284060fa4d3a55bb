// libvolym_hip.so: the label edit (volym_edit_labels, volym_relabel_check, volym_read_labels) beside the kernels it launches
// (relabel_kernels.h), its history (volym_label_history, volym_undo_labels, volym_redo_labels, volym_label_history_info), and the
// pieces of the edit's transition that label_edit.hpp declares for this unit, brush.hip, lasso.hip and smooth.hip.  Blocking set-up
// calls, like the other edits of the scene's bytes.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "label_edit.hpp"
#include "relabel_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_relabel) == 308 && offsetof(volym_relabel, flags) == 24 && offsetof(volym_relabel, to) == 36 && offsetof(volym_relabel, id_lo) == 292 &&
              offsetof(volym_relabel, d2_lo) == 300, "volym_relabel has no padding");
static_assert(sizeof(volym_relabel_result) == 4128 && offsetof(volym_relabel_result, left) == 8 && offsetof(volym_relabel_result, arrived) == 2056 &&
              offsetof(volym_relabel_result, box) == 4104, "volym_relabel_result has no padding");
// (the info struct shares its name with the call that fills it: the tag is needed)
static_assert(sizeof(struct volym_label_history_info) == 56 && offsetof(struct volym_label_history_info, undo_steps) == 16 &&
              offsetof(struct volym_label_history_info, next_undo_records) == 24 && offsetof(struct volym_label_history_info, lost) == 48,
              "volym_label_history_info has no padding");

// ---- the history of label edits (volym_label_history, volym_undo_labels, volym_redo_labels) ----------------------------------------
// A step is what one edit destroyed: the chunks it stored, with the bytes they held (edit_chunks.h LabelJournal), in device
// memory of its own, sized by its records.  Undo and redo swap a step with the labels (volym_label_swap_kernel) and take the edit's
// follow-up.  scene.LabelHistory of the Python package is the twin of the bookkeeping below, equal in every field of the info.

static void free_step(volym_ctx::LabelStep& s) { (void)hipFree(s.index); (void)hipFree(s.old); s = volym_ctx::LabelStep{}; }

// steps [first, last) go; the cursor follows
static void drop_steps(volym_ctx* c, size_t first, size_t last)
{
    for (size_t i = first; i < last; ++i) { c->history_used -= JOURNAL_RECORD_BYTES * c->history_steps[i].records; free_step(c->history_steps[i]); }
    c->history_steps.erase(c->history_steps.begin() + static_cast<std::ptrdiff_t>(first), c->history_steps.begin() + static_cast<std::ptrdiff_t>(last));
    if (c->history_cursor > last) c->history_cursor -= last - first;
    else if (c->history_cursor > first) c->history_cursor = first;
}

// Back inside the budget: the oldest undoable steps go first; when none is left, the redo steps that would be redone last (a gap
// in front of a step would make it wrong).  Each counts as dropped.
static void fit_history(volym_ctx* c)
{
    while (c->history_used > c->history_budget && !c->history_steps.empty()) {
        if (c->history_cursor > 0u) drop_steps(c, 0u, 1u);
        else drop_steps(c, c->history_steps.size() - 1u, c->history_steps.size());
        ++c->history_dropped;
    }
}

namespace volym {

void clear_label_history(volym_ctx* c)
{
    if (c->history_steps.empty()) return;
    (void)hipSetDevice(c->device);
    drop_steps(c, 0u, c->history_steps.size());
}

void free_label_history(volym_ctx* c)
{
    clear_label_history(c);
    c->journal_index.release();
    c->journal_old.release();
    c->history_budget = c->history_dropped = c->history_lost = 0u;
}

}  // namespace volym

// The journal of the edit that has just stored (records > 0 of them counted, the first min(records, capacity) in the staging area)
// becomes the newest step, in memory of its own, and every redo step goes.  A journal that ran past its capacity, or one there is no
// memory for, has a gap: undoing older steps across it would be wrong, so the whole history is given up and `lost` counts it.
void volym::record_step(volym_ctx* c, const volym_relabel_result& res, uint64_t records, uint64_t capacity)
{
    drop_steps(c, c->history_cursor, c->history_steps.size());
    volym_ctx::LabelStep step;
    bool kept = records <= capacity;
    if (kept) {
        const hipStream_t stream = c->slot0().stream;
        hipError_t e = hipMalloc(&step.index, records * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&step.old, records * sizeof(uint4));
        if (e == hipSuccess) e = hipMemcpyAsync(step.index, c->journal_index.ptr, records * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(step.old, c->journal_old.ptr, records * sizeof(uint4), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipGetLastError(); free_step(step); kept = false; }
    }
    if (!kept) {
        drop_steps(c, 0u, c->history_steps.size());
        ++c->history_lost;
        return;
    }
    step.records = records;
    step.result = res;
    c->history_steps.push_back(step);
    c->history_cursor = c->history_steps.size();
    c->history_used += JOURNAL_RECORD_BYTES * records;
    fit_history(c);
}

// ---- the pieces of an edit's transition (label_edit.hpp) -------------------------------------------------------------------------------

int volym::begin_edit(volym_ctx* c, const uint8_t receives[256])
{
    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    bool hidden_target = false;
    for (int l = 0; l < 256; ++l) hidden_target = hidden_target || (receives[l] && c->seg_hidden[l]);
    if (hidden_target || mask_active(c)) rc = ensure_uncropped_copies(c, true);
    return rc;
}

uint64_t volym::edit_slab(const volym_ctx* c, const uint32_t box[6], CropSlab& s)
{
    const uint64_t items = make_crop_slab(c, c->bricked, box, nullptr, s);
    for (int a = 0; a < 3; ++a) { s.box_lo[a] = box[a]; s.box_hi[a] = box[3 + a]; }
    s.planes = 0u; s.pn[0] = s.pn[1] = s.pn[2] = s.pd = 0;
    return items;
}

int volym::reserve_journal(volym_ctx* c, hipStream_t stream, uint64_t capacity)
{
    const int rc = c->journal_index.reserve(c, stream, capacity, "label journal");
    return rc == VOLYM_OK ? c->journal_old.reserve(c, stream, capacity, "label journal") : rc;
}

hipError_t volym::launch_label_swap(const volym_ctx* c, hipStream_t stream, const uint32_t* index, uint4* old, uint64_t records, const RelabelOut& out)
{
    hipLaunchKernelGGL(volym_label_swap_kernel, dim3(stream_grid(c, records)), dim3(256), 0, stream, reinterpret_cast<uint4*>(c->d_labels), index, old, out, c->nx,
                       c->ny, c->bricked ? 1u : 0u, static_cast<uint32_t>(records));
    return hipGetLastError();
}

int volym::finish_edit(volym_ctx* c, volym_relabel_result& res, bool dry, bool journalled, uint64_t records, uint64_t capacity, const char* who)
{
    if (res.changed == 0u) { std::memset(res.box, 0, sizeof res.box); return VOLYM_OK; }
    for (int a = 3; a < 6; ++a) ++res.box[a];                             // hi exclusive
    if (dry) return VOLYM_OK;
    if (journalled) record_step(c, res, records, capacity);
    const int rc = follow_labels(c, res, who);
    if (rc != VOLYM_OK) c->have_vol = c->have_frame = false;
    return rc;
}

// volym_edit_labels' request as an edit: the relabel kernel of its flags, plain or journalling
static int relabel_labels(volym_ctx* c, const volym_relabel* r, volym_relabel_result& res)
{
    const bool with_ids = (r->flags & VOLYM_RELABEL_IDS) != 0u, with_map = (r->flags & VOLYM_RELABEL_DISTANCE) != 0u;
    const bool uncut_bytes = (r->flags & VOLYM_RELABEL_UNCUT) != 0u, dry = (r->flags & VOLYM_RELABEL_DRY_RUN) != 0u;
    RelabelRule rule = {};
    rule.min_byte = r->min_byte; rule.max_byte = r->max_byte;
    rule.id_lo = r->id_lo; rule.id_hi = r->id_hi; rule.ids_except = (r->flags & VOLYM_RELABEL_IDS_EXCEPT) ? 1u : 0u;
    rule.d2_lo = r->d2_lo; rule.d2_hi = r->d2_hi;
    rule.store = dry ? 0u : 1u;
    std::memcpy(rule.ids_box, c->component_box, sizeof rule.ids_box);
    std::memcpy(rule.map_box, c->distance_box, sizeof rule.map_box);
    const uint32_t* ids = with_ids ? c->component_ids.ptr : nullptr;
    const uint32_t* dmap = with_map ? c->distance_map.ptr : nullptr;
    const LabelEdit edit = {r->box, r->to, dry, "volym_edit_labels"};
    return edit_labels(c, edit, res, [&](hipStream_t stream, dim3 grid, const RelabelOut& out, const LabelTable& to, const CropSlab& s, uint32_t items,
                                         const LabelJournal* journal) {
        const auto plain = with_ids ? (with_map ? volym_relabel_kernel<true, true> : volym_relabel_kernel<true, false>)
                                    : (with_map ? volym_relabel_kernel<false, true> : volym_relabel_kernel<false, false>);
        const auto journalling = with_ids ? (with_map ? volym_relabel_journal_kernel<true, true> : volym_relabel_journal_kernel<true, false>)
                                          : (with_map ? volym_relabel_journal_kernel<false, true> : volym_relabel_journal_kernel<false, false>);
        launch_edit(c, plain, journalling, stream, grid, out, to, s, rule, items, journal, edit_density(c, uncut_bytes), ids, dmap);
    });
}

// Undo (redo false) or redo: the step next to the cursor is swapped with the labels, the device counts what the swap changed, and the
// edit's follow-up runs on that result.  The labels that receive texels are the step's saved `left` (undo) or `arrived` (redo): one of
// them may be hidden now and have had no voxels, which needs the uncut copies as an edit into such a label does.
static int swap_step(volym_ctx* c, bool redo, volym_relabel_result& res, const char* who)
{
    volym_ctx::LabelStep& step = c->history_steps[redo ? c->history_cursor : c->history_cursor - 1u];
    std::memset(&res, 0, sizeof res);
    const uint64_t* arrives = redo ? step.result.arrived : step.result.left;
    uint8_t receives[256];
    for (int l = 0; l < 256; ++l) receives[l] = arrives[l] != 0u;
    int rc = begin_edit(c, receives);
    if (rc != VOLYM_OK) return rc;
    {
        DeviceResult d;
        rc = d.alloc(c, c->slot0().stream);
        if (rc != VOLYM_OK) return rc;
        hipError_t e = d.seed<volym_relabel_result>();
        if (e == hipSuccess) e = launch_label_swap(c, d.stream, step.index, step.old, step.records, d.out());
        if (e == hipSuccess) e = d.fetch(res);
        if (e != hipSuccess) {
            std::memset(&res, 0, sizeof res);
            c->have_vol = c->have_frame = false;                          // (the kernel may have stored)
            clear_label_history(c);
            return fail(c, VOLYM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
        }
    }
    if (redo) ++c->history_cursor; else --c->history_cursor;
    return finish_edit(c, res, false, false, 0u, 0u, who);                // (a step holds a changed byte: changed != 0)
}

// what volym_edit_labels refuses of the context's state, in the name of `who`
int volym::editable_state(volym_ctx* c, const char* who)
{
    const std::string w(who);
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, w + ": no volume (volym_set_volume first)");
    if (!labels_fit(c)) return fail(c, VOLYM_E_STATE, w + ": no labels of the volume's dimensions (volym_set_labels first; volym_set_importances drops them)");
    if (c->labels_bricked != c->bricked || (imp_croppable(c) && c->imp_bricked != c->labels_bricked))
        return fail(c, VOLYM_E_STATE, w + ": volume, importances and labels were uploaded under different VOLYM_OPT_VOLUME_LAYOUT settings");
    return VOLYM_OK;
}

static int undo_or_redo(volym_ctx* c, bool redo, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    const char* who = redo ? "volym_redo_labels" : "volym_undo_labels";
    if (c->history_budget == 0u) return fail(c, VOLYM_E_STATE, std::string(who) + ": the history is off (volym_label_history first)");
    if (redo ? c->history_cursor == c->history_steps.size() : c->history_cursor == 0u)
        return fail(c, VOLYM_E_STATE, std::string(who) + (redo ? ": nothing to redo" : ": nothing to undo"));
    const int ok = editable_state(c, who);
    if (ok != VOLYM_OK) return ok;
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = swap_step(c, redo, res, who);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

extern "C" {

int volym_relabel_check(const volym_relabel* r, const uint32_t dims[3])
{
    if (!r || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(r->box, dims)) return VOLYM_E_INVALID;
    const uint32_t known = VOLYM_RELABEL_UNCUT | VOLYM_RELABEL_IDS | VOLYM_RELABEL_IDS_EXCEPT | VOLYM_RELABEL_DISTANCE | VOLYM_RELABEL_DRY_RUN;
    if (r->flags & ~known) return VOLYM_E_INVALID;
    if ((r->flags & VOLYM_RELABEL_IDS_EXCEPT) && !(r->flags & VOLYM_RELABEL_IDS)) return VOLYM_E_INVALID;
    if (r->min_byte > r->max_byte || r->max_byte > 255u) return VOLYM_E_INVALID;
    if ((r->flags & VOLYM_RELABEL_IDS) && r->id_lo > r->id_hi) return VOLYM_E_INVALID;
    if ((r->flags & VOLYM_RELABEL_DISTANCE) && r->d2_lo > r->d2_hi) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_edit_labels(volym_ctx* c, const volym_relabel* r, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!r) return fail(c, VOLYM_E_INVALID, "volym_edit_labels: NULL request");
    const int ok = editable_state(c, "volym_edit_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_relabel_check(r, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_edit_labels: need lo <= hi <= volume size on every axis, known flags, IDS_EXCEPT only with IDS, min_byte <= max_byte <= 255, "
                                        "id_lo <= id_hi with IDS and d2_lo <= d2_hi with DISTANCE");
    const auto inside = [&](const uint32_t box[6]) {
        for (int a = 0; a < 3; ++a) if (r->box[a] < box[a] || r->box[3 + a] > box[3 + a]) return false;
        return true;
    };
    if (r->flags & VOLYM_RELABEL_IDS) {
        if (c->components.count == 0u) return fail(c, VOLYM_E_STATE, "volym_edit_labels: IDS without a volym_components_pass since the volume was set");
        if (!inside(c->component_box)) return fail(c, VOLYM_E_INVALID, "volym_edit_labels: IDS with a box that reaches outside the box of the components pass");
    }
    if (r->flags & VOLYM_RELABEL_DISTANCE) {
        if (c->distance.count == 0u) return fail(c, VOLYM_E_STATE, "volym_edit_labels: DISTANCE without a volym_distance_pass since the volume was set");
        if (!inside(c->distance_box)) return fail(c, VOLYM_E_INVALID, "volym_edit_labels: DISTANCE with a box that reaches outside the box of the distance pass");
    }
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = relabel_labels(c, r, res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

int volym_label_history(volym_ctx* c, uint64_t budget_bytes)
{
    if (!c) return VOLYM_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (budget_bytes == 0u) {
        if (c->history_budget != 0u) {
            const int rc = quiesce_slots(c);                              // (every stream idle: the staging area goes too)
            if (rc != VOLYM_OK) return rc;
        }
        free_label_history(c);
        return VOLYM_OK;
    }
    if (c->history_budget == 0u) c->history_dropped = c->history_lost = 0u;
    c->history_budget = budget_bytes;
    fit_history(c);
    return VOLYM_OK;
}

int volym_undo_labels(volym_ctx* c, struct volym_relabel_result* out) { return undo_or_redo(c, false, out); }

int volym_redo_labels(volym_ctx* c, struct volym_relabel_result* out) { return undo_or_redo(c, true, out); }

int volym_label_history_info(volym_ctx* c, struct volym_label_history_info* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_label_history_info: NULL output");
    std::memset(out, 0, sizeof *out);
    out->budget_bytes = c->history_budget;
    out->used_bytes = c->history_used;
    out->undo_steps = static_cast<uint32_t>(c->history_cursor);
    out->redo_steps = static_cast<uint32_t>(c->history_steps.size() - c->history_cursor);
    if (out->undo_steps) out->next_undo_records = c->history_steps[c->history_cursor - 1u].records;
    if (out->redo_steps) out->next_redo_records = c->history_steps[c->history_cursor].records;
    out->dropped_steps = c->history_dropped;
    out->lost = c->history_lost;
    return VOLYM_OK;
}

int volym_read_labels(volym_ctx* c, const uint32_t sub[6], uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->d_labels) return fail(c, VOLYM_E_STATE, "volym_read_labels: no labels (volym_set_labels first; volym_set_importances drops them)");
    const uint32_t dims[3] = {c->lnx, c->lny, c->lnz};
    uint32_t whole[6];
    whole_volume_box(dims, whole);
    if (!sub) sub = whole;
    if (!box_in_volume(sub, dims)) return fail(c, VOLYM_E_INVALID, "volym_read_labels: the sub-box must have lo <= hi <= the labels' dimensions on every axis");
    const uint32_t w = sub[3] - sub[0], h = sub[4] - sub[1];
    const uint64_t total = static_cast<uint64_t>(w) * h * (sub[5] - sub[2]);
    if (total == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_labels: NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    uint8_t* d_out = nullptr;
    hipError_t e = hipMalloc(&d_out, total);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(label read-back): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(volym_read_labels_kernel, dim3(static_cast<uint32_t>((total + 255u) / 256u)), dim3(256), 0, stream, c->d_labels, d_out, c->lnx, c->lny,
                       c->labels_bricked ? 1u : 0u, sub[0], sub[1], sub[2], w, h, total);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, VOLYM_E_HIP, std::string("volym_read_labels: ") + hipGetErrorString(e));
    return VOLYM_OK;
}

}  // extern "C"
