// The label edit (volym_edit_labels, volym_relabel_check, volym_read_labels): included at the end of scene_bytes.hip, beside the
// kernels it launches (relabel_kernels.h) and the transition whose pieces it is built from (rewrite, ensure_uncropped_copies,
// refresh_macro_cells, scan_label_stats), and its history (volym_label_history, volym_undo_labels, volym_redo_labels,
// volym_label_history_info).  Blocking set-up calls like the other edits of that unit.  brush.inc and lasso.inc, included after this
// file, build their edits on what is here: editable_state, LabelEdit and edit_labels (the transition, with the kernel as a parameter),
// and the three things every launch site needs: edit_density, launch_edit and CallArray.
// smooth.inc, the edit in two phases, takes the pieces instead: editable_state, DeviceRelabelResult, edit_density, record_step, follow_labels.

#include <cstddef>

static_assert(sizeof(volym_relabel) == 308 && offsetof(volym_relabel, flags) == 24 && offsetof(volym_relabel, to) == 36 && offsetof(volym_relabel, id_lo) == 292 &&
              offsetof(volym_relabel, d2_lo) == 300, "volym_relabel has no padding");
static_assert(sizeof(volym_relabel_result) == 4128 && offsetof(volym_relabel_result, left) == 8 && offsetof(volym_relabel_result, arrived) == 2056 &&
              offsetof(volym_relabel_result, box) == 4104, "volym_relabel_result has no padding");
// (the info struct shares its name with the call that fills it: the tag is needed)
static_assert(sizeof(struct volym_label_history_info) == 56 && offsetof(struct volym_label_history_info, undo_steps) == 16 &&
              offsetof(struct volym_label_history_info, next_undo_records) == 24 && offsetof(struct volym_label_history_info, lost) == 48,
              "volym_label_history_info has no padding");

// What follows a change of labels under a (box, plane, mask) that stays -- an edit, an undo, a redo -- once the labels are stored and
// `res` names the labels that left and arrived and the hull of the changed texels (changed != 0).
// Precondition: density and importances held the invariant of context.hpp for the labels as they were.  Postcondition: they hold it
// for the labels as they are, label_count and label_box describe those, and everything derived from the bytes is up to date.
static int follow_labels(volym_ctx* c, const volym_relabel_result& res, const char* who)
{
    // counts and boxes first: mask_active and volym_visibility_boxes read them
    const hipError_t es = scan_label_stats(c);
    if (es != hipSuccess) return fail(c, VOLYM_E_HIP, std::string(who) + " (label statistics): " + hipGetErrorString(es));
    ++c->scene_serial;                                                    // labels changed: a surface pass is stale
    // A texel's bytes differ from the rule's only where its old and its new label differ in what they give: visibility for the
    // density, visibility and the table's byte for importances mapped from the labels.  Every such texel carries a label that
    // arrived, inside the result's box: the visibility kernel stores the chunks that hold one, whole, by the rule.
    uint8_t flipped[256];
    bool hidden_moved = false;
    for (int l = 0; l < 256; ++l) {
        flipped[l] = res.left[l] != 0u || res.arrived[l] != 0u;
        hidden_moved = hidden_moved || (flipped[l] && c->seg_hidden[l]);
    }
    int rc = VOLYM_OK;
    if (hidden_moved) rc = rewrite(c, density_of(c), res.box, flipped, nullptr);
    if (rc == VOLYM_OK && imp_croppable(c) && (imp_from_labels(c) || hidden_moved)) rc = rewrite(c, importances_of(c), res.box, flipped, nullptr);
    if (rc == VOLYM_OK && hidden_moved) rc = refresh_macro_cells(c, &res.box, 1u);
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->slot0().stream));                   // every slot's next frame reads the new bytes
    if (imp_from_labels(c)) segment_important_box(c);
    crop_important_box(c);
    return rebuild_lists(c);
}

// ---- the history of label edits (volym_label_history, volym_undo_labels, volym_redo_labels) ----------------------------------------
// A step is what one edit destroyed: the chunks it stored, with the bytes they held (relabel_kernels.h LabelJournal), in device
// memory of its own, sized by its records.  Undo and redo swap a step with the labels (volym_label_swap_kernel) and take the edit's
// follow-up.  scene.LabelHistory of the Python package is the twin of the bookkeeping below, equal in every field of the info.
static const uint64_t JOURNAL_RECORD_BYTES = 20u;          // a chunk index and 16 bytes

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
static void record_step(volym_ctx* c, const volym_relabel_result& res, uint64_t records, uint64_t capacity)
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

// the working result of an edit, an undo or a redo in device memory: the result, then the journal's counter
struct DeviceRelabelResult { volym_relabel_result result; uint32_t records, pad; };

// What the edit's transition needs to know of a request, whichever kernel carries it out (volym_edit_labels here, the brush of
// brush.inc): the box its kernel walks and keeps to, the table, DRY_RUN, and the name errors carry.
struct LabelEdit {
    const uint32_t* box;
    const uint8_t* to;
    bool dry;
    const char* who;
};

// The edit's own transition, the counterpart of retarget for a change of labels under a (box, plane, mask) that stays (follow_labels).
// launch(stream, grid, out, to, slab, items, journal) enqueues the request's kernel over the slab of r.box (keep = inside that box);
// journal is NULL unless the history is on and the request is no DRY_RUN.  With no texel changed (or DRY_RUN) nothing but the result is
// written.  A failure after the kernel has stored leaves bytes that belong to neither state: the context then asks for
// volym_set_volume again, as after a failed retarget.
template <class Launch>
static int edit_labels(volym_ctx* c, const LabelEdit& r, volym_relabel_result& res, Launch launch)
{
    const bool dry = r.dry;
    const bool journalled = c->history_budget != 0u && !dry;
    std::memset(&res, 0, sizeof res);
    for (int a = 0; a < 3; ++a) if (r.box[a] == r.box[3 + a]) return VOLYM_OK;        // an empty box: nothing to walk

    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    // A hidden label that has voxels has made the uncut copies already; one without voxels has not (retarget takes the idle path for
    // it), and texels are about to move into it.  The bytes are still uncut then: the precondition of ensure_uncropped_copies.
    bool hidden_target = false;
    for (int l = 0; l < 256; ++l) hidden_target = hidden_target || (r.to[l] != l && c->seg_hidden[r.to[l]]);
    if (hidden_target || mask_active(c)) {
        rc = ensure_uncropped_copies(c, true);                            // in stream order in front of the kernel and the rewrites
        if (rc != VOLYM_OK) return rc;
    }

    const hipStream_t stream = c->slot0().stream;
    CropSlab s;
    const uint64_t items = make_crop_slab(c, c->bricked, r.box, nullptr, s);
    // the staging area holds the slab's worst case, one record per item, or what the budget holds: past that the kernel only counts
    const uint64_t capacity = journalled ? std::min<uint64_t>(items, c->history_budget / JOURNAL_RECORD_BYTES) : 0u;
    if (journalled) {
        rc = c->journal_index.reserve(c, stream, capacity, "label journal");
        if (rc == VOLYM_OK) rc = c->journal_old.reserve(c, stream, capacity, "label journal");
        if (rc != VOLYM_OK) return rc;
    }
    DeviceRelabelResult init = {}, back = {};
    for (int a = 0; a < 3; ++a) init.result.box[a] = 0xffffffffu;         // lo = max, hi = 0: the kernel keeps INCLUSIVE maxima
    DeviceRelabelResult* d_res = nullptr;
    hipError_t e = hipMalloc(&d_res, sizeof init);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(relabel result): ") + hipGetErrorString(e));
    e = hipMemcpyAsync(d_res, &init, sizeof init, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        // keep = inside the request's box, whatever the crop box and the plane are: the cuts are in the bytes the window reads
        for (int a = 0; a < 3; ++a) { s.box_lo[a] = r.box[a]; s.box_hi[a] = r.box[3 + a]; }
        s.planes = 0u; s.pn[0] = s.pn[1] = s.pn[2] = s.pd = 0;
        LabelTable to;
        std::memcpy(to.v, r.to, 256);
        volym_relabel_result* const dr = &d_res->result;
        const RelabelOut out = {reinterpret_cast<unsigned long long*>(&dr->changed), reinterpret_cast<unsigned long long*>(dr->left),
                                reinterpret_cast<unsigned long long*>(dr->arrived), dr->box};
        const LabelJournal journal = {c->journal_index.ptr, c->journal_old.ptr, &d_res->records, static_cast<uint32_t>(capacity)};
        launch(stream, dim3(stream_grid(c, items)), out, to, s, static_cast<uint32_t>(items), journalled ? &journal : nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&back, d_res, sizeof back, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_res);
    if (e != hipSuccess) {
        if (!dry) c->have_vol = c->have_frame = false;                    // (the kernel may have stored)
        return fail(c, VOLYM_E_HIP, std::string(r.who) + ": " + hipGetErrorString(e));
    }
    res = back.result;
    if (res.changed == 0u) { std::memset(res.box, 0, sizeof res.box); return VOLYM_OK; }
    for (int a = 3; a < 6; ++a) ++res.box[a];                             // hi exclusive
    if (dry) return VOLYM_OK;

    if (journalled) record_step(c, res, back.records, capacity);
    rc = follow_labels(c, res, r.who);
    if (rc != VOLYM_OK) c->have_vol = c->have_frame = false;
    return rc;
}

// the density an edit's window reads: the uncut copy with UNCUT, where there is one (call it after ensure_uncropped_copies: inside launch)
static const uint4* edit_density(const volym_ctx* c, bool uncut) { return reinterpret_cast<const uint4*>(uncut && c->d_vol0 ? c->d_vol0 : c->d_vol); }

// What edit_labels' launch does with what it is handed, for a pair of kernels (plain, journalling) that differ in the journal argument
// alone: the labels first, then `front` (what the kernel reads beside them), the result, the table, the slab and the rule, the journal
// where there is one, and the volume's shape.
template <class Plain, class Journalling, class Rule, class... Front>
static void launch_edit(const volym_ctx* c, Plain plain, Journalling journalling, hipStream_t stream, dim3 grid, const RelabelOut& out, const LabelTable& to,
                        const CropSlab& s, const Rule& rule, uint32_t items, const LabelJournal* journal, Front... front)
{
    uint4* const labels = reinterpret_cast<uint4*>(c->d_labels);
    const uint32_t bricked = c->bricked ? 1u : 0u;
    if (journal) hipLaunchKernelGGL(journalling, grid, dim3(256), 0, stream, labels, front..., out, to, s, rule, *journal, c->nx, c->ny, c->nz, bricked, items);
    else hipLaunchKernelGGL(plain, grid, dim3(256), 0, stream, labels, front..., out, to, s, rule, c->nx, c->ny, c->nz, bricked, items);
}

// A small host array on the device for the length of one call (the brush's segments, the lasso's edges): copied on `stream`, in
// stream order in front of the call's kernels, and freed when the call returns, once the stream is idle (after a refusal the copy or a
// kernel may still run).
template <class T>
struct CallArray {
    T* ptr = nullptr;
    hipStream_t stream = nullptr;

    // VOLYM_E_NOMEM "hipMalloc(<what>): <hip error>", or VOLYM_E_HIP "<who>: <hip error>" for the copy
    int upload(volym_ctx* c, hipStream_t on, const std::vector<T>& host, const char* what, const char* who)
    {
        stream = on;
        hipError_t e = hipMalloc(&ptr, host.size() * sizeof(T));
        if (e != hipSuccess) { ptr = nullptr; return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e)); }
        e = hipMemcpyAsync(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? VOLYM_OK : fail(c, VOLYM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    CallArray() = default;
    CallArray(const CallArray&) = delete;
    ~CallArray() { if (ptr) { (void)hipStreamSynchronize(stream); (void)hipFree(ptr); } }
};

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
    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    const uint64_t* arrives = redo ? step.result.arrived : step.result.left;
    bool hidden_target = false;
    for (int l = 0; l < 256; ++l) hidden_target = hidden_target || (arrives[l] != 0u && c->seg_hidden[l]);
    if (hidden_target || mask_active(c)) {
        rc = ensure_uncropped_copies(c, true);
        if (rc != VOLYM_OK) return rc;
    }
    const hipStream_t stream = c->slot0().stream;
    volym_relabel_result init = {};
    for (int a = 0; a < 3; ++a) init.box[a] = 0xffffffffu;
    volym_relabel_result* d_res = nullptr;
    hipError_t e = hipMalloc(&d_res, sizeof init);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(relabel result): ") + hipGetErrorString(e));
    e = hipMemcpyAsync(d_res, &init, sizeof init, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const RelabelOut out = {reinterpret_cast<unsigned long long*>(&d_res->changed), reinterpret_cast<unsigned long long*>(d_res->left),
                                reinterpret_cast<unsigned long long*>(d_res->arrived), d_res->box};
        hipLaunchKernelGGL(volym_label_swap_kernel, dim3(stream_grid(c, step.records)), dim3(256), 0, stream, reinterpret_cast<uint4*>(c->d_labels), step.index,
                           step.old, out, c->nx, c->ny, c->bricked ? 1u : 0u, static_cast<uint32_t>(step.records));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_res);
    if (e != hipSuccess) {
        std::memset(&res, 0, sizeof res);
        c->have_vol = c->have_frame = false;                              // (the kernel may have stored)
        clear_label_history(c);
        return fail(c, VOLYM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    if (redo) ++c->history_cursor; else --c->history_cursor;
    if (res.changed == 0u) { std::memset(res.box, 0, sizeof res.box); return VOLYM_OK; }      // (a step holds a changed byte: not reached)
    for (int a = 3; a < 6; ++a) ++res.box[a];
    rc = follow_labels(c, res, who);
    if (rc != VOLYM_OK) c->have_vol = c->have_frame = false;
    return rc;
}

// what volym_edit_labels refuses of the context's state, in the name of `who`
static int editable_state(volym_ctx* c, const char* who)
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
