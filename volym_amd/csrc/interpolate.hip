// libvolym_hip.so: the interpolate pass -- fill between slices -- (volym_interpolate_pass, volym_interpolate_check, the reads,
// volym_interpolate_at and the three device pointers) and the edit by it (volym_interpolate_labels, volym_interpolate_labels_check),
// beside the kernels they launch (interpolate_kernels.h).  The pass is a read-only pass like the distance pass: enqueue-only on slot 0's
// stream but for the allocations, its results a snapshot that later edits of the scene leave valid.  The edit is an edit like the
// others and goes through label_edit.hpp's transition.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "label_edit.hpp"
#include "interpolate_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_interpolate) == 820 && offsetof(volym_interpolate, flags) == 24 && offsetof(volym_interpolate, min_byte) == 28 &&
              offsetof(volym_interpolate, select) == 32 && offsetof(volym_interpolate, weight) == 288 && offsetof(volym_interpolate, axis) == 300 &&
              offsetof(volym_interpolate, max_gap) == 304 && offsetof(volym_interpolate, keys) == 308, "volym_interpolate has no padding");
static_assert(sizeof(volym_interpolate_summary) == 4u * INTERPOLATE_SUMMARY_WORDS && offsetof(volym_interpolate_summary, n_keys) == 4u * IS_N_KEYS &&
              offsetof(volym_interpolate_summary, n_gaps) == 4u * IS_N_GAPS && offsetof(volym_interpolate_summary, n_gap_slices) == 4u * IS_N_GAP_SLICES &&
              offsetof(volym_interpolate_summary, n_refused) == 4u * IS_N_REFUSED && offsetof(volym_interpolate_summary, n_shape) == 4u * IS_N_SHAPE &&
              offsetof(volym_interpolate_summary, n_inside) == 4u * IS_N_INSIDE && offsetof(volym_interpolate_summary, n_new) == 4u * IS_N_NEW &&
              offsetof(volym_interpolate_summary, n_stale) == 4u * IS_N_STALE && offsetof(volym_interpolate_summary, slice) == 4u * IS_SLICE,
              "volym_interpolate_summary is the 16398 words the kernels index");
static_assert(offsetof(volym_interpolate_slice, kind) == 4u * ISL_KIND && offsetof(volym_interpolate_slice, key_lo) == 4u * ISL_KEY_LO &&
              offsetof(volym_interpolate_slice, key_hi) == 4u * ISL_KEY_HI && offsetof(volym_interpolate_slice, count) == 4u * ISL_COUNT,
              "volym_interpolate_slice is the four words the kernels index");
static_assert(sizeof(volym_interpolate_edit) == 548 && offsetof(volym_interpolate_edit, flags) == 24 && offsetof(volym_interpolate_edit, min_byte) == 28 &&
              offsetof(volym_interpolate_edit, to) == 36 && offsetof(volym_interpolate_edit, out) == 292, "volym_interpolate_edit has no padding");
static_assert(VOLYM_INTERPOLATE_EDIT_UNCUT == VOLYM_RELABEL_UNCUT, "edit_density reads the flag of either");

void volym::free_interpolate(volym_ctx* c)
{
    c->interpolate.release();
    c->interpolate_work.release();
    c->interpolate_state.release();
    c->interpolate_counts.release();
    c->interpolate_texels = 0u;
}

static bool have_pass(const volym_ctx* c) { return c->interpolate.count != 0u; }
// the signed map of the latest pass: over the first stack of its column sweeps
static uint32_t* signed_map(const volym_ctx* c) { return c->interpolate_work.ptr ? c->interpolate_work.ptr + 2u * static_cast<size_t>(c->interpolate_texels) : nullptr; }

// volym_interpolate_labels' request as an edit: the table only marks the labels either table moves, the receiving labels come from both
static int interpolate_labels(volym_ctx* c, const volym_interpolate_edit* e, volym_relabel_result& res)
{
    const bool dry = (e->flags & VOLYM_INTERPOLATE_EDIT_DRY_RUN) != 0u, uncut_bytes = (e->flags & VOLYM_INTERPOLATE_EDIT_UNCUT) != 0u;
    InterpolateRule rule = {};
    rule.min_byte = e->min_byte; rule.max_byte = e->max_byte;
    rule.store = dry ? 0u : 1u;
    std::memcpy(rule.box, c->interpolate_box, sizeof rule.box);
    std::memcpy(rule.to, e->to, 256);
    std::memcpy(rule.out, e->out, 256);
    uint8_t marks[256], receives[256] = {};
    for (int l = 0; l < 256; ++l) {
        marks[l] = static_cast<uint8_t>((e->to[l] != l || e->out[l] != l) ? l ^ 1 : l);
        if (e->to[l] != l) receives[e->to[l]] = 1u;
        if (e->out[l] != l) receives[e->out[l]] = 1u;
    }
    const uint8_t* state = c->interpolate_state.ptr;
    const LabelEdit edit = {e->box, marks, dry, "volym_interpolate_labels", receives};
    return edit_labels(c, edit, res, [&](hipStream_t stream, dim3 grid, const RelabelOut& out, const LabelTable& to, const CropSlab& s, uint32_t items,
                                         const LabelJournal* journal) {
        launch_edit(c, volym_interpolate_edit_kernel, volym_interpolate_edit_journal_kernel, stream, grid, out, to, s, rule, items, journal,
                    edit_density(c, uncut_bytes), state);
    });
}

extern "C" {

int volym_interpolate_check(const volym_interpolate* q, const uint32_t dims[3])
{
    if (!q || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(q->box, dims)) return VOLYM_E_INVALID;
    if (q->flags & ~static_cast<uint32_t>(VOLYM_INTERPOLATE_UNCUT | VOLYM_INTERPOLATE_KEYS)) return VOLYM_E_INVALID;
    if (q->min_byte > 255u) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a)
        if (q->weight[a] == 0u || q->weight[a] > VOLYM_DISTANCE_WEIGHT_MAX) return VOLYM_E_INVALID;
    if (q->axis > 2u) return VOLYM_E_INVALID;
    if (!box_at_most(q->box, VOLYM_DISTANCE_BOX_MAX)) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a)
        if (q->box[3 + a] - q->box[a] > VOLYM_INTERPOLATE_SLICES) return VOLYM_E_INVALID;      // (a volume has at most 4096 texels per axis)
    return VOLYM_OK;
}

int volym_interpolate_pass(volym_ctx* c, const volym_interpolate* q)
{
    if (!c) return VOLYM_E_INVALID;
    if (!q) return fail(c, VOLYM_E_INVALID, "volym_interpolate_pass: NULL request");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_interpolate_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_interpolate_check(q, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_interpolate_pass: need lo <= hi <= volume size on every axis, at most 2^31 - 2 texels in the box, known flags, "
                                        "min_byte in 0..255, weights in 1..64 and an axis in 0..2");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_interpolate_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;       // where the other passes over a box go
    const uint32_t n_texels = static_cast<uint32_t>(box_texels(q->box));      // (checked: at most 2^31 - 2)
    const bool empty = n_texels == 0u;
    const uint32_t w = q->box[3] - q->box[0], h = q->box[4] - q->box[1], d = q->box[5] - q->box[2];
    const uint32_t n_rows = empty ? 0u : h * d;

    // (set-up steps: the one blocking path of a pass.  Whatever grows voids the snapshot first; should an allocation fail none is left)
    if (c->interpolate.capacity < 1u || c->interpolate_counts.capacity < INTERPOLATE_SLICES || n_texels > c->interpolate_state.capacity) {
        c->interpolate.count = 0;
        rc = c->interpolate.reserve(c, stream, 1, "interpolate summary");
        if (rc == VOLYM_OK) rc = c->interpolate_counts.reserve(c, stream, INTERPOLATE_SLICES, "interpolate slice counts");
        if (rc == VOLYM_OK && n_texels > c->interpolate_state.capacity) {
            rc = c->interpolate_state.reserve(c, stream, n_texels, "interpolate state map");
            if (rc == VOLYM_OK) { c->interpolate_work.release(); rc = c->interpolate_work.reserve(c, stream, 4u * static_cast<size_t>(n_texels), "interpolate maps and work arrays"); }
        }
        if (rc != VOLYM_OK) { free_interpolate(c); return rc; }
    }
    uint32_t* const summary = reinterpret_cast<uint32_t*>(c->interpolate.ptr);
    uint32_t* const counts = c->interpolate_counts.ptr;
    hipLaunchKernelGGL(volym_interpolate_init_kernel, dim3(1), dim3(256), 0, stream, summary, counts);
    HIPCHK(c, hipGetLastError());
    c->interpolate.count = 1;
    c->interpolate_state.count = n_texels;
    c->interpolate_texels = n_texels;
    std::memcpy(c->interpolate_box, q->box, sizeof c->interpolate_box);
    if (empty) return VOLYM_OK;                         // no texel, no slice: the summary of the zeroing kernel, no maps

    const bool uncut = (q->flags & VOLYM_INTERPOLATE_UNCUT) != 0u;
    const InterpolateArgs a = {box_walk_args(c, q->box, q->min_byte, uncut && c->d_vol0 ? c->d_vol0 : c->d_vol, with_labels),
                               {q->weight[0], q->weight[1], q->weight[2]}, q->axis, q->max_gap, (q->flags & VOLYM_INTERPOLATE_KEYS) ? 1u : 0u};
    BoxSelect select;
    std::memcpy(select.v, q->select, 256);
    InterpolateKeys keys;
    std::memcpy(keys.v, q->keys, sizeof keys.v);
    uint32_t* const dout = c->interpolate_work.ptr;
    uint32_t* const din = dout + n_texels;
    uint32_t* const stack = din + n_texels;             // ... and the signed map, once the sweeps are done
    uint32_t* const stack_g = stack + n_texels;
    uint8_t* const state = c->interpolate_state.ptr;
    const dim3 grid(walk_grid(c, n_rows)), block(256);
    const bool axis_x = q->axis == 0u;

    const auto rows = axis_x ? (with_labels ? volym_interpolate_rows_kernel<true, true> : volym_interpolate_rows_kernel<false, true>)
                             : (with_labels ? volym_interpolate_rows_kernel<true, false> : volym_interpolate_rows_kernel<false, false>);
    hipLaunchKernelGGL(rows, grid, block, 0, stream, a, select, dout, din, state, counts);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(volym_interpolate_keys_kernel, dim3(1), block, 0, stream, a, keys, counts, summary);
    HIPCHK(c, hipGetLastError());
    // the column sweeps, one lane per column, of the in-plane axes the rows have not covered, for both maps.  An axis of one texel has
    // nothing to sweep.
    const InterpolateColumns along_y = {h, w, w * d, w, w * h, q->weight[1], axis_x ? 1u : w, axis_x ? w : 0xffffffffu};
    const InterpolateColumns along_z = {d, w * h, w * h, w * h, 0u, q->weight[2], axis_x ? 1u : w, axis_x ? w : 0xffffffffu};
    const InterpolateColumns* const sweeps[2] = {q->axis != 1u && h > 1u ? &along_y : nullptr, q->axis != 2u && d > 1u ? &along_z : nullptr};
    for (const InterpolateColumns* cols : sweeps) {
        if (!cols) continue;
        for (uint32_t* map : {dout, din}) {
            hipLaunchKernelGGL(volym_interpolate_columns_kernel, dim3((cols->n_cols + 63u) / 64u), dim3(64), 0, stream, *cols, summary, map, stack, stack_g);
            HIPCHK(c, hipGetLastError());
        }
    }
    if (axis_x) hipLaunchKernelGGL(volym_interpolate_resolve_kernel<true>, grid, block, 0, stream, a, dout, din, stack, state, summary);
    else hipLaunchKernelGGL(volym_interpolate_resolve_kernel<false>, grid, block, 0, stream, a, dout, din, stack, state, summary);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_interpolate(volym_ctx* c, struct volym_interpolate_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_interpolate: NULL output");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_read_interpolate: no volym_interpolate_pass since the volume was set");
    return c->interpolate.read(c, c->slot0().stream, out, 1);
}

int volym_read_interpolate_map(volym_ctx* c, const uint32_t sub[6], uint32_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_volume(c, "volym_read_interpolate_map", "volym_interpolate_pass", have_pass(c), c->interpolate_box, signed_map(c), sub, out);
}

int volym_read_interpolate_state(volym_ctx* c, const uint32_t sub[6], uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    const std::string who = "volym_read_interpolate_state";
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, who + ": no volym_interpolate_pass since the volume was set");
    const uint32_t* const box = c->interpolate_box;
    if (!sub) sub = box;
    for (int k = 0; k < 3; ++k)
        if (sub[k] > sub[3 + k] || sub[k] < box[k] || sub[3 + k] > box[3 + k])
            return fail(c, VOLYM_E_INVALID, who + ": the sub-box must have lo <= hi and lie inside the box of the pass");
    const uint64_t total = box_texels(sub);
    if (total == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, who + ": NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    const uint32_t w = box[3] - box[0], h = box[4] - box[1], sw = sub[3] - sub[0], sh = sub[4] - sub[1];
    const uint32_t first = (sub[0] - box[0]) + w * ((sub[1] - box[1]) + h * (sub[2] - box[2]));
    if (sw == w && sh == h) return read_back(c, stream, out, c->interpolate_state.ptr + first, total);      // whole slices: one run
    // any other sub-box: gathered on the device into a buffer for the length of the call, as volym_read_labels does
    uint8_t* d_out = nullptr;
    hipError_t e = hipMalloc(&d_out, total);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(interpolate state read-back): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(volym_interpolate_gather_kernel, dim3(static_cast<uint32_t>((total + 255u) / 256u)), dim3(256), 0, stream, c->interpolate_state.ptr, d_out, w, h,
                       first, sw, sh, static_cast<uint32_t>(total));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, VOLYM_E_HIP, who + ": " + hipGetErrorString(e));
    return VOLYM_OK;
}

int volym_interpolate_at(volym_ctx* c, uint32_t x, uint32_t y, uint32_t z, uint32_t* word, uint8_t* state)
{
    if (!c) return VOLYM_E_INVALID;
    const std::string who = "volym_interpolate_at";
    if (!word && !state) return fail(c, VOLYM_E_INVALID, who + ": NULL output");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, who + ": no volym_interpolate_pass since the volume was set");
    const uint32_t* const box = c->interpolate_box;
    if (x < box[0] || x >= box[3] || y < box[1] || y >= box[4] || z < box[2] || z >= box[5])
        return fail(c, VOLYM_E_INVALID, who + ": the texel lies outside the box of the pass");
    // checked once; then only what was asked for is read
    const size_t at = (x - box[0]) + static_cast<size_t>(box[3] - box[0]) * ((y - box[1]) + (box[4] - box[1]) * static_cast<size_t>(z - box[2]));
    const hipStream_t stream = c->slot0().stream;
    int rc = VOLYM_OK;
    if (word) rc = read_back(c, stream, word, signed_map(c) + at, sizeof *word);
    if (rc == VOLYM_OK && state) rc = read_back(c, stream, state, c->interpolate_state.ptr + at, 1);
    return rc;
}

void* volym_interpolate_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->interpolate.ptr : nullptr; }
void* volym_interpolate_map_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? signed_map(c) : nullptr; }
void* volym_interpolate_state_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->interpolate_state.ptr : nullptr; }

int volym_interpolate_labels_check(const volym_interpolate_edit* e, const uint32_t dims[3])
{
    if (!e || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(e->box, dims)) return VOLYM_E_INVALID;
    if (e->flags & ~static_cast<uint32_t>(VOLYM_INTERPOLATE_EDIT_UNCUT | VOLYM_INTERPOLATE_EDIT_DRY_RUN)) return VOLYM_E_INVALID;
    if (e->min_byte > e->max_byte || e->max_byte > 255u) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_interpolate_labels(volym_ctx* c, const volym_interpolate_edit* e, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!e) return fail(c, VOLYM_E_INVALID, "volym_interpolate_labels: NULL request");
    const int ok = editable_state(c, "volym_interpolate_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_interpolate_labels_check(e, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_interpolate_labels: need lo <= hi <= volume size on every axis, known flags and min_byte <= max_byte <= 255");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_interpolate_labels: no volym_interpolate_pass since the volume was set");
    for (int a = 0; a < 3; ++a)
        if (e->box[a] < c->interpolate_box[a] || e->box[3 + a] > c->interpolate_box[3 + a])
            return fail(c, VOLYM_E_INVALID, "volym_interpolate_labels: a box that reaches outside the box of the interpolate pass");
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = interpolate_labels(c, e, res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

}  // extern "C"
