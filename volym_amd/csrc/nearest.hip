// libvolym_hip.so: the nearest pass (volym_nearest_pass, volym_nearest_check, the reads, volym_nearest_at and the three device
// pointers) and the fill by it (volym_fill_labels, volym_fill_check), beside the kernels they launch (nearest_kernels.h).  The pass is
// a read-only pass like the distance pass: enqueue-only on slot 0's stream but for the allocations, its results a snapshot that later
// edits of the scene leave valid.  The fill is an edit like the others and goes through label_edit.hpp's transition.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "label_edit.hpp"
#include "nearest_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_nearest_summary) == 8u * NEAREST_SUMMARY_WORDS && offsetof(volym_nearest_summary, n_present) == 8u * NS_N_PRESENT &&
              offsetof(volym_nearest_summary, n_finite) == 8u * NS_N_FINITE && offsetof(volym_nearest_summary, cell) == 8u * NS_CELL &&
              offsetof(volym_nearest_summary, cell_present) == 8u * NS_CELL_PRESENT, "volym_nearest_summary is the 515 words the kernels index");
static_assert(sizeof(volym_nearest_site) == 20 && offsetof(volym_nearest_site, d2) == 12 && offsetof(volym_nearest_site, label) == 16, "volym_nearest_site has no padding");
static_assert(sizeof(volym_fill) == 556 && offsetof(volym_fill, flags) == 24 && offsetof(volym_fill, min_byte) == 28 && offsetof(volym_fill, give) == 36 &&
              offsetof(volym_fill, take) == 292 && offsetof(volym_fill, d2_lo) == 548, "volym_fill has no padding");
static_assert(VOLYM_FILL_UNCUT == VOLYM_RELABEL_UNCUT, "edit_density reads the flag of either");

void volym::free_nearest(volym_ctx* c)
{
    c->nearest.release();
    c->nearest_sites.release();
    c->nearest_labels.release();
    c->nearest_winners.release();
    c->nearest_work.release();
}

static bool have_pass(const volym_ctx* c) { return c->nearest.count != 0u; }

// the sub-box of a read: NULL is the pass's box; lo <= hi and inside that box, in the name of `who`
static int sub_box(volym_ctx* c, const char* who, const uint32_t*& sub)
{
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, std::string(who) + ": no volym_nearest_pass since the volume was set");
    if (!sub) sub = c->nearest_box;
    for (int k = 0; k < 3; ++k)
        if (sub[k] > sub[3 + k] || sub[k] < c->nearest_box[k] || sub[3 + k] > c->nearest_box[3 + k])
            return fail(c, VOLYM_E_INVALID, std::string(who) + ": the sub-box must have lo <= hi and lie inside the box of the pass");
    return VOLYM_OK;
}

// volym_fill_labels' request as an edit: the table only marks the labels that give, the receiving labels are those that take
static int fill_labels(volym_ctx* c, const volym_fill* f, volym_relabel_result& res)
{
    const bool dry = (f->flags & VOLYM_FILL_DRY_RUN) != 0u, uncut_bytes = (f->flags & VOLYM_FILL_UNCUT) != 0u;
    FillRule rule = {};
    rule.min_byte = f->min_byte; rule.max_byte = f->max_byte;
    rule.d2_lo = f->d2_lo; rule.d2_hi = f->d2_hi;
    rule.store = dry ? 0u : 1u;
    std::memcpy(rule.box, c->nearest_box, sizeof rule.box);
    std::memcpy(rule.weight, c->nearest_weight, sizeof rule.weight);
    std::memcpy(rule.take, f->take, 256);
    uint8_t marks[256], receives[256];
    for (int l = 0; l < 256; ++l) { marks[l] = static_cast<uint8_t>(f->give[l] ? l ^ 1 : l); receives[l] = f->take[l] != 0u; }
    const uint32_t* sites = c->nearest_sites.ptr;
    const uint8_t* near = c->nearest_labels.ptr;
    const LabelEdit edit = {f->box, marks, dry, "volym_fill_labels", receives};
    return edit_labels(c, edit, res, [&](hipStream_t stream, dim3 grid, const RelabelOut& out, const LabelTable& to, const CropSlab& s, uint32_t items,
                                         const LabelJournal* journal) {
        launch_edit(c, volym_nearest_fill_kernel, volym_nearest_fill_journal_kernel, stream, grid, out, to, s, rule, items, journal, edit_density(c, uncut_bytes), sites,
                    near);
    });
}

extern "C" {

int volym_nearest_check(const volym_distance* q, const uint32_t dims[3])
{
    const int rc = volym_distance_check(q, dims);
    if (rc != VOLYM_OK) return rc;
    return (q->flags & VOLYM_DISTANCE_INSIDE) ? VOLYM_E_INVALID : VOLYM_OK;
}

int volym_nearest_pass(volym_ctx* c, const volym_distance* q)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_nearest_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_distance whole = {};                   // the whole volume, min_byte 1, every label selected, weights 1, no flags
    whole_volume_box(dims, whole.box);
    whole.min_byte = 1u;
    std::memset(whole.select, 1, sizeof whole.select);
    whole.weight[0] = whole.weight[1] = whole.weight[2] = 1u;
    if (!q) q = &whole;
    if (volym_nearest_check(q, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_nearest_pass: need lo <= hi <= volume size on every axis, at most 2^31 - 2 texels in the box, no flag but UNCUT, "
                                        "min_byte in 1..255 and weights in 1..64");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_nearest_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;       // where the distance pass goes: the two share work arrays in stream order
    const uint32_t n_texels = static_cast<uint32_t>(box_texels(q->box));      // (checked: at most 2^31 - 2)
    const bool empty = n_texels == 0u;
    const uint32_t w = q->box[3] - q->box[0], h = q->box[4] - q->box[1], d = q->box[5] - q->box[2];
    const uint32_t n_rows = empty ? 0u : h * d;
    const bool sweeps = !empty && (h > 1u || d > 1u);
    // the stacks: the distance pass's two work arrays where they are large enough, else the pass's own
    const bool borrow = c->distance_work.capacity >= 2u * static_cast<size_t>(n_texels);
    const size_t own_work = (sweeps && !borrow) ? 2u * static_cast<size_t>(n_texels) : 0u;

    // (set-up steps: the one blocking path of a pass.  Whatever grows voids the snapshot first; should an allocation fail none is left)
    if (c->nearest.capacity < 1u || n_texels > c->nearest_sites.capacity || own_work > c->nearest_work.capacity) {
        c->nearest.count = 0;
        rc = c->nearest.reserve(c, stream, 1, "nearest summary");
        if (rc == VOLYM_OK && n_texels > c->nearest_sites.capacity) {
            rc = c->nearest_sites.reserve(c, stream, n_texels, "nearest site map");
            if (rc == VOLYM_OK) { c->nearest_labels.release(); rc = c->nearest_labels.reserve(c, stream, n_texels, "nearest label map"); }
            if (rc == VOLYM_OK) { c->nearest_winners.release(); rc = c->nearest_winners.reserve(c, stream, 3u * static_cast<size_t>(n_texels), "nearest winners"); }
        }
        if (rc == VOLYM_OK) rc = c->nearest_work.reserve(c, stream, own_work, "nearest work arrays");
        if (rc != VOLYM_OK) { free_nearest(c); return rc; }
    }
    unsigned long long* const summary = reinterpret_cast<unsigned long long*>(c->nearest.ptr);
    hipLaunchKernelGGL(volym_nearest_init_kernel, dim3(1), dim3(256), 0, stream, summary);
    HIPCHK(c, hipGetLastError());
    c->nearest.count = 1;
    c->nearest_sites.count = c->nearest_labels.count = n_texels;
    std::memcpy(c->nearest_box, q->box, sizeof c->nearest_box);
    std::memcpy(c->nearest_weight, q->weight, sizeof c->nearest_weight);
    if (empty) return VOLYM_OK;                         // no texel, no seed: the summary of the zeroing kernel, no maps

    const bool uncut = (q->flags & VOLYM_DISTANCE_UNCUT) != 0u;
    const NearestArgs a = {box_walk_args(c, q->box, q->min_byte, uncut && c->d_vol0 ? c->d_vol0 : c->d_vol, with_labels), {q->weight[0], q->weight[1], q->weight[2]}};
    BoxSelect select;
    std::memcpy(select.v, q->select, 256);
    uint32_t* const g = c->nearest_sites.ptr;           // the sweeps' g, until the resolve kernel stores the sites over it
    uint8_t* const near = c->nearest_labels.ptr;
    uint16_t* const wx = c->nearest_winners.ptr;
    uint16_t* const wy = wx + n_texels;
    uint16_t* const wz = wy + n_texels;
    uint32_t* const stack = borrow ? c->distance_work.ptr : c->nearest_work.ptr;
    uint32_t* const stack_g = stack + n_texels;
    const dim3 grid(walk_grid(c, n_rows)), block(256);

    hipLaunchKernelGGL(with_labels ? volym_nearest_rows_kernel<true> : volym_nearest_rows_kernel<false>, grid, block, 0, stream, a, select, g, wx, summary);
    HIPCHK(c, hipGetLastError());
    // the column sweeps, one lane per column: along y (the columns of every slice), then along z.  An axis of one texel has nothing to
    // sweep, and the resolve kernel takes the texel's own coordinate for its winner.
    if (h > 1u) {
        const NearestColumns cy = {h, w, w * d, w, w * h, q->weight[1]};
        hipLaunchKernelGGL(volym_nearest_columns_kernel, dim3((cy.n_cols + 63u) / 64u), dim3(64), 0, stream, cy, g, stack, stack_g, wy);
        HIPCHK(c, hipGetLastError());
    }
    if (d > 1u) {
        const NearestColumns cz = {d, w * h, w * h, w * h, 0u, q->weight[2]};
        hipLaunchKernelGGL(volym_nearest_columns_kernel, dim3((cz.n_cols + 63u) / 64u), dim3(64), 0, stream, cz, g, stack, stack_g, wz);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(with_labels ? volym_nearest_resolve_kernel<true> : volym_nearest_resolve_kernel<false>, grid, block, 0, stream, a, select, d, wx, wy, wz, g, near,
                       summary);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_nearest(volym_ctx* c, struct volym_nearest_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_nearest: NULL output");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_read_nearest: no volym_nearest_pass since the volume was set");
    return c->nearest.read(c, c->slot0().stream, out, 1);
}

int volym_read_nearest_sites(volym_ctx* c, const uint32_t sub[6], uint32_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_volume(c, "volym_read_nearest_sites", "volym_nearest_pass", have_pass(c), c->nearest_box, c->nearest_sites.ptr, sub, out);
}

int volym_read_nearest_labels(volym_ctx* c, const uint32_t sub[6], uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    const char* const who = "volym_read_nearest_labels";
    const int ok = sub_box(c, who, sub);
    if (ok != VOLYM_OK) return ok;
    const uint64_t total = box_texels(sub);
    if (total == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, std::string(who) + ": NULL output");
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    const uint32_t* const box = c->nearest_box;
    const uint32_t w = box[3] - box[0], h = box[4] - box[1], sw = sub[3] - sub[0], sh = sub[4] - sub[1];
    const uint32_t first = (sub[0] - box[0]) + w * ((sub[1] - box[1]) + h * (sub[2] - box[2]));
    if (sw == w && sh == h) return read_back(c, stream, out, c->nearest_labels.ptr + first, total);      // whole slices: one run
    // any other sub-box: gathered on the device into a buffer for the length of the call, as volym_read_labels does
    uint8_t* d_out = nullptr;
    hipError_t e = hipMalloc(&d_out, total);
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(nearest label read-back): ") + hipGetErrorString(e));
    hipLaunchKernelGGL(volym_nearest_gather_kernel, dim3(static_cast<uint32_t>((total + 255u) / 256u)), dim3(256), 0, stream, c->nearest_labels.ptr, d_out, w, h, first,
                       sw, sh, static_cast<uint32_t>(total));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, VOLYM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return VOLYM_OK;
}

int volym_nearest_at(volym_ctx* c, uint32_t x, uint32_t y, uint32_t z, struct volym_nearest_site* out)
{
    if (!c) return VOLYM_E_INVALID;
    uint32_t site = NEAREST_NONE;
    int rc = read_box_texel(c, "volym_nearest_at", "volym_nearest_pass", have_pass(c), c->nearest_box, c->nearest_sites.ptr, x, y, z, out ? &site : nullptr);
    if (rc != VOLYM_OK) return rc;
    const uint32_t* const box = c->nearest_box;
    const uint32_t w = box[3] - box[0], h = box[4] - box[1];
    *out = volym_nearest_site{{0u, 0u, 0u}, NEAREST_NONE, 0u};
    if (site == NEAREST_NONE) return VOLYM_OK;
    uint8_t label = 0;
    rc = read_back(c, c->slot0().stream, &label, c->nearest_labels.ptr + ((x - box[0]) + static_cast<size_t>(w) * ((y - box[1]) + h * static_cast<size_t>(z - box[2]))), 1);
    if (rc != VOLYM_OK) return rc;
    out->at[0] = box[0] + site % w; out->at[1] = box[1] + (site / w) % h; out->at[2] = box[2] + site / (w * h);
    const uint32_t t[3] = {x, y, z};
    out->d2 = 0u;
    for (int a = 0; a < 3; ++a) { const uint32_t dd = t[a] > out->at[a] ? t[a] - out->at[a] : out->at[a] - t[a]; out->d2 += c->nearest_weight[a] * dd * dd; }
    out->label = label;
    return VOLYM_OK;
}

void* volym_nearest_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->nearest.ptr : nullptr; }
void* volym_nearest_sites_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->nearest_sites.ptr : nullptr; }
void* volym_nearest_labels_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->nearest_labels.ptr : nullptr; }

int volym_fill_check(const volym_fill* f, const uint32_t dims[3])
{
    if (!f || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(f->box, dims)) return VOLYM_E_INVALID;
    if (f->flags & ~static_cast<uint32_t>(VOLYM_FILL_UNCUT | VOLYM_FILL_DRY_RUN)) return VOLYM_E_INVALID;
    if (f->min_byte > f->max_byte || f->max_byte > 255u) return VOLYM_E_INVALID;
    if (f->d2_lo > f->d2_hi) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_fill_labels(volym_ctx* c, const volym_fill* f, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!f) return fail(c, VOLYM_E_INVALID, "volym_fill_labels: NULL request");
    const int ok = editable_state(c, "volym_fill_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_fill_check(f, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_fill_labels: need lo <= hi <= volume size on every axis, known flags, min_byte <= max_byte <= 255 and d2_lo <= d2_hi");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_fill_labels: no volym_nearest_pass since the volume was set");
    for (int a = 0; a < 3; ++a)
        if (f->box[a] < c->nearest_box[a] || f->box[3 + a] > c->nearest_box[3 + a])
            return fail(c, VOLYM_E_INVALID, "volym_fill_labels: a box that reaches outside the box of the nearest pass");
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = fill_labels(c, f, res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

}  // extern "C"
