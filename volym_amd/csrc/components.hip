// libvolym_hip.so: the components pass (volym_components_pass, volym_components_check, volym_read_components,
// volym_read_component_table, volym_read_component_ids, volym_component_of and the three device pointers) beside the kernels it
// launches (components_kernels.h).  Like the surface pass it only reads the scene's bytes and is enqueue-only on slot 0's stream, but
// for the allocations; its results are a snapshot that later edits of the scene leave valid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

#include "components_kernels.h"
#include "context.hpp"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_components) == 292 && offsetof(volym_components, flags) == 24 && offsetof(volym_components, min_byte) == 28 &&
              offsetof(volym_components, select) == 32 && offsetof(volym_components, max_components) == 288, "volym_components has no padding");
static_assert(sizeof(volym_components_summary) == 2072 && offsetof(volym_components_summary, n_solid) == 8 && offsetof(volym_components_summary, recorded) == 16 &&
              offsetof(volym_components_summary, per_label) == 24 && sizeof(volym_components_summary) == 8u * COMPONENT_SUMMARY_WORDS,
              "volym_components_summary is the 259 words the kernels index");
static_assert(sizeof(volym_component) == 24 && offsetof(volym_component, x) == 0 && offsetof(volym_component, y) == 2 && offsetof(volym_component, z) == 4 &&
              offsetof(volym_component, label) == 6 && offsetof(volym_component, flags) == 7 && offsetof(volym_component, count) == 8 &&
              offsetof(volym_component, box) == 12, "volym_component is the six words the pack kernel stores");

void volym::free_components(volym_ctx* c)
{
    c->components.release();
    c->component_ids.release();
    c->component_table.release();
    c->component_work.release();
    c->component_offsets.release();
}

extern "C" {

int volym_components_check(const volym_components* q, const uint32_t dims[3])
{
    if (!q || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(q->box, dims)) return VOLYM_E_INVALID;
    if (q->flags & ~static_cast<uint32_t>(VOLYM_COMPONENTS_UNCUT | VOLYM_COMPONENTS_SPLIT_LABELS)) return VOLYM_E_INVALID;
    if (q->min_byte == 0u || q->min_byte > 255u) return VOLYM_E_INVALID;
    if (q->max_components > VOLYM_COMPONENTS_TABLE_MAX) return VOLYM_E_INVALID;
    if (!box_at_most(q->box, VOLYM_COMPONENTS_BOX_MAX)) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_components_pass(volym_ctx* c, const volym_components* q)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_components_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_components whole = {};                 // the whole volume, min_byte 1, every label selected, no flags, the default capacity
    whole_volume_box(dims, whole.box);
    whole.min_byte = 1u;
    std::memset(whole.select, 1, sizeof whole.select);
    if (!q) q = &whole;
    if (volym_components_check(q, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_components_pass: need lo <= hi <= volume size on every axis, at most 2^31 - 2 texels in the box, known flags, "
                                        "min_byte in 1..255 and max_components <= 2^24");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_components_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;       // where pick, measure and surface passes go
    const uint32_t n_texels = static_cast<uint32_t>(box_texels(q->box));      // (checked: at most 2^31 - 2)
    const bool empty = n_texels == 0u;
    const uint32_t n_rows = empty ? 0u : (q->box[4] - q->box[1]) * (q->box[5] - q->box[2]);
    // no more records than the box has texels: a component has at least one
    const uint32_t capacity = std::min(q->max_components ? q->max_components : VOLYM_COMPONENTS_DEFAULT_MAX, n_texels);

    // (set-up steps: the one blocking path of a pass.  Whatever grows voids the snapshot first; should an allocation fail none is left)
    const bool grows = c->components.capacity < 1u || n_texels > c->component_ids.capacity || capacity > c->component_table.capacity ||
                       n_rows > c->component_offsets.rows.capacity;
    if (grows) {
        c->components.count = 0;
        rc = c->components.reserve(c, stream, 1, "components summary");
        if (rc == VOLYM_OK) rc = c->component_ids.reserve(c, stream, n_texels, "component ids");
        if (rc == VOLYM_OK && capacity > c->component_table.capacity) {
            rc = c->component_table.reserve(c, stream, capacity, "component table");
            if (rc == VOLYM_OK) { c->component_work.release(); rc = c->component_work.reserve(c, stream, static_cast<size_t>(capacity) * COMPONENT_WORK_WORDS, "component table"); }
        }
        if (rc == VOLYM_OK) rc = c->component_offsets.reserve(c, stream, n_rows, "component row offsets");
        if (rc != VOLYM_OK) { free_components(c); return rc; }
    }
    unsigned long long* const summary = reinterpret_cast<unsigned long long*>(c->components.ptr);
    uint32_t* const work = c->component_work.ptr;
    const uint32_t init_grid = std::max(std::min((capacity * COMPONENT_WORK_WORDS + 255u) / 256u, static_cast<uint32_t>(c->n_cus) * 8u), 1u);
    hipLaunchKernelGGL(volym_components_init_kernel, dim3(init_grid), dim3(256), 0, stream, summary, work, capacity);
    HIPCHK(c, hipGetLastError());
    c->components.count = 1;
    c->component_ids.count = n_texels;
    c->component_table.count = capacity;
    std::memcpy(c->component_box, q->box, sizeof c->component_box);
    if (empty) return VOLYM_OK;                         // a zero summary, no ids, no records: nothing else is launched

    const bool uncut = (q->flags & VOLYM_COMPONENTS_UNCUT) != 0u;
    const bool split = (q->flags & VOLYM_COMPONENTS_SPLIT_LABELS) != 0u && with_labels;     // (without labels every label is 0: nothing to split)
    const ComponentsArgs a = {box_walk_args(c, q->box, q->min_byte, uncut && c->d_vol0 ? c->d_vol0 : c->d_vol, with_labels), capacity};
    BoxSelect select;
    std::memcpy(select.v, q->select, 256);
    uint32_t* const parent = c->component_ids.ptr;
    uint32_t* const rows = c->component_offsets.rows.ptr;
    const dim3 grid(walk_grid(c, n_rows)), block(256);

    const auto rows_kernel = !with_labels ? volym_components_rows_kernel<false, false>
                             : split      ? volym_components_rows_kernel<true, true>
                                          : volym_components_rows_kernel<true, false>;
    hipLaunchKernelGGL(rows_kernel, grid, block, 0, stream, a, select, parent, summary);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(split ? volym_components_merge_kernel<true> : volym_components_merge_kernel<false>, grid, block, 0, stream, a, parent);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(volym_components_flatten_kernel, grid, block, 0, stream, a, parent, rows);
    HIPCHK(c, hipGetLastError());
    rc = scan_row_offsets(c, stream, c->component_offsets, n_rows);      // roots per row -> the number of every row's first root, in place
    if (rc != VOLYM_OK) return rc;
    hipLaunchKernelGGL(with_labels ? volym_components_number_kernel<true> : volym_components_number_kernel<false>, grid, block, 0, stream, a, parent, rows,
                       work, summary);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(volym_components_relabel_kernel, grid, block, 0, stream, a, parent, work);
    HIPCHK(c, hipGetLastError());
    const uint32_t pack_grid = std::max(std::min((capacity + 255u) / 256u, static_cast<uint32_t>(c->n_cus) * 8u), 1u);
    hipLaunchKernelGGL(volym_components_pack_kernel, dim3(pack_grid), block, 0, stream, work, reinterpret_cast<uint32_t*>(c->component_table.ptr), summary, capacity);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_components(volym_ctx* c, struct volym_components_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_components: NULL output");
    if (c->components.count == 0u) return fail(c, VOLYM_E_STATE, "volym_read_components: no volym_components_pass since the volume was set");
    return c->components.read(c, c->slot0().stream, out, 1);
}

int volym_read_component_table(volym_ctx* c, struct volym_component* out, uint64_t capacity)
{
    if (!c) return VOLYM_E_INVALID;
    if (c->components.count == 0u) return fail(c, VOLYM_E_STATE, "volym_read_component_table: no volym_components_pass since the volume was set");
    uint64_t recorded = 0;
    const int rc = read_back(c, c->slot0().stream, &recorded, &c->components.ptr->recorded, sizeof recorded);
    if (rc != VOLYM_OK) return rc;
    if (capacity < recorded) return fail(c, VOLYM_E_INVALID, "volym_read_component_table: the output holds fewer records than the pass wrote (volym_read_components: recorded)");
    if (recorded == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_component_table: NULL output");
    return c->component_table.read(c, c->slot0().stream, out, static_cast<size_t>(recorded));
}

int volym_read_component_ids(volym_ctx* c, const uint32_t sub[6], uint32_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_volume(c, "volym_read_component_ids", "volym_components_pass", c->components.count != 0u, c->component_box, c->component_ids.ptr, sub, out);
}

int volym_component_of(volym_ctx* c, uint32_t x, uint32_t y, uint32_t z, uint32_t* id)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_texel(c, "volym_component_of", "volym_components_pass", c->components.count != 0u, c->component_box, c->component_ids.ptr, x, y, z, id);
}

void* volym_components_device_ptr(volym_ctx* c) { return (c && c->components.count != 0u) ? c->components.ptr : nullptr; }
void* volym_component_ids_device_ptr(volym_ctx* c) { return (c && c->components.count != 0u) ? c->component_ids.ptr : nullptr; }
void* volym_component_table_device_ptr(volym_ctx* c) { return (c && c->components.count != 0u) ? c->component_table.ptr : nullptr; }

}  // extern "C"
