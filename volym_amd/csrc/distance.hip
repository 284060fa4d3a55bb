// libvolym_hip.so: the distance pass (volym_distance_pass, volym_distance_check, volym_read_distance, volym_read_distance_map,
// volym_distance_at and the two device pointers) beside the kernels it launches (distance_kernels.h).  Like the components pass it
// only reads the scene's bytes and is enqueue-only on slot 0's stream, but for the allocations; its results are a snapshot that later
// edits of the scene leave valid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

#include "context.hpp"
#include "distance_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_distance) == 300 && offsetof(volym_distance, flags) == 24 && offsetof(volym_distance, min_byte) == 28 &&
              offsetof(volym_distance, select) == 32 && offsetof(volym_distance, weight) == 288, "volym_distance has no padding");
static_assert(sizeof(volym_distance_summary) == 6184 && offsetof(volym_distance_summary, n_present) == 8 && offsetof(volym_distance_summary, n_finite) == 16 &&
              offsetof(volym_distance_summary, max_d2) == 4u * DS_MAX_D2 && offsetof(volym_distance_summary, max_at) == 4u * DS_MAX_AT &&
              offsetof(volym_distance_summary, near_d2) == 4u * DS_NEAR_D2 && offsetof(volym_distance_summary, near_at) == 4u * DS_NEAR_AT &&
              offsetof(volym_distance_summary, hist) == 4u * DS_HIST && sizeof(volym_distance_summary) == 4u * DISTANCE_SUMMARY_WORDS,
              "volym_distance_summary is the 1546 words the kernels index");

void volym::free_distance(volym_ctx* c)
{
    c->distance.release();
    c->distance_map.release();
    c->distance_work.release();
    c->distance_keys.release();
}

extern "C" {

int volym_distance_check(const volym_distance* q, const uint32_t dims[3])
{
    if (!q || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(q->box, dims)) return VOLYM_E_INVALID;
    if (q->flags & ~static_cast<uint32_t>(VOLYM_DISTANCE_UNCUT | VOLYM_DISTANCE_INSIDE)) return VOLYM_E_INVALID;
    if (q->min_byte == 0u || q->min_byte > 255u) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a)
        if (q->weight[a] == 0u || q->weight[a] > VOLYM_DISTANCE_WEIGHT_MAX) return VOLYM_E_INVALID;
    if (!box_at_most(q->box, VOLYM_DISTANCE_BOX_MAX)) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_distance_pass(volym_ctx* c, const volym_distance* q)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_distance_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_distance whole = {};                   // the whole volume, min_byte 1, every label selected, weights 1, no flags
    whole_volume_box(dims, whole.box);
    whole.min_byte = 1u;
    std::memset(whole.select, 1, sizeof whole.select);
    whole.weight[0] = whole.weight[1] = whole.weight[2] = 1u;
    if (!q) q = &whole;
    if (volym_distance_check(q, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_distance_pass: need lo <= hi <= volume size on every axis, at most 2^31 - 2 texels in the box, known flags, "
                                        "min_byte in 1..255 and weights in 1..64");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_distance_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;       // where pick, measure, surface and components passes go
    const uint32_t n_texels = static_cast<uint32_t>(box_texels(q->box));      // (checked: at most 2^31 - 2)
    const bool empty = n_texels == 0u;
    const uint32_t w = q->box[3] - q->box[0], h = q->box[4] - q->box[1], d = q->box[5] - q->box[2];
    const uint32_t n_rows = empty ? 0u : h * d;

    // (set-up steps: the one blocking path of a pass.  Whatever grows voids the snapshot first; should an allocation fail none is left)
    if (c->distance.capacity < 1u || c->distance_keys.capacity < DISTANCE_KEY_WORDS || n_texels > c->distance_map.capacity) {
        c->distance.count = 0;
        rc = c->distance.reserve(c, stream, 1, "distance summary");
        if (rc == VOLYM_OK) rc = c->distance_keys.reserve(c, stream, DISTANCE_KEY_WORDS, "distance summary");
        if (rc == VOLYM_OK && n_texels > c->distance_map.capacity) {
            rc = c->distance_map.reserve(c, stream, n_texels, "distance map");
            if (rc == VOLYM_OK) { c->distance_work.release(); rc = c->distance_work.reserve(c, stream, 2u * static_cast<size_t>(n_texels), "distance work arrays"); }
        }
        if (rc != VOLYM_OK) { free_distance(c); return rc; }
    }
    unsigned long long* const keys = c->distance_keys.ptr;
    uint32_t* const summary = reinterpret_cast<uint32_t*>(c->distance.ptr);
    hipLaunchKernelGGL(volym_distance_init_kernel, dim3(1), dim3(256), 0, stream, keys, summary);
    HIPCHK(c, hipGetLastError());
    c->distance.count = 1;
    c->distance_map.count = n_texels;
    std::memcpy(c->distance_box, q->box, sizeof c->distance_box);
    if (empty) return VOLYM_OK;                         // no texel, no seed: the summary of the zeroing kernel, no map

    const bool uncut = (q->flags & VOLYM_DISTANCE_UNCUT) != 0u;
    const DistanceArgs a = {box_walk_args(c, q->box, q->min_byte, uncut && c->d_vol0 ? c->d_vol0 : c->d_vol, with_labels),
                            {q->weight[0], q->weight[1], q->weight[2]}, (q->flags & VOLYM_DISTANCE_INSIDE) ? 1u : 0u};
    BoxSelect select;
    std::memcpy(select.v, q->select, 256);
    uint32_t* const map = c->distance_map.ptr;
    uint32_t* const stack = c->distance_work.ptr;
    uint32_t* const stack_g = stack + n_texels;
    const dim3 grid(walk_grid(c, n_rows)), block(256);

    hipLaunchKernelGGL(with_labels ? volym_distance_rows_kernel<true> : volym_distance_rows_kernel<false>, grid, block, 0, stream, a, select, map, keys);
    HIPCHK(c, hipGetLastError());
    // the column sweeps, one lane per column: along y (the columns of every slice), then along z.  An axis of one texel has nothing to sweep.
    if (h > 1u) {
        const DistanceColumns cy = {h, w, w * d, w, w * h, q->weight[1]};
        hipLaunchKernelGGL(volym_distance_columns_kernel, dim3((cy.n_cols + 63u) / 64u), dim3(64), 0, stream, cy, map, stack, stack_g);
        HIPCHK(c, hipGetLastError());
    }
    if (d > 1u) {
        const DistanceColumns cz = {d, w * h, w * h, w * h, 0u, q->weight[2]};
        hipLaunchKernelGGL(volym_distance_columns_kernel, dim3((cz.n_cols + 63u) / 64u), dim3(64), 0, stream, cz, map, stack, stack_g);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(with_labels ? volym_distance_finish_kernel<true> : volym_distance_finish_kernel<false>, grid, block, 0, stream, a, map, keys);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(volym_distance_pack_kernel, dim3(1), block, 0, stream, a, keys, summary);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_distance(volym_ctx* c, struct volym_distance_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_distance: NULL output");
    if (c->distance.count == 0u) return fail(c, VOLYM_E_STATE, "volym_read_distance: no volym_distance_pass since the volume was set");
    return c->distance.read(c, c->slot0().stream, out, 1);
}

int volym_read_distance_map(volym_ctx* c, const uint32_t sub[6], uint32_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_volume(c, "volym_read_distance_map", "volym_distance_pass", c->distance.count != 0u, c->distance_box, c->distance_map.ptr, sub, out);
}

int volym_distance_at(volym_ctx* c, uint32_t x, uint32_t y, uint32_t z, uint32_t* d2)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_texel(c, "volym_distance_at", "volym_distance_pass", c->distance.count != 0u, c->distance_box, c->distance_map.ptr, x, y, z, d2);
}

void* volym_distance_device_ptr(volym_ctx* c) { return (c && c->distance.count != 0u) ? c->distance.ptr : nullptr; }
void* volym_distance_map_device_ptr(volym_ctx* c) { return (c && c->distance.count != 0u) ? c->distance_map.ptr : nullptr; }

}  // extern "C"
