// libvolym_hip.so: the surface passes (volym_surface_pass, volym_read_surface, volym_surface_device_ptr, volym_surface_faces_pass,
// volym_read_surface_faces, volym_surface_check) beside the kernels they launch (surface_kernels.h).  Like the measure pass they
// only read the scene's bytes and are enqueue-only on slot 0's stream, but for the allocations and the one read of the total.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

#include "context.hpp"
#include "surface_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_surface) == 288 && offsetof(volym_surface, flags) == 24 && offsetof(volym_surface, min_byte) == 28 &&
              offsetof(volym_surface, select) == 32, "volym_surface has no padding");
static_assert(sizeof(volym_surface_summary) == 24584 && offsetof(volym_surface_summary, total) == 12288 && offsetof(volym_surface_summary, pos) == 12296 &&
              offsetof(volym_surface_summary, neg) == 18440, "volym_surface_summary has no padding");
static_assert(sizeof(volym_surface_face) == 8 && offsetof(volym_surface_face, dir) == 6 && offsetof(volym_surface_face, label) == 7,
              "volym_surface_face is the 8 bytes the emit kernel stores");

void volym::free_surface(volym_ctx* c)
{
    c->surface.release();
    c->surface_offsets.release();
    c->surface_faces.release();
    c->surface_faces_valid = c->surface_total_known = false;
}

extern "C" {

int volym_surface_check(const volym_surface* s, const uint32_t dims[3])
{
    if (!s || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(s->box, dims)) return VOLYM_E_INVALID;
    if (s->flags & ~static_cast<uint32_t>(VOLYM_SURFACE_UNCUT)) return VOLYM_E_INVALID;
    if (s->min_byte == 0u || s->min_byte > 255u) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_surface_pass(volym_ctx* c, const volym_surface* s)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_surface_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_surface whole = {};                    // the whole volume, min_byte 1, every label selected, no flags
    whole_volume_box(dims, whole.box);
    whole.min_byte = 1u;
    std::memset(whole.select, 1, sizeof whole.select);
    if (!s) s = &whole;
    if (volym_surface_check(s, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_surface_pass: need lo <= hi <= volume size on every axis, known flags and min_byte in 1..255");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_surface_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;       // where pick, slice, projection and measure passes go
    const bool empty = box_empty(s->box);
    const uint32_t n_rows = empty ? 0u : (s->box[4] - s->box[1]) * (s->box[5] - s->box[2]);
    // (a set-up step, once: with the growth below the one blocking path of a pass)
    rc = c->surface.reserve(c, stream, 1, "surface summary");
    if (rc != VOLYM_OK) return rc;
    if (n_rows > c->surface_offsets.rows.capacity) c->surface.count = 0;      // the summary the offsets belong to is void from here on
    rc = c->surface_offsets.reserve(c, stream, n_rows, "surface row offsets");
    if (rc != VOLYM_OK) return rc;
    hipLaunchKernelGGL(volym_surface_init_kernel, dim3(1), dim3(256), 0, stream, reinterpret_cast<unsigned long long*>(c->surface.ptr),
                       static_cast<uint32_t>(sizeof(volym_surface_summary) / 8u));
    HIPCHK(c, hipGetLastError());
    const bool uncut = (s->flags & VOLYM_SURFACE_UNCUT) != 0u;
    c->surface.count = 1;
    c->surface_serial = c->scene_serial;
    c->surface_request = *s;
    c->surface_vol = uncut && c->d_vol0 ? c->d_vol0 : c->d_vol;
    c->surface_labels = with_labels;
    c->surface_total_known = empty;                     // (an empty box has no faces: nothing to learn)
    c->surface_total = 0;
    c->surface_faces_valid = false;
    if (empty) return VOLYM_OK;                         // a zero summary, no rows: nothing else is launched

    const SurfaceArgs a = box_walk_args(c, s->box, s->min_byte, c->surface_vol, with_labels);
    BoxSelect select;
    std::memcpy(select.v, s->select, 256);
    volym_surface_summary* d = c->surface.ptr;
    const SurfaceOut out = {reinterpret_cast<unsigned long long*>(&d->faces[0][0]), reinterpret_cast<unsigned long long*>(&d->total),
                            reinterpret_cast<unsigned long long*>(&d->pos[0][0]), reinterpret_cast<unsigned long long*>(&d->neg[0][0])};
    const auto count = with_labels ? volym_surface_count_kernel<true> : volym_surface_count_kernel<false>;
    hipLaunchKernelGGL(count, dim3(walk_grid(c, n_rows)), dim3(256), 0, stream, a, select, out, c->surface_offsets.rows.ptr);
    HIPCHK(c, hipGetLastError());
    return scan_row_offsets(c, stream, c->surface_offsets, n_rows);      // counts -> offsets, in place
}

int volym_read_surface(volym_ctx* c, struct volym_surface_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_surface: NULL output");
    if (c->surface.count == 0u) return fail(c, VOLYM_E_STATE, "volym_read_surface: no volym_surface_pass since the volume was set");
    const int rc = c->surface.read(c, c->slot0().stream, out, 1);
    if (rc != VOLYM_OK) return rc;
    c->surface_total = out->total;
    c->surface_total_known = true;
    return VOLYM_OK;
}

void* volym_surface_device_ptr(volym_ctx* c) { return (c && c->surface.count != 0u) ? c->surface.ptr : nullptr; }

int volym_surface_faces_pass(volym_ctx* c, void* target_device, uint64_t capacity_faces)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol || c->surface.count == 0u)
        return fail(c, VOLYM_E_STATE, "volym_surface_faces_pass: no volym_surface_pass since the volume was set");
    if (c->surface_serial != c->scene_serial)
        return fail(c, VOLYM_E_STATE, "volym_surface_faces_pass: the scene's bytes changed since the surface pass (run volym_surface_pass again)");
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    if (!c->surface_total_known) {
        uint64_t total = 0;
        const int rc = read_back(c, stream, &total, &c->surface.ptr->total, sizeof total);
        if (rc != VOLYM_OK) return rc;
        c->surface_total = total;
        c->surface_total_known = true;
    }
    const uint64_t total = c->surface_total;
    if (total > UINT32_MAX) return fail(c, VOLYM_E_INVALID, "volym_surface_faces_pass: more than 2^32 - 1 faces (the row offsets are 32-bit): ask for a smaller box");
    uint2* target = static_cast<uint2*>(target_device);
    if (target_device) {
        if (capacity_faces < total) return fail(c, VOLYM_E_INVALID, "volym_surface_faces_pass: the target holds fewer faces than the surface has (volym_read_surface: total)");
        if (reinterpret_cast<uintptr_t>(target_device) & 7u) return fail(c, VOLYM_E_INVALID, "volym_surface_faces_pass: the target must be 8-byte aligned");
    } else {
        c->surface_faces_valid = false;
        const int rc = c->surface_faces.reserve(c, stream, static_cast<size_t>(total), "surface faces");
        if (rc != VOLYM_OK) return rc;
        target = reinterpret_cast<uint2*>(c->surface_faces.ptr);
        c->surface_faces_valid = true;
        c->surface_faces.count = static_cast<size_t>(total);
    }
    if (total == 0u) return VOLYM_OK;                    // (an empty box has no rows either)
    const volym_surface& s = c->surface_request;
    const SurfaceArgs a = box_walk_args(c, s.box, s.min_byte, c->surface_vol, c->surface_labels);
    BoxSelect select;
    std::memcpy(select.v, s.select, 256);
    const auto emit = c->surface_labels ? volym_surface_emit_kernel<true> : volym_surface_emit_kernel<false>;
    hipLaunchKernelGGL(emit, dim3(walk_grid(c, a.n_rows)), dim3(256), 0, stream, a, select, c->surface_offsets.rows.ptr, target);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_surface_faces(volym_ctx* c, struct volym_surface_face* out, uint64_t capacity_faces)
{
    if (!c) return VOLYM_E_INVALID;
    if (c->surface.count == 0u || !c->surface_faces_valid)
        return fail(c, VOLYM_E_STATE, "volym_read_surface_faces: no volym_surface_faces_pass into the context's own buffer since the latest surface pass");
    const size_t n = c->surface_faces.count;
    if (capacity_faces < n) return fail(c, VOLYM_E_INVALID, "volym_read_surface_faces: the output holds fewer faces than the pass wrote");
    if (n == 0u) return VOLYM_OK;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_surface_faces: NULL output");
    return c->surface_faces.read(c, c->slot0().stream, out, n);
}

}  // extern "C"
