// The projection pass (gfx950): maximum and mean intensity along the view rays.  A unit of its own, as pick.hip, outline.hip,
// slice.hip and scene_bytes.hip are: nothing here is instantiated in, or changes, the units of the frame, pick, outline, slice or
// scene kernels.  It holds the pass's kernel (project_kernels.h), its C ABI (volym_project_pass, volym_project_image_pass,
// volym_read_projection, volym_read_projection_image, the two device pointers and sizes, volym_project_at), the host arithmetic of the rule
// (volym_project_check, volym_project_samples) and what the context keeps for it: its own records and image, their capacities and
// the rect size of the latest pass into each.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstring>

#include "context.hpp"
#include "project_kernels.h"

static_assert(sizeof(volym_project) == 1040 && offsetof(volym_project, background) == 12 && offsetof(volym_project, palette) == 16, "volym_project has no padding");
static_assert(sizeof(volym_projection) == sizeof(uint4), "a projection record is one 16-byte store");
static_assert(offsetof(volym_projection, x) == 4 && offsetof(volym_projection, z) == 8 && offsetof(volym_projection, max) == 10 && offsetof(volym_projection, mean) == 11 &&
              offsetof(volym_projection, label) == 12 && offsetof(volym_projection, status) == 13 && offsetof(volym_projection, n_samples) == 14,
              "the kernel packs the record by these offsets");
static_assert(VOLYM_PROJECT_TF == static_cast<int>(volym::PROJECT_TF) && VOLYM_PROJECT_LABELS == static_cast<int>(volym::PROJECT_LABELS) &&
              VOLYM_PROJECT_NO_SKIP == static_cast<int>(volym::PROJECT_NO_SKIP), "the kernel's flag bits are the header's");
static_assert(sizeof(volym::ProjectArgs) + sizeof(volym::FrameParams) < 4096, "palette and table travel with the launch: kernel arguments stay below 4 KiB");

namespace volym {

void free_projection(volym_ctx* c)
{
    c->projection.release();
    c->projection_image.release();
    c->projection_at.release();
    c->projection_w = c->projection_h = c->projection_image_w = c->projection_image_h = 0;
}

// one validated launch; own_image: the image goes to the context's own target
static int project_pass(volym_ctx* c, const volym_project* p, const uint32_t rect[4], void* records_device, void* image_rgba8, bool own_image, const char* who)
{
    if (!c) return VOLYM_E_INVALID;
    const std::string name(who);
    if (!p) return ctx_fail(c, VOLYM_E_INVALID, name + ": NULL volym_project");
    if (volym_project_check(p) != VOLYM_OK)
        return ctx_fail(c, VOLYM_E_INVALID, name + ": a step outside [1e-4, 1], an unknown mode or flag, or LABELS with MEAN");
    uint32_t r[4];
    int rc = frame_rect(c, rect, who, r);
    if (rc != VOLYM_OK) return rc;
    if (!c->have_vol) return ctx_fail(c, VOLYM_E_STATE, name + ": no volume (volym_set_volume)");
    const bool with_labels = labels_fit(c);
    if ((p->flags & VOLYM_PROJECT_LABELS) && !with_labels)
        return ctx_fail(c, VOLYM_E_STATE, name + ": VOLYM_PROJECT_LABELS needs labels of the volume's dimensions on the device (volym_set_labels)");
    if ((p->flags & VOLYM_PROJECT_TF) && !c->have_tf)
        return ctx_fail(c, VOLYM_E_STATE, name + ": VOLYM_PROJECT_TF needs a transfer function (volym_set_transfer_function)");
    if (!c->have_frame) return ctx_fail(c, VOLYM_E_STATE, name + ": call volym_update first");
    FrameSlot& s0 = c->slot0();                    // where the pick passes go: ordered with them and with itself
    if (s0.fp.nx != c->nx || s0.fp.ny != c->ny || s0.fp.nz != c->nz)
        return ctx_fail(c, VOLYM_E_STATE, name + ": the volume changed since the last volym_update");
    VOLYM_HIPCHK(c, hipSetDevice(c->device));
    const size_t need = static_cast<size_t>(r[2]) * r[3];
    // grown on demand (a set-up step: the one blocking path of a pass)
    if (!records_device && (rc = c->projection.reserve(c, s0.stream, need, "projection records")) != VOLYM_OK) return rc;
    if (own_image && (rc = c->projection_image.reserve(c, s0.stream, need, "projection image")) != VOLYM_OK) return rc;

    ProjectArgs a;
    a.vol = c->d_vol;
    a.labels = with_labels ? c->d_labels : nullptr;
    a.mc = c->d_mc;
    a.out = static_cast<uint4*>(records_device ? records_device : static_cast<void*>(c->projection.ptr));
    a.image = own_image ? c->projection_image.ptr : static_cast<uint32_t*>(image_rgba8);
    a.x0 = r[0]; a.y0 = r[1]; a.w = r[2]; a.h = r[3];
    a.tiles_x = (a.w + 15u) / 16u;
    a.mc_n = c->mc_n;
    a.labels_bricked = c->labels_bricked ? 1u : 0u;
    a.mode = p->mode; a.flags = p->flags;
    a.tf_n = c->tf_n;
    a.background = pack_rgba(p->background);
    a.step = p->step;
    pack_palette_and_lut(c, p->palette, a.palette, a.lut);

    const uint32_t grid = a.tiles_x * ((a.h + 15u) / 16u);
    if (c->bricked) hipLaunchKernelGGL((volym_project_kernel<true>), dim3(grid), dim3(256), 0, s0.stream, a, s0.fp);
    else hipLaunchKernelGGL((volym_project_kernel<false>), dim3(grid), dim3(256), 0, s0.stream, a, s0.fp);
    VOLYM_HIPCHK(c, hipGetLastError());
    if (!records_device) { c->projection_w = r[2]; c->projection_h = r[3]; c->projection.count = need; }
    if (own_image) { c->projection_image_w = r[2]; c->projection_image_h = r[3]; c->projection_image.count = need; }
    return VOLYM_OK;
}

// t_k of the rule, in f32 (this unit is compiled with -ffp-contract=off: a multiply, then an add)
static float sample_t(float t_entry, float step, uint32_t k) { return t_entry + static_cast<float>(k) * step; }

}  // namespace volym

using namespace volym;

extern "C" {

int volym_project_check(const volym_project* p)
{
    if (!p) return VOLYM_E_INVALID;
    if (!std::isfinite(p->step) || !(p->step >= 1.0e-4f && p->step <= 1.0f)) return VOLYM_E_INVALID;
    if (p->mode > static_cast<uint32_t>(VOLYM_PROJECT_MEAN)) return VOLYM_E_INVALID;
    if (p->flags & ~static_cast<uint32_t>(VOLYM_PROJECT_TF | VOLYM_PROJECT_LABELS | VOLYM_PROJECT_NO_SKIP)) return VOLYM_E_INVALID;
    if (p->mode == static_cast<uint32_t>(VOLYM_PROJECT_MEAN) && (p->flags & VOLYM_PROJECT_LABELS)) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_project_samples(float t_entry, float t_exit, float step, uint32_t* n)
{
    if (!n) return VOLYM_E_INVALID;
    if (!std::isfinite(step) || !(step >= 1.0e-4f && step <= 1.0f)) return VOLYM_E_INVALID;
    if (!(t_entry >= 0.0f && t_entry <= 128.0f) || !(t_exit >= 0.0f && t_exit <= 128.0f)) return VOLYM_E_INVALID;
    if (!(t_entry < t_exit)) { *n = 0u; return VOLYM_OK; }
    // an estimate in double, then the rule itself decides: t_k does not decrease with k, so the count is the one k with
    // t_{k-1} < t_exit <= t_k
    const double est = std::ceil((static_cast<double>(t_exit) - static_cast<double>(t_entry)) / static_cast<double>(step));
    uint32_t k = est < 1.0 ? 1u : static_cast<uint32_t>(est);      // <= 128 / 1e-4
    while (k > 1u && !(sample_t(t_entry, step, k - 1u) < t_exit)) --k;
    while (sample_t(t_entry, step, k) < t_exit) ++k;
    *n = k;
    return VOLYM_OK;
}

int volym_project_pass(volym_ctx* c, const volym_project* p, const uint32_t rect[4], void* records_device, void* image_rgba8)
{
    return project_pass(c, p, rect, records_device, image_rgba8, false, "volym_project_pass");
}

int volym_project_image_pass(volym_ctx* c, const volym_project* p, const uint32_t rect[4])
{
    return project_pass(c, p, rect, nullptr, nullptr, true, "volym_project_image_pass");
}

int volym_read_projection(volym_ctx* c, struct volym_projection* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_read_projection: NULL output");
    if (c->projection.count == 0u) return ctx_fail(c, VOLYM_E_STATE, "volym_read_projection: no projection pass into the context's own records yet");
    return c->projection.read(c, c->slot0().stream, out, c->projection.count);
}

int volym_read_projection_image(volym_ctx* c, uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_read_projection_image: NULL output");
    if (c->projection_image.count == 0u) return ctx_fail(c, VOLYM_E_STATE, "volym_read_projection_image: no volym_project_image_pass yet");
    return c->projection_image.read(c, c->slot0().stream, out, c->projection_image.count);
}

void* volym_projection_device_ptr(volym_ctx* c) { return (c && c->projection.count != 0u) ? c->projection.ptr : nullptr; }
void* volym_projection_image_device_ptr(volym_ctx* c) { return (c && c->projection_image.count != 0u) ? c->projection_image.ptr : nullptr; }

int volym_projection_size(volym_ctx* c, uint32_t size[2])
{
    if (!c) return VOLYM_E_INVALID;
    if (!size) return ctx_fail(c, VOLYM_E_INVALID, "volym_projection_size: NULL output");
    size[0] = c->projection.count ? c->projection_w : 0u; size[1] = c->projection.count ? c->projection_h : 0u;
    return VOLYM_OK;
}

int volym_projection_image_size(volym_ctx* c, uint32_t size[2])
{
    if (!c) return VOLYM_E_INVALID;
    if (!size) return ctx_fail(c, VOLYM_E_INVALID, "volym_projection_image_size: NULL output");
    size[0] = c->projection_image.count ? c->projection_image_w : 0u; size[1] = c->projection_image.count ? c->projection_image_h : 0u;
    return VOLYM_OK;
}

int volym_project_at(volym_ctx* c, uint32_t x, uint32_t y, float step, struct volym_projection* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_project_at: NULL output");
    VOLYM_HIPCHK(c, hipSetDevice(c->device));
    // a record of its own (a set-up step, once): the context's own records keep what the latest pass put there
    int rc = c->projection_at.reserve(c, c->slot0().stream, 1, "projection record");
    if (rc != VOLYM_OK) return rc;
    volym_project p;
    std::memset(&p, 0, sizeof p);
    p.step = step;
    const uint32_t rect[4] = {x, y, 1u, 1u};
    rc = project_pass(c, &p, rect, c->projection_at.ptr, nullptr, false, "volym_project_at");
    if (rc != VOLYM_OK) return rc;
    return c->projection_at.read(c, c->slot0().stream, out, 1);
}

}  // extern "C"
