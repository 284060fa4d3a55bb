// The slice pass (gfx950): axis-aligned and oblique planes of the scene, gathered on the device.  A unit of its own, as pick.hip,
// outline.hip and scene_bytes.hip are: nothing here is instantiated in, or changes, the units of the frame, pick, outline or scene
// kernels.  It holds the pass's kernel (slice_kernels.h), its C ABI (volym_slice_pass, volym_read_slice, volym_slice_device_ptr),
// the host arithmetic of a slice (volym_slice_check, volym_slice_axis, volym_slice_texel) and what the context keeps for it: its
// own target, that target's capacity and the size of the latest pass into it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "context.hpp"
#include "slice_kernels.h"

static_assert(sizeof(volym_slice) == 1084, "volym_slice is 1084 bytes");
static_assert(offsetof(volym_slice, width) == 36 && offsetof(volym_slice, background) == 52 && offsetof(volym_slice, palette) == 60, "volym_slice has no padding");
static_assert(VOLYM_SLICE_LABELS == static_cast<int>(volym::SLICE_LABELS) && VOLYM_SLICE_MARK_CUT == static_cast<int>(volym::SLICE_MARK_CUT), "the kernel's flag bits are the header's");

namespace volym {

// position of pixel (i, j) on axis a, over the integers
static int64_t slice_pos(const volym_slice* s, int a, uint32_t i, uint32_t j)
{
    return static_cast<int64_t>(s->origin[a]) + static_cast<int64_t>(i) * s->du[a] + static_cast<int64_t>(j) * s->dv[a];
}

void free_slice(volym_ctx* c)
{
    c->slice.release();
    c->slice_w = c->slice_h = 0;
}

}  // namespace volym

using namespace volym;

extern "C" {

int volym_slice_check(const volym_slice* s)
{
    if (!s) return VOLYM_E_INVALID;
    if (s->mode > static_cast<uint32_t>(VOLYM_SLICE_IMPORTANCE)) return VOLYM_E_INVALID;
    if (s->flags & ~static_cast<uint32_t>(VOLYM_SLICE_UNCUT | VOLYM_SLICE_LABELS | VOLYM_SLICE_MARK_CUT)) return VOLYM_E_INVALID;
    if (s->mode == static_cast<uint32_t>(VOLYM_SLICE_IMPORTANCE) && (s->flags & VOLYM_SLICE_UNCUT)) return VOLYM_E_INVALID;
    if (s->width < 1u || s->width > 8192u || s->height < 1u || s->height > 8192u) return VOLYM_E_INVALID;
    const int64_t lim = int64_t{1} << 30;
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 4; ++k) {
            const int64_t p = slice_pos(s, a, (k & 1) ? s->width - 1u : 0u, (k & 2) ? s->height - 1u : 0u);
            if (p < -lim || p >= lim) return VOLYM_E_INVALID;
        }
    return VOLYM_OK;
}

int volym_slice_axis(int axis, uint32_t index, const uint32_t dims[3], volym_slice* out)
{
    if (!dims || !out || axis < 0 || axis > 2) return VOLYM_E_INVALID;
    if (index >= dims[axis]) return VOLYM_E_INVALID;
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;      // z: u = +x, v = +y.  y: u = +x, v = +z.  x: u = +y, v = +z
    if (dims[u] < 1u || dims[u] > 8192u || dims[v] < 1u || dims[v] > 8192u || index >= (1u << 14)) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a) { out->origin[a] = 0x8000; out->du[a] = 0; out->dv[a] = 0; }     // through texel centres
    out->origin[axis] = static_cast<int32_t>((index << 16) + 0x8000u);
    out->du[u] = 1 << 16;
    out->dv[v] = 1 << 16;
    out->width = dims[u];
    out->height = dims[v];
    return VOLYM_OK;
}

int volym_slice_texel(const volym_slice* s, uint32_t i, uint32_t j, int32_t t[3])
{
    if (!s || !t || i >= s->width || j >= s->height) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a) {
        const int64_t q = slice_pos(s, a, i, j) >> 16;      // floor: an arithmetic shift
        if (q < INT32_MIN || q > INT32_MAX) return VOLYM_E_INVALID;
        t[a] = static_cast<int32_t>(q);
    }
    return VOLYM_OK;
}

int volym_slice_pass(volym_ctx* c, const volym_slice* sl, void* target_rgba8)
{
    if (!c) return VOLYM_E_INVALID;
    if (!sl) return ctx_fail(c, VOLYM_E_INVALID, "volym_slice_pass: NULL volym_slice");
    if (volym_slice_check(sl) != VOLYM_OK)
        return ctx_fail(c, VOLYM_E_INVALID, "volym_slice_pass: unknown mode or flag, IMPORTANCE with UNCUT, a size outside 1..8192 or a corner outside [-2^30, 2^30)");
    if (!c->have_vol) return ctx_fail(c, VOLYM_E_STATE, "volym_slice_pass: no volume (volym_set_volume)");
    const bool with_labels = labels_fit(c);
    if ((sl->flags & VOLYM_SLICE_LABELS) && !with_labels)
        return ctx_fail(c, VOLYM_E_STATE, "volym_slice_pass: VOLYM_SLICE_LABELS needs labels of the volume's dimensions on the device (volym_set_labels)");
    if (sl->mode == static_cast<uint32_t>(VOLYM_SLICE_IMPORTANCE) && !(c->have_imp && c->d_imp && c->inx == c->nx && c->iny == c->ny && c->inz == c->nz))
        return ctx_fail(c, VOLYM_E_STATE, "volym_slice_pass: VOLYM_SLICE_IMPORTANCE needs importances of the volume's dimensions");
    if (sl->mode == static_cast<uint32_t>(VOLYM_SLICE_TF) && !c->have_tf)
        return ctx_fail(c, VOLYM_E_STATE, "volym_slice_pass: VOLYM_SLICE_TF needs a transfer function (volym_set_transfer_function)");
    VOLYM_HIPCHK(c, hipSetDevice(c->device));
    FrameSlot& s0 = c->slot0();                    // where the pick passes go: ordered with them and with itself
    uint32_t* dst = static_cast<uint32_t*>(target_rgba8);
    if (!dst) {
        // grown on demand (a set-up step: the one blocking path of the call)
        const int rc = c->slice.reserve(c, s0.stream, static_cast<size_t>(sl->width) * sl->height, "slice target");
        if (rc != VOLYM_OK) return rc;
        dst = c->slice.ptr;
    }

    SliceArgs a;
    a.vol = ((sl->flags & VOLYM_SLICE_UNCUT) && c->d_vol0) ? c->d_vol0 : c->d_vol;
    a.imp = c->d_imp;
    a.labels = with_labels ? c->d_labels : nullptr;
    a.out = dst;
    for (int k = 0; k < 3; ++k) {
        a.origin[k] = static_cast<uint32_t>(sl->origin[k]); a.du[k] = static_cast<uint32_t>(sl->du[k]); a.dv[k] = static_cast<uint32_t>(sl->dv[k]);
        a.crop_lo[k] = c->crop_lo[k]; a.crop_hi[k] = c->crop_hi[k];
        a.clip_n[k] = c->clip_n[k];
    }
    a.clip_d = c->clip_d;
    a.width = sl->width; a.height = sl->height;
    a.tiles_x = (sl->width + 15u) / 16u;
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    a.mode = sl->mode; a.flags = sl->flags;
    a.imp_bricked = c->imp_bricked ? 1u : 0u;
    a.labels_bricked = c->labels_bricked ? 1u : 0u;
    a.tf_n = c->tf_n;
    a.background = pack_rgba(sl->background);
    a.cut = pack_rgba(sl->cut_rgba);
    std::memset(a.hidden, 0, sizeof a.hidden);
    if (with_labels)
        for (uint32_t l = 0; l < 256u; ++l)
            if (c->seg_hidden[l]) a.hidden[l >> 5] |= 1u << (l & 31u);
    pack_palette_and_lut(c, sl->palette, a.palette, a.lut);

    const uint32_t grid = a.tiles_x * ((sl->height + 15u) / 16u);        // <= 512 * 512
    if (c->bricked) hipLaunchKernelGGL((volym_slice_kernel<true>), dim3(grid), dim3(256), 0, s0.stream, a);
    else hipLaunchKernelGGL((volym_slice_kernel<false>), dim3(grid), dim3(256), 0, s0.stream, a);
    VOLYM_HIPCHK(c, hipGetLastError());
    if (!target_rgba8) { c->slice_w = sl->width; c->slice_h = sl->height; c->slice.count = static_cast<size_t>(sl->width) * sl->height; }
    return VOLYM_OK;
}

int volym_read_slice(volym_ctx* c, uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_read_slice: NULL output");
    if (c->slice.count == 0u) return ctx_fail(c, VOLYM_E_STATE, "volym_read_slice: no volym_slice_pass into the context's own target yet");
    return c->slice.read(c, c->slot0().stream, out, c->slice.count);
}

void* volym_slice_device_ptr(volym_ctx* c) { return (c && c->slice.count != 0u) ? c->slice.ptr : nullptr; }

}  // extern "C"
