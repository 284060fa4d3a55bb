// The pick pass (gfx950): segment, texel and depth under a pixel, by the rule the picture was made by.  A unit of its own, as
// scene_bytes.hip is: nothing here is instantiated in, or changes, the units of the frame kernels.  It holds the pass's kernel
// (pick_kernels.h), its C ABI (volym_pick_pass, volym_read_picks, volym_pick_device_ptr, volym_pick) and what the context keeps
// for it: its own records, and the rect of the latest pass into them.
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "pick_kernels.h"

static_assert(sizeof(volym_pick_record) == sizeof(uint4), "a pick record is one 16-byte store");

namespace volym {

// one pick march of rect {x0, y0, w, h} (inside the frame, not empty) into `out` (w * h records), enqueued on the slot's stream
// with the slot's frame parameters, tables and -- when it is the one of the current threshold and scene -- distance field
static int launch_pick(volym_ctx* c, FrameSlot& s, const uint32_t rect[4], float alpha_min, void* out)
{
    FrameParams fp = s.fp;
    fp.mc_n = c->mc_n;
    PickArgs a;
    a.vol = c->d_vol;
    a.imp = c->d_imp;
    a.labels = labels_fit(c) ? c->d_labels : nullptr;
    a.labels_bricked = c->labels_bricked ? 1u : 0u;
    a.tables = s.d_tables;
    // the slot's distance field, when it is the one of this frame's threshold and scene (every edit of the scene's bytes and every
    // change of the threshold invalidates df_thr_byte until the next frame rebuilds it in stream order) and fits the kernel's LDS
    const bool table_mode = !(fp.flags & (F_LINEAR | F_GAUSSIAN));
    a.df4 = (table_mode && s.df_thr_byte == s.thr_byte_cull && s.thr_byte_cull == fp.thr_byte && c->mc_n <= 32u) ? s.d_df : nullptr;
    a.out = static_cast<uint4*>(out);
    a.x0 = rect[0]; a.y0 = rect[1]; a.w = rect[2]; a.h = rect[3];
    a.tiles_x = (a.w + 15u) / 16u;
    a.alpha_min = alpha_min;
    const uint32_t grid = a.tiles_x * ((a.h + 15u) / 16u);
    // general: anything the common table-mode march does not carry (look-ahead, colouring, smoothing, trilinear)
    const bool general = !table_mode || (fp.flags & (F_IMP_RENDERING | F_IMP_COLORING)) != 0u;
    if (c->bricked) {
        if (general) hipLaunchKernelGGL((volym_pick_kernel<true, true>), dim3(grid), dim3(256), 0, s.stream, a, fp);
        else hipLaunchKernelGGL((volym_pick_kernel<true, false>), dim3(grid), dim3(256), 0, s.stream, a, fp);
    } else {
        if (general) hipLaunchKernelGGL((volym_pick_kernel<false, true>), dim3(grid), dim3(256), 0, s.stream, a, fp);
        else hipLaunchKernelGGL((volym_pick_kernel<false, false>), dim3(grid), dim3(256), 0, s.stream, a, fp);
    }
    VOLYM_HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

void free_pick(volym_ctx* c)
{
    c->picks.release();
    c->pick_w = c->pick_h = c->pick_x0 = c->pick_y0 = 0;
}

}  // namespace volym

using namespace volym;

extern "C" {

int volym_pick_pass(volym_ctx* c, const uint32_t rect[4], float alpha_min)
{
    if (!c) return VOLYM_E_INVALID;
    if (!(alpha_min >= 0.0f && alpha_min <= 0.95f)) return ctx_fail(c, VOLYM_E_INVALID, "volym_pick_pass: alpha_min must be in [0, 0.95]");
    uint32_t r[4];
    int rc = frame_rect(c, rect, "volym_pick_pass", r);
    if (rc != VOLYM_OK) return rc;
    if (!c->have_vol || !c->have_imp || !c->have_tf) return ctx_fail(c, VOLYM_E_STATE, "volym_pick_pass: set volume, importances and transfer function first");
    if (!c->have_frame) return ctx_fail(c, VOLYM_E_STATE, "volym_pick_pass: call volym_update first");
    FrameSlot& s = c->slot0();
    if (s.fp.nx != c->nx || s.fp.ny != c->ny || s.fp.nz != c->nz || c->inx != c->nx || c->iny != c->ny || c->inz != c->nz)
        return ctx_fail(c, VOLYM_E_STATE, "volym_pick_pass: the volume changed since the last volym_update");
    VOLYM_HIPCHK(c, hipSetDevice(c->device));
    const size_t need = static_cast<size_t>(r[2]) * r[3];
    rc = c->picks.reserve(c, s.stream, need, "pick records");
    if (rc != VOLYM_OK) return rc;
    rc = launch_pick(c, s, r, alpha_min, c->picks.ptr);
    if (rc != VOLYM_OK) return rc;
    c->pick_x0 = r[0]; c->pick_y0 = r[1];
    c->pick_w = r[2]; c->pick_h = r[3];
    c->picks.count = need;
    return VOLYM_OK;
}

int volym_read_picks(volym_ctx* c, volym_pick_record* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_read_picks: NULL output");
    if (c->picks.count == 0u) return ctx_fail(c, VOLYM_E_STATE, "volym_read_picks: no volym_pick_pass yet");
    return c->picks.read(c, c->slot0().stream, out, c->picks.count);
}

void* volym_pick_device_ptr(volym_ctx* c) { return (c && c->picks.count != 0u) ? c->picks.ptr : nullptr; }

int volym_pick(volym_ctx* c, uint32_t x, uint32_t y, float alpha_min, volym_pick_record* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_pick: NULL output");
    const uint32_t rect[4] = {x, y, 1u, 1u};
    const int rc = volym_pick_pass(c, rect, alpha_min);
    return rc != VOLYM_OK ? rc : volym_read_picks(c, out);
}

}  // extern "C"
