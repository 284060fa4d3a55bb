// The pick march and its launcher (gfx950): segment, texel and depth under a pixel, by the rule the picture was made by.
// A unit of its own, as scene_bytes.hip is: nothing here is instantiated in, or changes, the units of the frame kernels.  The entry
// points (volym_pick_pass, volym_read_picks, volym_pick_device_ptr, volym_pick) and the buffer are raymarch.hip's; this unit turns
// one validated request into one kernel launch.
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "pick_kernels.h"

static_assert(sizeof(volym_pick_record) == sizeof(uint4), "a pick record is one 16-byte store");

namespace volym {

int launch_pick(volym_ctx* c, FrameSlot& s, const uint32_t rect[4], float alpha_min, void* out)
{
    FrameParams fp = s.fp;
    fp.mc_n = c->mc_n;
    PickArgs a;
    a.vol = c->d_vol;
    a.imp = c->d_imp;
    // labels whose dimensions differ from the volume's count as absent
    a.labels = (c->d_labels && c->lnx == c->nx && c->lny == c->ny && c->lnz == c->nz) ? c->d_labels : nullptr;
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

}  // namespace volym
