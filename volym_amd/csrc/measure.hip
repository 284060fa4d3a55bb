// libvolym_hip.so: the measure pass (volym_measure_pass, volym_read_measure, volym_measure_device_ptr, volym_measure_check) beside the
// kernels it launches (measure_kernels.h).  It only reads the scene's bytes, over the walk it shares with the rewrites (scene_bytes.hpp:
// make_crop_slab, stream_grid), and is enqueue-only on slot 0's stream: it writes the context's own 36 KB result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

#include "scene_bytes.hpp"
#include "measure_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_measure) == 284 && offsetof(volym_measure, flags) == 24 && offsetof(volym_measure, group) == 28, "volym_measure has no padding");
static_assert(sizeof(volym_segment_stats) == 80 && offsetof(volym_segment_stats, box) == 48 && offsetof(volym_segment_stats, min) == 72 &&
              offsetof(volym_segment_stats, max) == 76, "volym_segment_stats has no padding");
static_assert(sizeof(volym_measurement) == 36864 && offsetof(volym_measurement, hist) == 20480, "volym_measurement has no padding");

void volym::free_measure(volym_ctx* c) { c->measure.release(); }

extern "C" {

int volym_measure_check(const volym_measure* m, const uint32_t dims[3])
{
    if (!m || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(m->box, dims)) return VOLYM_E_INVALID;
    if (m->flags & ~static_cast<uint32_t>(VOLYM_MEASURE_UNCUT)) return VOLYM_E_INVALID;
    for (int l = 0; l < 256; ++l) if (m->group[l] >= VOLYM_MEASURE_GROUPS && m->group[l] != VOLYM_MEASURE_NO_GROUP) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_measure_pass(volym_ctx* c, const volym_measure* m)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_measure_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_measure whole = {};                    // every label in group 0, no flags
    whole_volume_box(dims, whole.box);
    if (!m) m = &whole;
    if (volym_measure_check(m, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_measure_pass: need lo <= hi <= volume size on every axis, known flags, and groups below 8 or VOLYM_MEASURE_NO_GROUP");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_measure_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;       // where pick, slice and projection passes go: ordered with them and with itself
    // (a set-up step, once: the one blocking path of a pass)
    rc = c->measure.reserve(c, stream, 1, "measurement");
    if (rc != VOLYM_OK) return rc;
    const MeasureOut out = {c->measure.ptr->seg, reinterpret_cast<unsigned long long*>(&c->measure.ptr->hist[0][0])};
    hipLaunchKernelGGL(volym_measure_init_kernel, dim3(1), dim3(256), 0, stream, out);
    HIPCHK(c, hipGetLastError());
    c->measure.count = 1;

    // the texels that can be in: the request's box, cut to the crop box unless UNCUT
    const bool uncut = (m->flags & VOLYM_MEASURE_UNCUT) != 0u;
    uint32_t box[6];
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        box[a] = uncut ? m->box[a] : std::max(m->box[a], c->crop_lo[a]);
        box[3 + a] = uncut ? m->box[3 + a] : std::min(m->box[3 + a], c->crop_hi[a]);
        empty = empty || box[a] >= box[3 + a];
    }
    if (empty) return VOLYM_OK;                         // 256 empty records
    CropSlab s;
    const uint64_t items = make_crop_slab(c, c->bricked, box, nullptr, s);
    // keep = inside the slab itself: a bricked chunk holds texels of the crop box beside the request's, which must not count
    for (int a = 0; a < 3; ++a) { s.box_lo[a] = box[a]; s.box_hi[a] = box[3 + a]; }
    if (uncut) { s.planes = 0u; s.pn[0] = s.pn[1] = s.pn[2] = s.pd = 0; }
    const bool masked = !uncut && with_labels && mask_active(c);
    LabelTable group, mask = {};
    std::memcpy(group.v, m->group, 256);
    for (int l = 0; l < 256; ++l) mask.v[l] = c->seg_hidden[l] ? 0u : 1u;
    // Eight items per lane before the grid grows: every workgroup ends in up to 2048 + 14 * 256 global atomics on the same 36 KB, and
    // with one item per lane (2048 workgroups at 256^3) that flush was the whole cost: 291 us against 118 us with eight; sixteen and
    // thirty-two leave too few workgroups for the latency of a lane's loads (123 and 180 us; profiles/measure.txt).  And at most
    // MEASURE_ITEMS_PER_LANE items per lane, whatever the device's CU count: the widths of measure_kernels.h rest on it.
    const uint64_t floor_grid = (items + 256ull * MEASURE_ITEMS_PER_LANE - 1u) / (256ull * MEASURE_ITEMS_PER_LANE);
    const dim3 grid(static_cast<uint32_t>(std::max<uint64_t>(stream_grid(c, (items + 7u) / 8u), floor_grid)));
    const uint4* vol = reinterpret_cast<const uint4*>(uncut && c->d_vol0 ? c->d_vol0 : c->d_vol);
    const uint4* labels = with_labels ? reinterpret_cast<const uint4*>(c->d_labels) : nullptr;
    const auto kernel = with_labels ? volym_measure_kernel<true> : volym_measure_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, vol, labels, out, group, mask, s, c->nx, c->ny, c->nz, c->bricked ? 1u : 0u, masked ? 1u : 0u,
                       static_cast<uint32_t>(items));
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_measure(volym_ctx* c, struct volym_measurement* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_measure: NULL output");
    if (c->measure.count == 0u) return fail(c, VOLYM_E_STATE, "volym_read_measure: no volym_measure_pass since the volume was set");
    return c->measure.read(c, c->slot0().stream, out, 1);
}

void* volym_measure_device_ptr(volym_ctx* c) { return (c && c->measure.count != 0u) ? c->measure.ptr : nullptr; }

}  // extern "C"
