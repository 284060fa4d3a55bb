// libvolym_hip.so: the brush (volym_brush_labels, volym_brush_check, volym_brush_box) beside the kernels it launches (brush_kernels.h).
// A form of relabel.hip's edit: the transition, the launch and the segments' stay on the device are label_edit.hpp's.  Here: the request's
// checks, the stroke's box and segments, and the rule the kernels read.  A blocking set-up call like that edit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "label_edit.hpp"
#include "brush_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_brush_point) == 8 && offsetof(volym_brush_point, flags) == 6, "volym_brush_point has no padding");
static_assert(sizeof(volym_brush) == 2360 && offsetof(volym_brush, flags) == 24 && offsetof(volym_brush, to) == 36 && offsetof(volym_brush, weight) == 292 &&
              offsetof(volym_brush, r2) == 304 && offsetof(volym_brush, n_points) == 308 && offsetof(volym_brush, points) == 312, "volym_brush has no padding");
static_assert(VOLYM_BRUSH_UNCUT == VOLYM_RELABEL_UNCUT && VOLYM_BRUSH_DRY_RUN == VOLYM_RELABEL_DRY_RUN, "the brush's flags carry the edit's values");

// how far the brush reaches along an axis, in texels: the largest m with weight * m * m <= r2 (e - 1 of include/volym_hip.h)
static uint32_t brush_reach(uint32_t r2, uint32_t weight)
{
    const uint64_t q = r2 / weight;
    uint64_t m = static_cast<uint64_t>(std::sqrt(static_cast<double>(q)));
    while (m * m > q) --m;
    while ((m + 1u) * (m + 1u) <= q) ++m;
    return static_cast<uint32_t>(m);
}

// [lo, hi) of the texels of the volume within `reach` of the coordinates p and q on each axis
static void brush_span(const uint16_t p[3], const uint16_t q[3], const uint32_t reach[3], const uint32_t dims[3], uint32_t lo[3], uint32_t hi[3])
{
    for (int a = 0; a < 3; ++a) {
        const uint32_t least = std::min<uint32_t>(p[a], q[a]), most = std::max<uint32_t>(p[a], q[a]);
        lo[a] = least > reach[a] ? least - reach[a] : 0u;
        hi[a] = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(most) + reach[a] + 1u, dims[a]));
    }
}

// the stroke's segments as the kernel reads them (brush_kernels.h BrushSegment): one per point
static void brush_segments(const volym_brush* b, const uint32_t dims[3], std::vector<BrushSegment>& segs)
{
    uint32_t reach[3];
    for (int a = 0; a < 3; ++a) reach[a] = brush_reach(b->r2, b->weight[a]);
    segs.assign(b->n_points, BrushSegment{});
    for (uint32_t i = 0; i < b->n_points; ++i) {
        const volym_brush_point& to = b->points[i];
        const volym_brush_point& from = (i == 0u || (to.flags & VOLYM_BRUSH_LIFT)) ? to : b->points[i - 1u];
        const uint16_t p[3] = {from.x, from.y, from.z}, q[3] = {to.x, to.y, to.z};
        BrushSegment& g = segs[i];
        uint32_t hi[3];
        brush_span(p, q, reach, dims, g.lo, hi);
        uint64_t dd = 0;
        for (int a = 0; a < 3; ++a) {
            g.a[a] = p[a]; g.b[a] = q[a]; g.hi[a] = hi[a] - 1u;              // (a point lies in the volume: hi > lo)
            const int64_t d = static_cast<int64_t>(q[a]) - p[a];
            dd += static_cast<uint64_t>(b->weight[a]) * static_cast<uint64_t>(d * d);
        }
        g.dd = static_cast<uint32_t>(dd);                                     // (< 2^32: include/volym_hip.h)
        const uint64_t r2dd = static_cast<uint64_t>(b->r2) * dd;
        g.r2dd_lo = static_cast<uint32_t>(r2dd); g.r2dd_hi = static_cast<uint32_t>(r2dd >> 32);
    }
}

extern "C" {

int volym_brush_check(const volym_brush* b, const uint32_t dims[3])
{
    if (!b || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(b->box, dims)) return VOLYM_E_INVALID;
    if (b->flags & ~static_cast<uint32_t>(VOLYM_BRUSH_UNCUT | VOLYM_BRUSH_DRY_RUN)) return VOLYM_E_INVALID;
    if (b->min_byte > b->max_byte || b->max_byte > 255u) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a) if (b->weight[a] < 1u || b->weight[a] > VOLYM_DISTANCE_WEIGHT_MAX) return VOLYM_E_INVALID;
    if (b->n_points < 1u || b->n_points > VOLYM_BRUSH_MAX_POINTS) return VOLYM_E_INVALID;
    for (uint32_t i = 0; i < b->n_points; ++i) {
        const volym_brush_point& p = b->points[i];
        if (p.x >= dims[0] || p.y >= dims[1] || p.z >= dims[2]) return VOLYM_E_INVALID;
        if (p.flags & ~static_cast<uint32_t>(VOLYM_BRUSH_LIFT)) return VOLYM_E_INVALID;
    }
    return VOLYM_OK;
}

int volym_brush_box(const volym_brush* b, const uint32_t dims[3], uint32_t box_out[6])
{
    if (!box_out || volym_brush_check(b, dims) != VOLYM_OK) return VOLYM_E_INVALID;
    uint32_t reach[3];
    uint16_t least[3] = {0xffffu, 0xffffu, 0xffffu}, most[3] = {0u, 0u, 0u};
    for (int a = 0; a < 3; ++a) reach[a] = brush_reach(b->r2, b->weight[a]);
    for (uint32_t i = 0; i < b->n_points; ++i) {
        const uint16_t p[3] = {b->points[i].x, b->points[i].y, b->points[i].z};
        for (int a = 0; a < 3; ++a) { least[a] = std::min(least[a], p[a]); most[a] = std::max(most[a], p[a]); }
    }
    uint32_t lo[3], hi[3];
    brush_span(least, most, reach, dims, lo, hi);
    bool empty = false;
    for (int a = 0; a < 3; ++a) {
        box_out[a] = std::max(lo[a], b->box[a]);
        box_out[3 + a] = std::min(hi[a], b->box[3 + a]);
        empty = empty || box_out[a] >= box_out[3 + a];
    }
    if (empty) std::memset(box_out, 0, 6 * sizeof(uint32_t));
    return VOLYM_OK;
}

int volym_brush_labels(volym_ctx* c, const volym_brush* b, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!b) return fail(c, VOLYM_E_INVALID, "volym_brush_labels: NULL request");
    const int ok = editable_state(c, "volym_brush_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_brush_check(b, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_brush_labels: need lo <= hi <= volume size on every axis, known flags, min_byte <= max_byte <= 255, weights in 1..64, "
                                        "1..256 points inside the volume and no point flag but LIFT");
    volym_relabel_result res;
    std::memset(&res, 0, sizeof res);
    uint32_t box[6];
    (void)volym_brush_box(b, dims, box);
    if (box[0] == box[3]) { if (out) *out = res; return VOLYM_OK; }         // the stroke's hull misses the box (or the box is empty)

    HIPCHK(c, hipSetDevice(c->device));
    std::vector<BrushSegment> segs;
    brush_segments(b, dims, segs);
    CallArray<BrushSegment> d_segs;
    int rc = d_segs.upload(c, c->slot0().stream, segs, "brush segments", "volym_brush_labels");
    if (rc != VOLYM_OK) return rc;

    const bool dry = (b->flags & VOLYM_BRUSH_DRY_RUN) != 0u;
    BrushRule rule = {};
    rule.min_byte = b->min_byte; rule.max_byte = b->max_byte;
    rule.store = dry ? 0u : 1u;
    rule.n_segments = static_cast<uint32_t>(segs.size());
    rule.r2 = b->r2;
    for (int a = 0; a < 3; ++a) rule.weight[a] = b->weight[a];
    const LabelEdit edit = {box, b->to, dry, "volym_brush_labels"};
    rc = edit_labels(c, edit, res, [&](hipStream_t stream, dim3 grid, const RelabelOut& o, const LabelTable& to, const CropSlab& s, uint32_t items,
                                       const LabelJournal* journal) {
        launch_edit(c, volym_brush_kernel, volym_brush_journal_kernel, stream, grid, o, to, s, rule, items, journal,
                    edit_density(c, (b->flags & VOLYM_BRUSH_UNCUT) != 0u), d_segs.ptr);
    });
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

}  // extern "C"
