// libvolym_hip.so: the lasso (volym_lasso_labels, volym_lasso_check, volym_lasso_rect, volym_read_lasso_mask) beside the kernels it
// launches (lasso_kernels.h).  A form of relabel.hip's edit: the transition, the launch and the edges' stay on the device are
// label_edit.hpp's.  Here: the request's checks, the mask's rect and plane, and the rule the kernels read.  A blocking set-up call like
// that edit.  The view's builder (volym_lasso_view_from_camera) is host arithmetic in scene.cpp.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "label_edit.hpp"
#include "lasso_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_lasso_view) == 88 && offsetof(volym_lasso_view, width) == 36 && offsetof(volym_lasso_view, height) == 40 &&
              offsetof(volym_lasso_view, scale_log2) == 44 && offsetof(volym_lasso_view, c) == 48 && offsetof(volym_lasso_view, depth) == 72, "volym_lasso_view has no padding");
static_assert(sizeof(volym_lasso_point) == 8 && offsetof(volym_lasso_point, y) == 4, "volym_lasso_point has no padding");
static_assert(sizeof(volym_lasso) == 8576 && offsetof(volym_lasso, flags) == 24 && offsetof(volym_lasso, to) == 36 && offsetof(volym_lasso, n_points) == 292 &&
              offsetof(volym_lasso, view) == 296 && offsetof(volym_lasso, points) == 384, "volym_lasso has no padding");
static_assert(VOLYM_LASSO_UNCUT == VOLYM_RELABEL_UNCUT && VOLYM_LASSO_DRY_RUN == VOLYM_RELABEL_DRY_RUN, "the lasso's flags carry the edit's values");
static_assert((VOLYM_LASSO_OUTSIDE & (VOLYM_RELABEL_UNCUT | VOLYM_RELABEL_IDS | VOLYM_RELABEL_IDS_EXCEPT | VOLYM_RELABEL_DISTANCE | VOLYM_RELABEL_DRY_RUN)) == 0,
              "OUTSIDE is no flag of the edit");

namespace volym {

void free_lasso(volym_ctx* c)
{
    c->lasso_plane.release();
    c->lasso_have = false;
}

}  // namespace volym

// what volym_lasso_rect needs of a request: the polygon and the frame
static bool lasso_polygon_ok(const volym_lasso* l)
{
    if (l->n_points < 3u || l->n_points > VOLYM_LASSO_MAX_POINTS) return false;
    if (l->view.width < 1u || l->view.width > VOLYM_LASSO_MAX_FRAME || l->view.height < 1u || l->view.height > VOLYM_LASSO_MAX_FRAME) return false;
    for (uint32_t i = 0; i < l->n_points; ++i) {
        const volym_lasso_point& p = l->points[i];
        if (p.x < -VOLYM_LASSO_VERTEX_MAX || p.x > VOLYM_LASSO_VERTEX_MAX || p.y < -VOLYM_LASSO_VERTEX_MAX || p.y > VOLYM_LASSO_VERTEX_MAX) return false;
    }
    return true;
}

extern "C" {

int volym_lasso_check(const volym_lasso* l, const uint32_t dims[3])
{
    if (!l || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(l->box, dims)) return VOLYM_E_INVALID;
    if (l->flags & ~static_cast<uint32_t>(VOLYM_LASSO_UNCUT | VOLYM_LASSO_DRY_RUN | VOLYM_LASSO_OUTSIDE)) return VOLYM_E_INVALID;
    if (l->min_byte > l->max_byte || l->max_byte > 255u) return VOLYM_E_INVALID;
    if (!lasso_polygon_ok(l)) return VOLYM_E_INVALID;
    const int64_t c_bound = int64_t(1) << 46;
    for (int r = 0; r < 3; ++r) {
        for (int a = 0; a < 3; ++a) if (l->view.m[r][a] == INT32_MIN) return VOLYM_E_INVALID;
        if (l->view.c[r] <= -c_bound || l->view.c[r] >= c_bound) return VOLYM_E_INVALID;
    }
    if (l->view.depth[0] < 1 || l->view.depth[0] > l->view.depth[1]) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_lasso_rect(const volym_lasso* l, uint32_t rect_out[4])
{
    if (!l || !rect_out || !lasso_polygon_ok(l)) return VOLYM_E_INVALID;
    int32_t x0 = l->points[0].x, y0 = l->points[0].y, x1 = x0, y1 = y0;
    for (uint32_t i = 1; i < l->n_points; ++i) {
        x0 = std::min(x0, l->points[i].x); x1 = std::max(x1, l->points[i].x);
        y0 = std::min(y0, l->points[i].y); y1 = std::max(y1, l->points[i].y);
    }
    // a pixel at the largest x or y of the polygon is never in the mask (the crossing rule is half-open): hi exclusive as it stands
    x0 = std::max(x0, 0); y0 = std::max(y0, 0);
    x1 = std::min<int32_t>(x1, static_cast<int32_t>(l->view.width)); y1 = std::min<int32_t>(y1, static_cast<int32_t>(l->view.height));
    if (x0 >= x1 || y0 >= y1) { std::memset(rect_out, 0, 4 * sizeof(uint32_t)); return VOLYM_OK; }
    rect_out[0] = static_cast<uint32_t>(x0); rect_out[1] = static_cast<uint32_t>(y0); rect_out[2] = static_cast<uint32_t>(x1); rect_out[3] = static_cast<uint32_t>(y1);
    return VOLYM_OK;
}

int volym_read_lasso_mask(volym_ctx* c, uint32_t rect_out[4], uint32_t* words, uint64_t capacity)
{
    if (!c) return VOLYM_E_INVALID;
    if (!rect_out) return fail(c, VOLYM_E_INVALID, "volym_read_lasso_mask: NULL rect");
    if (!c->lasso_have) return fail(c, VOLYM_E_STATE, "volym_read_lasso_mask: no lasso yet (volym_lasso_labels first)");
    std::memcpy(rect_out, c->lasso_rect, sizeof c->lasso_rect);
    if (!words || c->lasso_plane.count == 0u) return VOLYM_OK;
    if (capacity < c->lasso_plane.count) return fail(c, VOLYM_E_INVALID, "volym_read_lasso_mask: the plane has " + std::to_string(c->lasso_plane.count) + " words");
    return c->lasso_plane.read(c, c->slot0().stream, words, c->lasso_plane.count);
}

int volym_lasso_labels(volym_ctx* c, const volym_lasso* l, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!l) return fail(c, VOLYM_E_INVALID, "volym_lasso_labels: NULL request");
    const int ok = editable_state(c, "volym_lasso_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_lasso_check(l, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_lasso_labels: need lo <= hi <= volume size on every axis, known flags, min_byte <= max_byte <= 255, 3..1024 vertices within "
                                        "2^20 of the origin, |m| < 2^31, |c| < 2^46, 1 <= depth[0] <= depth[1] and a frame of 1..16384 pixels a side");
    volym_relabel_result res;
    std::memset(&res, 0, sizeof res);
    uint32_t rect[4];
    (void)volym_lasso_rect(l, rect);
    const uint32_t rect_w = rect[2] - rect[0], rect_h = rect[3] - rect[1], stride = (rect_w + 31u) / 32u;
    const size_t words = static_cast<size_t>(stride) * rect_h;

    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    std::vector<LassoEdge> edges;                                           // (outlives its copy: declared in front of d_edges)
    CallArray<LassoEdge> d_edges;
    if (words != 0u) {
        // the polygon's bit plane, in stream order in front of the edit kernel
        int rc = c->lasso_plane.reserve(c, stream, words, "lasso plane");
        if (rc != VOLYM_OK) { c->lasso_have = false; return rc; }
        edges.resize(l->n_points);
        for (uint32_t i = 0; i < l->n_points; ++i) {
            const volym_lasso_point& p = l->points[i];
            const volym_lasso_point& q = l->points[i + 1u == l->n_points ? 0u : i + 1u];
            edges[i] = LassoEdge{p.x, p.y, q.x, q.y};
        }
        rc = d_edges.upload(c, stream, edges, "lasso edges", "volym_lasso_labels");
        if (rc != VOLYM_OK) { c->lasso_have = false; return rc; }
        const uint64_t waves = static_cast<uint64_t>((rect_w + 63u) / 64u) * rect_h;
        hipLaunchKernelGGL(volym_lasso_raster_kernel, dim3(static_cast<uint32_t>((waves + 3u) / 4u)), dim3(256), 0, stream, c->lasso_plane.ptr, d_edges.ptr,
                           l->n_points, rect[0], rect[1], rect[2], rect[3], stride);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { c->lasso_have = false; return fail(c, VOLYM_E_HIP, std::string("volym_lasso_labels: ") + hipGetErrorString(e)); }
    }
    std::memcpy(c->lasso_rect, rect, sizeof rect);
    c->lasso_plane.count = words;
    c->lasso_have = true;

    const bool dry = (l->flags & VOLYM_LASSO_DRY_RUN) != 0u, outside = (l->flags & VOLYM_LASSO_OUTSIDE) != 0u;
    int rc = VOLYM_OK;
    if (words != 0u || outside) {                                           // (an empty rect without OUTSIDE selects nothing)
        LassoRule rule = {};
        for (int r = 0; r < 3; ++r) { rule.c[r] = l->view.c[r]; for (int a = 0; a < 3; ++a) rule.m[r][a] = l->view.m[r][a]; }
        rule.depth[0] = l->view.depth[0]; rule.depth[1] = l->view.depth[1];
        std::memcpy(rule.rect, rect, sizeof rect);
        rule.stride = stride;
        rule.min_byte = l->min_byte; rule.max_byte = l->max_byte;
        rule.store = dry ? 0u : 1u;
        rule.outside = outside ? 1u : 0u;
        const uint32_t* plane = words != 0u ? c->lasso_plane.ptr : nullptr;
        const LabelEdit edit = {l->box, l->to, dry, "volym_lasso_labels"};
        rc = edit_labels(c, edit, res, [&](hipStream_t s0, dim3 grid, const RelabelOut& o, const LabelTable& to, const CropSlab& s, uint32_t items,
                                           const LabelJournal* journal) {
            launch_edit(c, volym_lasso_kernel, volym_lasso_journal_kernel, s0, grid, o, to, s, rule, items, journal,
                        edit_density(c, (l->flags & VOLYM_LASSO_UNCUT) != 0u), plane);
        });
    }
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

}  // extern "C"
