// libvolym_hip.so: context, frame loop and their C ABI (include/volym_hip.h) over the gfx950 kernels.  The bytes of the scene
// (volume, labels, importances, crop box, segment visibility, macro cells) and their C ABI are scene_bytes.hip; the read-only
// passes over frame and scene (pick, outline, slice, projection, surface, components, distance) are units of their own, each with its C ABI.
// Replaces the reference's gpu_context.rs / gpu_resources/* / demos/pipeline.rs for the
// ray-march path; citations are file:line under /root/reference/.
//
// Threading contract: volym_update and volym_compute_pass only enqueue -- no hipMalloc, no
// hipFree, no stream synchronisation on their path.  Everything that allocates or waits lives in the set-up calls
// (volym_create, volym_set_*, volym_set_option, volym_set_shard) and in the explicitly blocking ones (volym_sync,
// volym_settle, volym_read_*, volym_stats_pass, volym_time_*).  The cost feedback of the work lists runs on a thread
// of its own (below, "cost feedback").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <queue>
#include <string>
#include <vector>

#include "context.hpp"
#include "worklist.hpp"
#include "raymarch_kernels.h"
#include "raymarch_pq.h"
#include "raymarch_pool.h"
#include "blit.h"

// the common instantiation lives in raymarch_common.hip (its own scheduler flag)
namespace volym {
extern template __global__ void volym_raymarch_pq_kernel<true, false, false, 4, false, false, false, PQ_WAVES, 0, false, true>(
    const uint8_t* __restrict__, const uint8_t* __restrict__, const FrameTables* __restrict__, const uint8_t* __restrict__, const uint2* __restrict__, uint32_t,
    uint16_t* __restrict__, uint32_t* __restrict__, uint32_t* __restrict__, float4* __restrict__, Counters* __restrict__, uint4* __restrict__, const FrameParams);
extern template __global__ void volym_raymarch_cube256_kernel<true, false, false, 4, false, false, false, PQ_WAVES, 0, false, true>(
    const uint8_t* __restrict__, const uint8_t* __restrict__, const FrameTables* __restrict__, const uint8_t* __restrict__, const uint2* __restrict__, uint32_t,
    uint16_t* __restrict__, uint32_t* __restrict__, uint32_t* __restrict__, float4* __restrict__, Counters* __restrict__, uint4* __restrict__, const FrameParams);
}  // namespace volym

using namespace volym;

static_assert(sizeof(volym_camera_uniforms) == 208, "CameraUniforms is 208 bytes (src/gpu_resources/camera.rs:56-64)");
static_assert(sizeof(volym_parameter_uniforms) == 32, "ParameterUniforms is 32 bytes (src/gpu_resources/parameters.rs:55-66)");

// cos/sin of (s/8) * 2 * 3.14159 for s = 0..7 (wgsl:99-103), f32
static const float k_cone_cos[8] = {0x1p+0f, 0x1.6a09f6p-1f, 0x1.54442ep-20f, -0x1.6a09bap-1f,
                                    -0x1p+0f, -0x1.6a0a32p-1f, -0x1.fe6644p-19f, 0x1.6a097ep-1f};
static const float k_cone_sin[8] = {0x0p+0f, 0x1.6a09d8p-1f, 0x1p+0f, 0x1.6a0a14p-1f,
                                    0x1.54442ep-19f, -0x1.6a099cp-1f, -0x1p+0f, -0x1.6a0a5p-1f};

static thread_local std::string g_create_error;

int volym::ctx_fail(volym_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}
static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static void recompute_shard(volym_ctx* c)
{
    c->n_local = c->n_tiles > c->rank ? (c->n_tiles - c->rank + c->world - 1) / c->world : 0;
    c->shard_tiles = (c->n_tiles + c->world - 1) / c->world;   // equal-sized shards, padded
}

static ShardGrid shard_grid(const volym_ctx* c) { return ShardGrid{c->W, c->H, c->tiles_x, c->tiles_y, c->rank, c->world, c->n_local}; }

static uint32_t max_grid(const volym_ctx* c) { return static_cast<uint32_t>(c->n_cus) * c->wgs_per_cu; }

// Does a plain frame with these flags run the ray pool (variant 3, raymarch_pool.h)?  The common instantiation only: nearest
// filter, no smoothing, opacity on, no importance mode; every other flag set runs variant 2.
static bool frame_uses_pool(const volym_ctx* c, uint32_t flags)
{
    return c->kernel_variant == 3 && !(flags & (F_LINEAR | F_GAUSSIAN | F_IMP_COLORING | F_IMP_RENDERING)) && (flags & F_OPACITY);
}

// ---- host-side table construction (EXACT arithmetic, same recipe as the device) --------------
static void host_texel_linear(float u, int n, int& i0, int& i1, float& w)
{
    const float x = u * static_cast<float>(n) - 0.5f;
    float fl = std::floor(x);
    w = x - fl;
    if (!(fl >= -2.0f)) fl = -2.0f;
    if (fl > static_cast<float>(n)) fl = static_cast<float>(n);
    const int i = static_cast<int>(fl);
    i0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    i1 = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : i + 1);
}

static void build_tables(volym_ctx* c, FrameTables& t, float alpha_y)
{
    const int n = static_cast<int>(c->tf_n);
    for (int b = 0; b < 256; ++b) {
        t.rho[b] = static_cast<float>(b) / 255.0f;
        const uint8_t* q = c->lut + 4 * (b < n ? b : n - 1);
        t.lut_f[b] = make_float4(static_cast<float>(q[0]) / 255.0f, static_cast<float>(q[1]) / 255.0f,
                                 static_cast<float>(q[2]) / 255.0f, static_cast<float>(q[3]) / 255.0f);
    }
    for (int b = 0; b < 256; ++b) {
        int i0, i1;
        float w;
        host_texel_linear(t.rho[b], n, i0, i1, w);   // wgsl:297-302: rho is the coordinate
        const float4 a = t.lut_f[i0], bb = t.lut_f[i1];
        const float iw = 1.0f - w;
        const float A = a.w * iw + bb.w * w;
        t.tf_tab[b] = make_float4(a.x * iw + bb.x * w, a.y * iw + bb.y * w, a.z * iw + bb.z * w,
                                  1.0f - wgsl_pow(1.0f - A, alpha_y));   // wgsl:314
        t.ic_alpha[b] = 1.0f - wgsl_pow(1.0f - t.rho[b], alpha_y);       // wgsl:83-84, :314
    }
}// ---- exact culling inputs (raymarch_pq.h): hulls of the projected unit cube and of the projected AABB of the
// occupied macro cells, in pixel coordinates, plus the AABB itself.  Double precision on the host; the kernel
// applies a 1.5 pixel margin, far above the f32 noise of the per-pixel ray set-up it stands in for. ----
namespace {
struct P2 { double x, y; };

bool invert4d(const double m[16], double inv[16])
{
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int col = 0; col < 4; ++col) { a[r][col] = m[col * 4 + r]; a[r][4 + col] = r == col ? 1.0 : 0.0; }
    for (int i = 0; i < 4; ++i) {
        int piv = i;
        for (int r = i + 1; r < 4; ++r) if (std::fabs(a[r][i]) > std::fabs(a[piv][i])) piv = r;
        if (std::fabs(a[piv][i]) < 1e-300) return false;
        if (piv != i) for (int k = 0; k < 8; ++k) std::swap(a[i][k], a[piv][k]);
        const double d = a[i][i];
        for (int k = 0; k < 8; ++k) a[i][k] /= d;
        for (int r = 0; r < 4; ++r) if (r != i) { const double f = a[r][i]; if (f != 0.0) for (int k = 0; k < 8; ++k) a[r][k] -= f * a[i][k]; }
    }
    for (int r = 0; r < 4; ++r) for (int col = 0; col < 4; ++col) inv[col * 4 + r] = a[r][4 + col];
    return true;
}

// convex hull (monotone chain) of <= 8 points -> edges (a, b, c, 1) with |(a,b)| = 1, inside >= 0
bool hull_edges(const P2* pts, int n, float out[8][4])
{
    std::vector<P2> p(pts, pts + n);
    std::sort(p.begin(), p.end(), [](const P2& u, const P2& v) { return u.x < v.x || (u.x == v.x && u.y < v.y); });
    auto cross = [](const P2& o, const P2& u, const P2& v) { return (u.x - o.x) * (v.y - o.y) - (u.y - o.y) * (v.x - o.x); };
    std::vector<P2> h(2 * p.size());
    int k = 0;
    for (size_t i = 0; i < p.size(); ++i) { while (k >= 2 && cross(h[k - 2], h[k - 1], p[i]) <= 0) --k; h[k++] = p[i]; }
    for (size_t i = p.size() - 1, t = k + 1; i > 0; --i) { while (k >= static_cast<int>(t) && cross(h[k - 2], h[k - 1], p[i - 1]) <= 0) --k; h[k++] = p[i - 1]; }
    const int m = k - 1;                          // closed polygon, last == first
    for (int e = 0; e < 8; ++e) out[e][0] = out[e][1] = out[e][2] = out[e][3] = 0.0f;
    if (m < 3 || m > 8) return false;
    double cx = 0, cy = 0;
    for (int i = 0; i < m; ++i) { cx += h[i].x; cy += h[i].y; }
    cx /= m; cy /= m;
    for (int i = 0; i < m; ++i) {
        const P2 &u = h[i], &v = h[(i + 1) % m];
        double a = -(v.y - u.y), b = v.x - u.x;
        const double len = std::sqrt(a * a + b * b);
        if (len < 1e-9) return false;
        a /= len; b /= len;
        double cc = -(a * u.x + b * u.y);
        if (a * cx + b * cy + cc < 0) { a = -a; b = -b; cc = -cc; }
        out[i][0] = static_cast<float>(a); out[i][1] = static_cast<float>(b); out[i][2] = static_cast<float>(cc); out[i][3] = 1.0f;
    }
    return true;
}

// Is camera_position the centre of projection of inverse_view_proj?  ("a consistent eye".)  The shader's ray of pixel n
// (in NDC) starts at the eye E and passes through N = unproject(n, z = 0), so its points are X = (1 - s) E + s N, and in clip space
// (M = inverse_view_proj^-1, affine in X) clip(X) = (1 - s) e + s w_N (n, z, 1) with e = clip(E), w_N = clip(N).w.  The hulls and the
// cells' rectangles say where X projects: ndc(X) - n = (1 - s) (e.xy - n e.w) / w_X, and with s = (w_X - e.w) / (w_N - e.w)
//     |ndc(X) - n| <= (|e.xy| + |e.w|) |w_N / w_X - 1| / (w_N - |e.w|)      for |n| <= 1.
// For a box whose corners all have w >= w_min > |e.w| the middle factor is at most max(1, w_N / w_min - 1): 1 for everything beyond
// the near plane, more only for a box between the eye and that plane.  e = 0 for the centre of projection itself.
struct ViewCheck {
    double M[16];            // world -> clip, column-major
    double e[4];             // clip(camera_position)
    double wn_lo, wn_hi;     // range of w_N over the frame
    double scale;            // |M's w row|_1: what a clip w is small against
};

bool view_check(const float (*ivp_f)[4], const float eye[3], ViewCheck& v)
{
    double ivp[16];
    for (int i = 0; i < 16; ++i) ivp[i] = (&ivp_f[0][0])[i];
    for (int i = 0; i < 16; ++i) if (!std::isfinite(ivp[i])) return false;
    if (!std::isfinite(eye[0]) || !std::isfinite(eye[1]) || !std::isfinite(eye[2])) return false;
    if (!invert4d(ivp, v.M)) return false;
    for (int r = 0; r < 4; ++r) v.e[r] = v.M[0 * 4 + r] * eye[0] + v.M[1 * 4 + r] * eye[1] + v.M[2 * 4 + r] * eye[2] + v.M[3 * 4 + r];
    v.scale = std::fabs(v.M[3]) + std::fabs(v.M[7]) + std::fabs(v.M[11]) + std::fabs(v.M[15]);
    // w_N = 1 / (inverse_view_proj (n, 0, 1)).w, affine in n under the division: its range is taken at the frame's corners
    v.wn_lo = INFINITY; v.wn_hi = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double wp = ivp[0 * 4 + 3] * ((k & 1) ? 1.0 : -1.0) + ivp[1 * 4 + 3] * ((k & 2) ? 1.0 : -1.0) + ivp[3 * 4 + 3];
        if (!(wp > 0.0) || !std::isfinite(1.0 / wp)) return false;     // a near plane that is not in front of the centre: not a view this code reasons about
        v.wn_lo = std::min(v.wn_lo, 1.0 / wp); v.wn_hi = std::max(v.wn_hi, 1.0 / wp);
    }
    return std::isfinite(v.scale) && std::isfinite(v.e[0]) && std::isfinite(v.e[1]) && std::isfinite(v.e[3]);
}

// The most pixels by which a point with clip w >= w_min on a ray of the frame can project away from the ray's own pixel
// (w_min <= 0: any point beyond the near plane); +inf where the bound does not hold
double view_eye_displacement(const ViewCheck& v, uint32_t W, uint32_t H, double w_min)
{
    const double ew = std::fabs(v.e[3]);
    if (!(ew < v.wn_lo)) return INFINITY;
    double g = 1.0;
    if (w_min > 0.0) {
        if (!(ew < w_min)) return INFINITY;
        g = std::max(1.0, v.wn_hi / w_min - 1.0);
    }
    const double k = g / (v.wn_lo - ew);
    return std::max((std::fabs(v.e[0]) + ew) * k * 0.5 * W, (std::fabs(v.e[1]) + ew) * k * 0.5 * H);
}
}  // namespace

extern "C" int volym_view_eye_displacement(const volym_camera_uniforms* camera, uint32_t W, uint32_t H, double w_min, double* pixels)
{
    if (!camera || !pixels || W == 0 || H == 0 || !(w_min == w_min)) return VOLYM_E_INVALID;
    ViewCheck v;
    if (!view_check(camera->inverse_view_proj, camera->camera_position, v)) return VOLYM_E_INVALID;
    *pixels = view_eye_displacement(v, W, H, w_min);
    return VOLYM_OK;
}

static void compute_culling(const volym_ctx* c, FrameSlot& s)
{
    FrameParams& fp = s.fp;
    fp.cull = 0;
    std::memset(fp.hull, 0, sizeof fp.hull);
    // variant 3's lattice rectangle: the whole frame unless the hull of the occupied cells says less (below)
    fp.rect[0] = 0; fp.rect[1] = 0;
    fp.rect[2] = (c->W + PL_SBW - 1u) / PL_SBW * PL_SBW; fp.rect[3] = (c->H + PL_SBH - 1u) / PL_SBH * PL_SBH;
    s.hull_dirty = false;
    s.mask_wanted = false;
    if (!c->culling) return;
    // AABB of the occupied cells (per threshold byte, computed when the volume was set), grown by what a sample may
    // reach beyond its own position
    const int* h_aabb = c->aabb_tab[std::min(s.thr_byte_cull, 256u)];
    const bool none = h_aabb[3] < h_aabb[0];
    if (none) fp.cull |= CULL_NOTHING_DENSE;
    double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const double margin = 1.0e-4 + ((fp.flags & F_GAUSSIAN) ? 0.0101 : 0.0);   // smoothing taps sit up to 2*0.005 along the ray (wgsl:53-60)
    if (!none) {
        for (int i = 0; i < 3; ++i) {
            lo[i] = static_cast<double>(h_aabb[i]) / c->mc_n - margin;
            hi[i] = static_cast<double>(h_aabb[3 + i] + 1) / c->mc_n + margin;
            fp.aabb_lo[i] = static_cast<float>(lo[i]);
            fp.aabb_hi[i] = static_cast<float>(hi[i]);
        }
        fp.cull |= CULL_AABB;
    }
    // world -> clip as the exact inverse of the matrix the rays are generated from
    ViewCheck view;
    if (!view_check(c->cam_copy.inverse_view_proj, fp.eye, view)) return;
    const double* M = view.M;
    const double scale = view.scale;
    auto clip = [&](double x, double y, double z, double out[4]) {
        for (int r = 0; r < 4; ++r) out[r] = M[0 * 4 + r] * x + M[1 * 4 + r] * y + M[2 * 4 + r] * z + M[3 * 4 + r];
    };
    // the eye must be the centre of projection of that matrix (clip x, y and w all 0), otherwise the hulls say nothing about the
    // rays: no point beyond the near plane may project further than VOLYM_VIEW_EYE_SLACK_PIXELS from the pixel of its ray
    if (!(view_eye_displacement(view, c->W, c->H, 0.0) <= VOLYM_VIEW_EYE_SLACK_PIXELS)) return;
    double bb[4] = {0, 0, 0, 0};      // bounding rectangle of the last projected box
    auto project_box = [&](const double blo[3], const double bhi[3], float out[8][4]) -> bool {
        P2 pts[8];
        double w_min = INFINITY;
        for (int k = 0; k < 8; ++k) {
            double q[4];
            clip((k & 1) ? bhi[0] : blo[0], (k & 2) ? bhi[1] : blo[1], (k & 4) ? bhi[2] : blo[2], q);
            if (!(q[3] > 1e-3 * scale)) return false;       // a corner at or behind the eye plane: no hull
            w_min = std::min(w_min, q[3]);
            pts[k].x = (q[0] / q[3] + 1.0) * 0.5 * c->W;     // wgsl:221-229 inverted: pixel = (ndc + 1)/2 * W
            pts[k].y = (1.0 - q[1] / q[3]) * 0.5 * c->H;
            if (!std::isfinite(pts[k].x) || !std::isfinite(pts[k].y)) return false;
            bb[0] = k ? std::min(bb[0], pts[k].x) : pts[k].x; bb[1] = k ? std::min(bb[1], pts[k].y) : pts[k].y;
            bb[2] = k ? std::max(bb[2], pts[k].x) : pts[k].x; bb[3] = k ? std::max(bb[3], pts[k].y) : pts[k].y;
        }
        // a box between the eye and the near plane magnifies what the eye is off by: the same bound with this box's nearest corner
        if (!(view_eye_displacement(view, c->W, c->H, w_min) <= VOLYM_VIEW_EYE_SLACK_PIXELS)) return false;
        return hull_edges(pts, 8, out);
    };
    const double c0[3] = {0, 0, 0}, c1[3] = {1, 1, 1};
    if (project_box(c0, c1, fp.hull[0])) fp.cull |= CULL_CUBE_HULL;
    if (!none && project_box(lo, hi, fp.hull[1])) {
        fp.cull |= CULL_OBJ_HULL;
        // every pixel outside the hull by more than its 1.5 pixel margin is constant: so is every pixel outside the hull's bounding
        // rectangle grown by 3 pixels, rounded outwards to whole superblocks
        const double x0 = std::max(0.0, std::floor((bb[0] - 3.0) / PL_SBW) * PL_SBW), y0 = std::max(0.0, std::floor((bb[1] - 3.0) / PL_SBH) * PL_SBH);
        const double x1 = std::min(static_cast<double>(fp.rect[2]), std::ceil((bb[2] + 3.0) / PL_SBW) * PL_SBW), y1 = std::min(static_cast<double>(fp.rect[3]), std::ceil((bb[3] + 3.0) / PL_SBH) * PL_SBH);
        if (x1 > x0 && y1 > y0) { fp.rect[0] = static_cast<uint32_t>(x0); fp.rect[1] = static_cast<uint32_t>(y0); fp.rect[2] = static_cast<uint32_t>(x1); fp.rect[3] = static_cast<uint32_t>(y1); }
        else { fp.rect[0] = fp.rect[1] = fp.rect[2] = fp.rect[3] = 0; }       // the object is off screen
    }
    if (none) { fp.rect[0] = fp.rect[1] = fp.rect[2] = fp.rect[3] = 0; }
    // the per-tile mask of the occupied cells' projections (volym_tile_mask_kernel): its cells lie inside the AABB whose
    // corners were all found in front of the eye, so their corners are too
    fp.mask_t8x = c->tiles_x * 2u;
    s.mask_margin = static_cast<float>(margin);
    for (int i = 0; i < 16; ++i) s.mask_clip[i] = static_cast<float>(M[i]);
    s.mask_wanted = (fp.cull & CULL_OBJ_HULL) != 0u && c->tile_mask && c->tile_mask_words != 0u;
}
// ================================================================================================================
// Work lists and their cost feedback (variant 2): the thread and the capture.  What list is dealt from what costs is the
// scheduler's business (worklist.hpp); this unit runs it.
//
// A launch can be asked to report a counted cost per list entry ("capture"): the costs are copied to pinned host
// memory on a second stream, and a feedback THREAD -- never the caller -- turns them into the next list (deal_list, or
// trim_list for a standing view) and uploads it.  The caller's volym_compute_pass only looks at an atomic flag: when a new
// list is ready it switches to it between two launches.  A moving camera simply keeps the feedback running (one capture
// in flight at a time).
// ================================================================================================================

static void feedback_thread(const volym_ctx* c, FrameSlot* sp)
{
    FrameSlot& s = *sp;
    (void)hipSetDevice(c->device);
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(s.fb_mu);
            s.fb_cv.wait(lk, [&] { const int st = s.fb_state.load(std::memory_order_acquire); return st == FrameSlot::FB_CAPTURED || st == FrameSlot::FB_QUIT; });
        }
        if (s.fb_state.load(std::memory_order_acquire) == FrameSlot::FB_QUIT) return;
        FbJob& job = s.fb_job;
        job.error.clear();
        auto now_us = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        job.t_us[1] = now_us();
        hipError_t e = hipEventSynchronize(s.ev_cost);            // the captured launch and its cost copy are done
        job.t_us[2] = now_us();
        const int next = job.list ^ 1;
        if (e == hipSuccess) {
            // A list dealt for this very view from whole-entry costs is not dealt again (its split tiles report estimates): it is
            // re-balanced from the workgroups' measured times, job.set.trim_rounds times.
            const WorkList& ran = s.lists[job.list];
            const bool same_view = s.view_serial.load(std::memory_order_relaxed) == job.launch.view_serial && ran.view_serial == job.launch.view_serial;
            bool trimmed = false;
            if (same_view && ran.trimmable && ran.trim_round < job.set.trim_rounds)
                trimmed = trim_list(job.set, job.launch, s.list_capacity, ran, reinterpret_cast<const uint32_t*>(s.h_cost_pinned + ((job.n_entries + 1u) & ~1u)), s.lists[next]);
            job.t_us[3] = now_us();
            if (!trimmed) {
                costs_to_items(ran, s.h_cost_pinned, job.n_entries, s.item_cost);
                job.t_us[3] = now_us();
                const bool moving = s.view_serial.load(std::memory_order_relaxed) != job.launch.view_serial;    // (a second load: has it moved by now?)
                deal_list(shard_grid(c), job.set, job.launch, moving, s.item_cost, s.item_is_dp, c->geometric, s.lists[next]);
            }
            job.t_us[4] = now_us();
            if (s.lists[next].entries.size() > s.list_capacity) {
                job.error = "work list larger than its buffers";    // cannot happen: capacity is the worst case
            } else {
                list_to_device_form(shard_grid(c), s.lists[next].entries, s.h_list_pinned);
                // every launch that read d_list[next] finished before the captured launch did (same stream, in order)
                e = hipMemcpyAsync(s.d_list[next], s.h_list_pinned, s.lists[next].entries.size() * 2u * sizeof(uint32_t), hipMemcpyHostToDevice, s.copy_stream);
                if (e == hipSuccess) e = hipEventRecord(s.ev_list, s.copy_stream);
                if (e == hipSuccess) e = hipEventSynchronize(s.ev_list);
            }
        }
        if (e != hipSuccess) job.error = std::string("cost feedback: ") + hipGetErrorString(e);
        job.t_us[5] = now_us();
        {
            // under the mutex: a caller in feedback_quiesce that has just found the state CAPTURED must be inside wait() before this
            // store and its notification happen, or it would sleep through them
            std::lock_guard<std::mutex> lk(s.fb_mu);
            s.fb_state.store(FrameSlot::FB_READY, std::memory_order_release);
        }
        s.fb_cv.notify_all();
    }
}

// caller side: adopt a finished list (never blocks)
static void feedback_poll(FrameSlot& s)
{
    if (s.fb_state.load(std::memory_order_acquire) != FrameSlot::FB_READY) return;
    if (s.fb_job.error.empty()) s.cur = s.fb_job.list ^ 1;
    s.fb_state.store(FrameSlot::FB_IDLE, std::memory_order_release);
}

// caller side, blocking (set-up calls, volym_settle): wait for a job in flight and adopt its list
static void feedback_quiesce(FrameSlot& s)
{
    if (s.fb_state.load(std::memory_order_acquire) == FrameSlot::FB_CAPTURED) {
        std::unique_lock<std::mutex> lk(s.fb_mu);
        s.fb_cv.wait(lk, [&] { return s.fb_state.load(std::memory_order_acquire) != FrameSlot::FB_CAPTURED; });
    }
    feedback_poll(s);
}

// Before a set-up call rewrites or frees what the slots share (the volume, the importances, the macro cells, the shard and its
// geometric list): the feedback of EVERY slot at rest, and EVERY slot's stream idle -- with two frames in flight, the frames
// of either slot may still read it.
int volym::quiesce_slots(volym_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < c->n_slots(); ++i) {
        feedback_quiesce(*c->slots[i]);
        HIPCHK(c, hipStreamSynchronize(c->slots[i]->stream));
    }
    return VOLYM_OK;
}

// The slot's lists in geometric order, no costs (the context's geometric list is current; the slot is at rest).
static int reset_slot_lists(volym_ctx* c, FrameSlot& s)
{
    // worst case: every 8x8 item split into four quarters, plus padding to a multiple of the grid
    const size_t need = static_cast<size_t>(c->n_local) * 16u + 2u * static_cast<size_t>(c->n_cus) * 8u + 64u;
    if (need > s.list_capacity) {
        for (int i = 0; i < 2; ++i) { if (s.d_list[i]) (void)hipFree(s.d_list[i]); s.d_list[i] = nullptr; }
        if (s.d_cost) (void)hipFree(s.d_cost);
        if (s.h_list_pinned) (void)hipHostFree(s.h_list_pinned);
        if (s.h_cost_pinned) (void)hipHostFree(s.h_cost_pinned);
        s.d_cost = nullptr; s.h_list_pinned = nullptr; s.h_cost_pinned = nullptr; s.list_capacity = 0;
        hipError_t e = hipMalloc(&s.d_list[0], need * 2u * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&s.d_list[1], need * 2u * sizeof(uint32_t));
        // + the times of the captured launch: a u32 per wave and per workgroup (raymarch_pq.h wg_time)
        const size_t cost_bytes = (need + 2u) * sizeof(uint16_t) + (static_cast<size_t>(c->n_cus) * 8u * (PQ_WAVES + 1u) + 64u) * sizeof(uint32_t);
        if (e == hipSuccess) e = hipMalloc(&s.d_cost, cost_bytes);
        if (e == hipSuccess) e = hipHostMalloc(&s.h_list_pinned, need * 2u * sizeof(uint32_t), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc(&s.h_cost_pinned, cost_bytes, hipHostMallocDefault);
        if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("work lists: ") + hipGetErrorString(e));
        s.list_capacity = need;
    }
    s.item_cost.assign(static_cast<size_t>(c->n_local) * 4, 0);
    s.item_is_dp.assign(static_cast<size_t>(c->n_local) * 4, 0);
    s.cur = 0;
    s.lists[0] = WorkList();                 // (no split entries, not final, dealt for no view)
    s.lists[0].entries = c->geometric;
    s.lists[1] = WorkList();
    if (!c->geometric.empty()) {
        list_to_device_form(shard_grid(c), c->geometric, s.h_list_pinned);
        HIPCHK(c, hipMemcpy(s.d_list[0], s.h_list_pinned, c->geometric.size() * 2u * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return VOLYM_OK;
}

// (Re)build the lists of this shard in every slot: geometric order, no costs.  Blocking set-up path (set_shard, options, uploads):
// costs no longer describe the scene (new volume, transfer function, threshold grid...).
int volym::rebuild_lists(volym_ctx* c)
{
    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    c->geometric = build_geometric(shard_grid(c));
    for (int i = 0; i < c->n_slots() && rc == VOLYM_OK; ++i) rc = reset_slot_lists(c, *c->slots[i]);
    return rc;
}

// the look-ahead's reject box (raymarch_device.h ahead_cannot_hit): positions u with clamp(floor(u * n), 0, n - 1) inside the
// texel AABB of the important voxels, open-ended where the AABB touches the border; 2e-6 covers the rounding of u * n
void volym::set_reject_box(const volym_ctx* c, FrameParams& fp)
{
    const uint32_t dims[3] = {c->inx, c->iny, c->inz};
    for (int a = 0; a < 3; ++a) {
        if (c->imp_box_lo[a] > c->imp_box_hi[a]) { fp.imp_lo[a] = INFINITY; fp.imp_hi[a] = -INFINITY; continue; }
        fp.imp_lo[a] = c->imp_box_lo[a] <= 0 ? -INFINITY : static_cast<float>(c->imp_box_lo[a]) / static_cast<float>(dims[a]) - 2.0e-6f;
        fp.imp_hi[a] = c->imp_box_hi[a] >= static_cast<int>(dims[a]) - 1 ? INFINITY : static_cast<float>(c->imp_box_hi[a] + 1) / static_cast<float>(dims[a]) + 2.0e-6f;
    }
}

extern "C" {

int volym_abi_version(void) { return VOLYM_ABI_VERSION; }

const char* volym_last_error(const volym_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// ---- frames in flight ------------------------------------------------------------------------------------------------
// A frame of the persistent kernel ends on its longest chains: for the last fifth of its time the CUs empty one by one
// (DESIGN.md 5).  With VOLYM_OPT_FRAMES_IN_FLIGHT = 2 the context has a second frame slot (context.hpp FrameSlot: stream,
// frame buffer, tables, distance field, work lists, feedback thread) that marches the same scene, and volym_compute_pass
// alternates between the two slots, so that the next frame's workgroups start on every CU the previous frame has left
// (measured: 31.9 -> 27.6 us per frame at 1920x1080).  The set-up calls act once on the scene and then on every slot's own
// state; the reading calls take the frame of the latest pass.

// Streams, buffers, lists and feedback thread of a new slot (set-up path).  On failure the caller frees the slot.
static int init_slot(volym_ctx* c, FrameSlot& s)
{
    auto bad = [&](hipError_t e, const char* what) {
        return fail(c, e == hipErrorOutOfMemory ? VOLYM_E_NOMEM : VOLYM_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    // the caller's current device may be another one: a slot's streams and buffers belong on the context's device
    HIPCHK(c, hipSetDevice(c->device));
    std::memset(&s.fp, 0, sizeof s.fp);
    std::memset(&s.tables_now, 0, sizeof s.tables_now);
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&s.own_stream, hipStreamNonBlocking)) != hipSuccess) return bad(e, "hipStreamCreate");
    if ((e = hipStreamCreateWithFlags(&s.copy_stream, hipStreamNonBlocking)) != hipSuccess) return bad(e, "hipStreamCreate");
    s.stream = s.own_stream;
    const size_t frame_bytes = static_cast<size_t>(c->W) * c->H * 4;
    if ((e = hipMalloc(&s.d_frame_own, frame_bytes)) != hipSuccess) return bad(e, "hipMalloc(frame)");
    if ((e = hipMalloc(&s.d_shard_own, static_cast<size_t>(c->n_tiles) * 1024)) != hipSuccess) return bad(e, "hipMalloc(shard)");
    if ((e = hipMalloc(&s.d_tables, sizeof(FrameTables))) != hipSuccess) return bad(e, "hipMalloc(tables)");
    if ((e = hipMalloc(&s.d_counters, sizeof(Counters))) != hipSuccess) return bad(e, "hipMalloc(counters)");
    if ((e = hipMemset(s.d_frame_own, 0, frame_bytes)) != hipSuccess) return bad(e, "hipMemset(frame)");
    if ((e = hipMalloc(&s.d_aabb, 6 * sizeof(int))) != hipSuccess) return bad(e, "hipMalloc(aabb)");
    if (c->tile_mask_words && (e = hipMalloc(&s.d_tile_mask, 2u * c->tile_mask_words * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMalloc(tile mask)");
    if (c->tile_mask_words && (e = hipMemset(s.d_tile_mask, 0, 2u * c->tile_mask_words * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMemset(tile mask)");
    if (c->tile_mask_words && (e = hipMalloc(&s.d_tile_depth, 64u * static_cast<size_t>(c->tile_mask_words) * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMalloc(tile depth)");
    if ((e = hipMalloc(&s.d_pack_counters, 4 * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMalloc(pack counters)");
    if ((e = hipMemset(s.d_pack_counters, 0, 4 * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMemset(pack counters)");
    if ((e = hipMalloc(&s.d_pool_sync, 4 * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMalloc(pool sync)");
    if ((e = hipMemset(s.d_pool_sync, 0, 4 * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMemset(pool sync)");
    if ((e = hipMalloc(&s.d_pool_dbg, static_cast<size_t>(c->n_cus) * 8u * PL_WAVES * 24u * sizeof(uint32_t))) != hipSuccess) return bad(e, "hipMalloc(pool timeline)");
    for (int i = 0; i < FrameSlot::TABLE_RING; ++i) {
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&s.h_tables[i]), sizeof(FrameTables), hipHostMallocDefault)) != hipSuccess) return bad(e, "hipHostMalloc(tables)");
        if ((e = hipEventCreateWithFlags(&s.tables_ev[i], hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    }
    if ((e = hipEventCreateWithFlags(&s.ev_march, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&s.ev_cost, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&s.ev_list, hipEventDisableTiming)) != hipSuccess) return bad(e, "hipEventCreate");
    if (c->write_f32 && (e = hipMalloc(&s.d_f32, static_cast<size_t>(c->W) * c->H * sizeof(float4))) != hipSuccess) return bad(e, "hipMalloc(f32 frame)");
    const int rc = reset_slot_lists(c, s);
    if (rc != VOLYM_OK) return rc;
    try {
        s.fb_thread = std::thread(feedback_thread, c, &s);
    } catch (...) {
        return fail(c, VOLYM_E_NOMEM, "cannot start the feedback thread");
    }
    return VOLYM_OK;
}

static void free_slot(FrameSlot& s)
{
    if (s.fb_thread.joinable()) {
        feedback_quiesce(s);
        {
            std::lock_guard<std::mutex> lk(s.fb_mu);
            s.fb_state.store(FrameSlot::FB_QUIT, std::memory_order_release);
        }
        s.fb_cv.notify_all();
        s.fb_thread.join();
    }
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.copy_stream) (void)hipStreamSynchronize(s.copy_stream);
    (void)hipFree(s.d_tables); (void)hipFree(s.d_df);
    (void)hipFree(s.d_shard_own); (void)hipFree(s.d_frame_own); (void)hipFree(s.d_f32); s.blit.release();
    s.gather_tmp.release(); (void)hipFree(s.d_pack_counters); (void)hipFree(s.d_counters); (void)hipFree(s.d_aabb); (void)hipFree(s.d_tile_mask);
    (void)hipFree(s.d_tile_depth);
    (void)hipFree(s.d_list[0]); (void)hipFree(s.d_list[1]); (void)hipFree(s.d_cost);
    (void)hipFree(s.d_pool_sync); (void)hipFree(s.d_pool_dbg);
    if (s.h_list_pinned) (void)hipHostFree(s.h_list_pinned);
    if (s.h_cost_pinned) (void)hipHostFree(s.h_cost_pinned);
    for (int i = 0; i < FrameSlot::TABLE_RING; ++i) {
        if (s.h_tables[i]) (void)hipHostFree(s.h_tables[i]);
        if (s.tables_ev[i]) (void)hipEventDestroy(s.tables_ev[i]);
    }
    if (s.ev_march) (void)hipEventDestroy(s.ev_march);
    if (s.ev_cost) (void)hipEventDestroy(s.ev_cost);
    if (s.ev_list) (void)hipEventDestroy(s.ev_list);
    if (s.own_stream) (void)hipStreamDestroy(s.own_stream);
    if (s.copy_stream) (void)hipStreamDestroy(s.copy_stream);
}

// the calls that address one stream or one shard buffer
static int refuse_two_slots(volym_ctx* c, const char* what)
{
    return fail(c, VOLYM_E_STATE, std::string(what) + ": not with VOLYM_OPT_FRAMES_IN_FLIGHT = 2");
}

int volym_create(volym_ctx** out, uint32_t width, uint32_t height, int device_id)
{
    if (!out) return fail(nullptr, VOLYM_E_INVALID, "volym_create: out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(nullptr, VOLYM_E_INVALID, "volym_create: viewport must be 1..32768 in each dimension");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(nullptr, VOLYM_E_NO_DEVICE, "volym_create: no HIP device visible");
    int dev = device_id;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= n_dev) return fail(nullptr, VOLYM_E_NO_DEVICE, "volym_create: device_id out of range");
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, VOLYM_E_NO_DEVICE,
                    std::string("volym_create: this library carries gfx950 code only, device is ") + prop.gcnArchName);
    HIPCHK(nullptr, hipSetDevice(dev));

    volym_ctx* c = new (std::nothrow) volym_ctx();
    if (!c) return fail(nullptr, VOLYM_E_NOMEM, "volym_create: out of host memory");
    c->device = dev;
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->W = width; c->H = height;
    c->tiles_x = (width + 15u) / 16u;     // src/demos/pipeline.rs:83-87
    c->tiles_y = (height + 15u) / 16u;
    c->n_tiles = c->tiles_x * c->tiles_y;
    recompute_shard(c);
    std::memset(c->aabb_tab, 0, sizeof c->aabb_tab);
    const uint64_t tiles8 = static_cast<uint64_t>(c->tiles_x) * 2u * c->tiles_y * 2u;
    const uint64_t words = (tiles8 + 31u) / 32u;
    c->tile_mask_words = words <= VOLYM_TILE_MASK_MAX_WORDS ? static_cast<uint32_t>(words) : 0u;
    c->geometric = build_geometric(shard_grid(c));

    c->slots[0].reset(new (std::nothrow) FrameSlot());
    const int rc = c->slots[0] ? init_slot(c, c->slot0()) : fail(c, VOLYM_E_NOMEM, "out of host memory");
    if (rc != VOLYM_OK) { const std::string m = c->err; volym_destroy(c); return fail(nullptr, rc, m); }
    *out = c;
    return VOLYM_OK;
}

void volym_destroy(volym_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (int i = 1; i >= 0; --i)
        if (c->slots[i]) free_slot(*c->slots[i]);
    // (every slot's stream is idle now: nothing reads the scene any more)
    (void)hipFree(c->d_vol); (void)hipFree(c->d_imp); (void)hipFree(c->d_labels); (void)hipFree(c->d_mc); (void)hipFree(c->d_mc_fine);
    (void)hipFree(c->d_vol0); (void)hipFree(c->d_imp0);
    free_pick(c);
    free_outline(c);
    free_slice(c);
    free_projection(c);
    free_measure(c);
    free_surface(c);
    free_components(c);
    free_distance(c);
    free_nearest(c);
    free_geodesic(c);
    free_cost(c);
    free_interpolate(c);
    free_label_history(c);
    free_lasso(c);
    for (uint32_t i = 0; i < volym_ctx::THROTTLE_RING; ++i) if (c->throttle_ev[i]) (void)hipEventDestroy(c->throttle_ev[i]);
    delete c;
}

int volym_set_stream(volym_ctx* c, void* hip_stream)
{
    if (!c) return VOLYM_E_INVALID;
    if (c->slots[1]) return refuse_two_slots(c, "volym_set_stream");
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    feedback_quiesce(s);
    HIPCHK(c, hipStreamSynchronize(s.stream));
    s.stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s.own_stream;
    return VOLYM_OK;
}

static int set_frames_in_flight(volym_ctx* c, int value)
{
    if (value != 1 && value != 2) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_FRAMES_IN_FLIGHT: 1 or 2");
    if (value == 1) {
        if (c->slots[1]) {
            int rc = volym_sync(c);
            if (rc != VOLYM_OK) return rc;
            // (a buffer of slot 1 itself does not stay bound: a caller may have bound what volym_frame_device_ptr gave)
            if (c->bound_frame == c->slots[1]->d_frame_own) c->bound_frame = nullptr;
            if (c->bound_shard == c->slots[1]->d_shard_own) c->bound_shard = nullptr;
            free_slot(*c->slots[1]);
            c->slots[1].reset();
            c->last = c->last_blit = 0; c->flight_parity = 0;
        }
        return VOLYM_OK;
    }
    if (c->slots[1]) return VOLYM_OK;
    if (c->have_vol || c->have_imp || c->have_tf)
        return fail(c, VOLYM_E_STATE, "VOLYM_OPT_FRAMES_IN_FLIGHT = 2: set it before the volume, the importances and the transfer function");
    if (c->slot0().stream != c->slot0().own_stream) return fail(c, VOLYM_E_STATE, "VOLYM_OPT_FRAMES_IN_FLIGHT = 2: not with a caller's stream (volym_set_stream)");
    // (slot 0's own buffer, bound by the caller, stays slot 0's alone: slot 1 renders into its own)
    if (c->bound_frame == c->slot0().d_frame_own) c->bound_frame = nullptr;
    if (c->bound_shard == c->slot0().d_shard_own) c->bound_shard = nullptr;
    c->slots[1].reset(new (std::nothrow) FrameSlot());
    const int rc = c->slots[1] ? init_slot(c, *c->slots[1]) : fail(c, VOLYM_E_NOMEM, "out of host memory");
    if (rc != VOLYM_OK) {
        if (c->slots[1]) free_slot(*c->slots[1]);
        c->slots[1].reset();
        return fail(c, rc, "second frame slot: " + c->err);
    }
    c->slots[1]->fp.dev = c->slot0().fp.dev;    // (dev option 110)
    return VOLYM_OK;
}

int volym_set_option(volym_ctx* c, int key, int value)
{
    if (!c) return VOLYM_E_INVALID;
    switch (key) {
    case VOLYM_OPT_FRAMES_IN_FLIGHT:
        return set_frames_in_flight(c, value);
    case VOLYM_OPT_KERNEL:
        if (value < 0 || value > 3) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_KERNEL: 0 (direct), 1 (macro-cell), 2 (persistent tiles + shading queue) or 3 (ray pool)");
        c->kernel_variant = value;
        return VOLYM_OK;
    case VOLYM_OPT_WRITE_F32:
        c->write_f32 = value != 0;
        for (int i = 0; i < c->n_slots() && c->write_f32; ++i) {
            FrameSlot& s = *c->slots[i];
            if (s.d_f32) continue;
            HIPCHK(c, hipSetDevice(c->device));
            hipError_t e = hipMalloc(&s.d_f32, static_cast<size_t>(c->W) * c->H * sizeof(float4));
            if (e != hipSuccess) { c->write_f32 = false; return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(f32 frame): ") + hipGetErrorString(e)); }
        }
        return VOLYM_OK;
    case VOLYM_OPT_MACRO_CELLS:
        // (64: the development build only -- a field that does not fit the LDS, measured slower; VOLYM_DF_IN_LDS)
        if (value < 4 || value > (VOLYM_DEV_SWITCHES ? 64 : 32) || (value & (value - 1)) != 0)
            return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_MACRO_CELLS: power of two in 4..32");
        c->mc_n = static_cast<uint32_t>(value);
        if (c->have_vol) { int rc = build_macro_cells(c); if (rc != VOLYM_OK) return rc; }
        return rebuild_lists(c);
    case VOLYM_OPT_BOUNDS_CELLS:
        if (value != -1 && value != 0 && (value < static_cast<int>(c->mc_n) || value > static_cast<int>(VOLYM_BOUNDS_CELLS_MAX) || (value & (value - 1)) != 0))
            return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_BOUNDS_CELLS: -1 (by the volume's size), 0 (the macro cells) or a power of two from VOLYM_OPT_MACRO_CELLS to 128");
        c->bounds_cells = value;
        for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->hull_dirty = true;
        return c->have_vol ? build_fine_cells(c) : VOLYM_OK;
    case VOLYM_OPT_VOLUME_LAYOUT:
        if (value < -1 || value > 1) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_VOLUME_LAYOUT: -1 (by size), 0 (linear) or 1 (4x4x4 bricks)");
        c->layout_choice = value;
        return VOLYM_OK;
    case VOLYM_OPT_CULLING:
        c->culling = value != 0;
        for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->hull_dirty = true;
        return VOLYM_OK;
    case VOLYM_OPT_COST_FEEDBACK:
        c->feedback = value != 0;
        return rebuild_lists(c);
    case VOLYM_OPT_DEPTH_PARALLEL:
        if (value < -100 || value > 65535) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_DEPTH_PARALLEL: < 0 adaptive (-N = N/10 x fair share), 0 off, else explicit cost");
        c->list_settings.dp_min_cost = value;
        return rebuild_lists(c);
    case VOLYM_OPT_REBALANCE_ROUNDS:   // 0: the dealt list is final
        if (value < 0 || value > 8) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_REBALANCE_ROUNDS: 0..8");
        c->list_settings.trim_rounds = static_cast<uint32_t>(value);
        return VOLYM_OK;
    case VOLYM_OPT_SETUP_IEEE:
        if (value != 0 && value != 1) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_SETUP_IEEE: 0 or 1");
        c->setup_ieee = value == 1;       // read by the next volym_update
        return VOLYM_OK;
    case VOLYM_OPT_TEXEL_BYTES:
        if (value != 0 && value != 1) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_TEXEL_BYTES: 0 or 1");
        c->texel_bytes = value == 1;      // read by the next launch
        return VOLYM_OK;
    case VOLYM_OPT_XCD_BANDS:
        if (value < 0 || value > 64) return fail(c, VOLYM_E_INVALID, "VOLYM_OPT_XCD_BANDS: 0..64");
        c->xcd_bands = static_cast<uint32_t>(value);
        return VOLYM_OK;
#if VOLYM_DEV_SWITCHES
    // tuning knobs of the development build (make DEV=1; scripts/ablate.py)
    case 101:   // persistent workgroups per CU (variant 2)
        if (value < 1 || value > 8) return fail(c, VOLYM_E_INVALID, "workgroups per CU: 1..8");
        c->wgs_per_cu = static_cast<uint32_t>(value);
        return rebuild_lists(c);
    case 107:   // 0 disables the 16x16 super fill items
        c->list_settings.super_fill = value != 0;
        return rebuild_lists(c);
    case 108:   // issue-priority thresholds t1 + 100*t2 + 10000*t3 in tenths of the fair share (0 = no priorities)
        if (value < 0) return fail(c, VOLYM_E_INVALID, "priority thresholds: t1 + 100*t2 + 10000*t3, tenths of the fair share");
        c->list_settings.prio_tenths[0] = static_cast<uint32_t>(value % 100);
        c->list_settings.prio_tenths[1] = static_cast<uint32_t>((value / 100) % 100);
        c->list_settings.prio_tenths[2] = static_cast<uint32_t>(value / 10000);
        return rebuild_lists(c);
    case 109:   // keep only the depth-parallel items in the work list (the frame is then incomplete)
        c->list_settings.only_quarters = value != 0;
        return rebuild_lists(c);
    case 110:   // FrameParams::dev
        for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->fp.dev = static_cast<uint32_t>(value);
        return VOLYM_OK;
    case 113:   // 1 freezes the cost feedback: no more captures, the current list stays (how fast do lists go stale?)
        for (int i = 0; i < c->n_slots(); ++i) feedback_quiesce(*c->slots[i]);
        c->feedback_frozen = value != 0;
        return VOLYM_OK;
    case 114:   // dilation radius (in 8x8 items) of the cost map when a list is dealt
        c->list_settings.dilate = std::max(-1, std::min(value, 4));
        return VOLYM_OK;
    case 115:   // waves per workgroup of the instantiations that need more than 128 VGPRs: 0 default, 12 or 16
        if (value != 0 && value != 12 && value != 16) return fail(c, VOLYM_E_INVALID, "wide waves: 0, 12 or 16");
        c->wide_waves = value;
        return rebuild_lists(c);
    case 119:   // floor of the adaptive split threshold (cost units)
        c->list_settings.dp_floor = static_cast<uint32_t>(std::max(value, 1));
        return rebuild_lists(c);
    case 118:   // drop the tiles of >= value/10 x the fair share from the lists (the frame is then incomplete): how much do they cost?
        c->list_settings.dev_drop_tenths = static_cast<uint32_t>(std::max(value, 0));
        return rebuild_lists(c);
    case 121:   // 1: the straight look-ahead as jobs shared by the workgroup (raymarch_pq.h CJ = 2)
        c->straight_jobs = value != 0;
        return VOLYM_OK;
    case 122:   // 1: the speculative voxel fetches of the common instantiation through LDS-staged bricks (raymarch_pq.h LB; bricked layout)
        c->lds_bricks = value != 0;
        return VOLYM_OK;
    case 123:   // 0: no per-tile depth bounds with the mask (raymarch_pq.h), 1 (default): bounds
        c->tile_depth = value != 0;
        for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->hull_dirty = true;
        return rebuild_lists(c);
    case 117:   // 0: no per-view tile mask (the hulls and the AABB clip stay); 2: a mask for every view, on its first frame
        c->tile_mask = value != 0;
        c->mask_eager = value == 2;
        for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->hull_dirty = true;
        return rebuild_lists(c);
    case 111:   // cost share of a depth-parallel quarter, percent of its tile's cost: value % 1000 (scripts still pass a combined value whose thousands nothing reads)
        c->list_settings.dp_share_pct = static_cast<uint32_t>(value % 1000);
        return rebuild_lists(c);
#endif
    default:
        return fail(c, VOLYM_E_INVALID, "volym_set_option: unknown key");
    }
}

int volym_set_shard(volym_ctx* c, uint32_t rank, uint32_t world)
{
    if (!c) return VOLYM_E_INVALID;
    if (world == 0 || rank >= world || world > 4096) return fail(c, VOLYM_E_INVALID, "volym_set_shard: need rank < world <= 4096");
    // the feedback threads read rank / world / n_local while they deal a list: let the jobs in flight finish (and the frames that
    // read the current lists) before any of them changes
    const int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    c->rank = rank; c->world = world;
    recompute_shard(c);
    return rebuild_lists(c);
}

int volym_set_transfer_function(volym_ctx* c, const uint8_t* rgba8, uint32_t n)
{
    if (!c) return VOLYM_E_INVALID;
    if (!rgba8 || n < 1 || n > 256) return fail(c, VOLYM_E_INVALID, "volym_set_transfer_function: 1..256 RGBA8 texels");
    std::memset(c->lut, 0, sizeof c->lut);
    std::memcpy(c->lut, rgba8, static_cast<size_t>(n) * 4);
    c->tf_n = n;
    c->have_tf = true;
    for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->tables_dirty = true;
    return VOLYM_OK;
}

}  // extern "C"

// Per-frame resources that depend on the uniforms: distance field for the threshold byte (a launch, in stream order) and
// the culling hulls (host arithmetic).  Nothing here allocates or waits.
static int ensure_frame_resources(volym_ctx* c, FrameSlot& s)
{
    if (s.df_thr_byte != s.thr_byte_cull) {
        // stream order: earlier frames finish reading d_df before this kernel rewrites it
        if (c->mc_n <= 32u) hipLaunchKernelGGL(volym_distance_field_kernel<1>, dim3(1), dim3(1024), 0, s.stream, c->d_mc, s.d_df, s.d_aabb, c->mc_n, s.thr_byte_cull);
        else hipLaunchKernelGGL(volym_distance_field_kernel<4>, dim3(1), dim3(1024), 0, s.stream, c->d_mc, s.d_df, s.d_aabb, c->mc_n, s.thr_byte_cull);
        HIPCHK(c, hipGetLastError());
        s.df_thr_byte = s.thr_byte_cull;
        s.hull_dirty = true;
    }
    if (s.hull_dirty) {
        compute_culling(c, s);
        s.fp.tile_mask = nullptr;
        s.fp.tile_depth = nullptr;
        s.fp.mask_words = c->tile_mask_words;
        s.fp.tile_mask_spare = s.d_tile_mask ? s.d_tile_mask + static_cast<size_t>(s.mask_cur ^ 1) * c->tile_mask_words : nullptr;
        s.mask_pending = s.mask_wanted;
        s.view_launches = 0;
    }
    // The tile mask costs a kernel per view (~13 us: device-scope atomics) and changes which tiles are constant from view to view.
    // It is built when a view is rendered a SECOND time: a standing view has it from its second frame on; a moving camera
    // never pays for it -- and does not want it: the lists it runs were dealt for earlier views, and a 16x16 entry that was
    // constant under that view's mask is four marched tiles on one wave under this one's (turntable at 3840x2160, 1 degree per
    // frame: 130 us per frame without a mask per view, 164 with; at 1080p, 0.25 degrees: 52 and 62).
    if (s.mask_pending && (s.view_launches >= 1u || c->mask_eager)) {
        ClipMatrix M;
        std::memcpy(M.m, s.mask_clip, sizeof M.m);
        // into the buffer the launches so far have kept zeroed; the launches from here on read it and zero the other one
        s.mask_cur ^= 1;
        uint32_t* cur = s.d_tile_mask + static_cast<size_t>(s.mask_cur) * c->tile_mask_words;
        // the cells of both kernels: the fine grid where the context holds one (the same criterion, the same margin, cells that nest
        // in the occupied macro cells, so inside the AABB whose corners compute_culling found in front of the eye)
        // A view with the cone look-ahead keeps the macro cells: its frame is the look-ahead jobs, not the march chains the finer grid
        // shortens, and with the 64 grid it was measured 1.7 % slower, reproducibly and for a reason not found (profiles/fine_bounds_ab.txt
        // point 2).  The flags belong to the view: a change of them makes the hulls dirty and the mask is built again.
        const bool cone_view = (s.fp.flags & F_IMP_RENDERING) != 0u && (s.fp.flags & F_CONE) != 0u;
        const bool fine = c->d_mc_fine != nullptr && !cone_view;
        const uint8_t* grid = fine ? c->d_mc_fine : c->d_mc;
        const uint32_t gn = fine ? c->fine_n : c->mc_n;
        const uint32_t cells = gn * gn * gn, nb = (gn + 7u) / 8u;
        if (static_cast<size_t>(c->tile_mask_words) * sizeof(uint32_t) <= 48u * 1024u) {
            // the mask fits LDS: aggregated per block of cells, only the words that are not zero travel
            hipLaunchKernelGGL(volym_tile_mask_lds_kernel, dim3(nb * nb * ((gn + 3u) / 4u)), dim3(256), c->tile_mask_words * sizeof(uint32_t), s.stream, grid, gn,
                               s.thr_byte_cull, M, s.mask_margin, c->W, c->H, c->tiles_x * 2u, c->tile_mask_words, cur);
        } else {
            hipLaunchKernelGGL(volym_tile_mask_kernel, dim3((cells + 255u) / 256u), dim3(256), 0, s.stream, grid, gn, s.thr_byte_cull, M, s.mask_margin,
                               c->W, c->H, c->tiles_x * 2u, c->tile_mask_words, cur);
        }
        HIPCHK(c, hipGetLastError());
        s.fp.tile_mask = cur;
        s.fp.cull |= CULL_TILE_MASK;
        if (c->tile_depth && s.d_tile_depth) {
            // the same cells' depth ranges per tile (raymarch_kernels.h volym_tile_depth_kernel): one buffer per slot, rewritten in stream
            // order behind the launches that read the last view's
            const uint32_t n_t8 = 32u * c->tile_mask_words;
            HIPCHK(c, hipMemsetAsync(s.d_tile_depth, 0, 2u * static_cast<size_t>(n_t8) * sizeof(uint32_t), s.stream));
            hipLaunchKernelGGL(volym_tile_depth_kernel, dim3(nb * nb * ((gn + 3u) / 4u)), dim3(256), 0, s.stream, grid, gn, s.thr_byte_cull, M,
                               s.mask_margin, s.fp.eye[0], s.fp.eye[1], s.fp.eye[2], c->W, c->H, c->tiles_x * 2u, n_t8, s.d_tile_depth);
            HIPCHK(c, hipGetLastError());
            s.fp.tile_depth = s.d_tile_depth;
            s.fp.cull |= CULL_TILE_DEPTH;
        }
        s.fp.tile_mask_spare = s.d_tile_mask + static_cast<size_t>(s.mask_cur ^ 1) * c->tile_mask_words;
        s.mask_pending = false;
        // costs measured before the mask existed describe tiles that are constant from here on: for the cost feedback this is a
        // new view (a list dealt from the old costs would balance work that is no longer there: 33.2 instead of 32.3 us)
        if (s.view_launches >= 1u) s.view_serial.fetch_add(1, std::memory_order_relaxed);
    }
    s.view_launches++;
    return VOLYM_OK;
}

// volym_update's part in one slot; view_changed: the uniforms differ from the last update's
static int update_slot(volym_ctx* c, FrameSlot& s, const volym_camera_uniforms* cam, const volym_parameter_uniforms* par, bool view_changed)
{
    const float step = par->raymarching_step_size;
    FrameParams& fp = s.fp;
    std::memcpy(fp.ivp, cam->inverse_view_proj, sizeof fp.ivp);
    fp.eye[0] = cam->camera_position[0]; fp.eye[1] = cam->camera_position[1]; fp.eye[2] = cam->camera_position[2];
    fp.thr = par->density_threshold;
    fp.base_step = step;
    fp.min_step = step * 0.25f;          // wgsl:244
    fp.alpha_y = fp.min_step * 100.0f;   // wgsl:314 with current_step_size == min_step_size
    fp.flags = (par->use_cone_importance_check == 1u ? F_CONE : 0u) | (par->use_importance_coloring == 1u ? F_IMP_COLORING : 0u) |
               (par->use_opacity == 1u ? F_OPACITY : 0u) | (par->use_importance_rendering == 1u ? F_IMP_RENDERING : 0u) |
               (par->use_gaussian_smoothing == 1u ? F_GAUSSIAN : 0u) | (c->filter == VOLYM_FILTER_LINEAR ? F_LINEAR : 0u);
    fp.ahead_steps = par->importance_check_ahead_steps;
    fp.W = c->W; fp.H = c->H;
    {
        // make_ray's shared-reciprocal divisions (raymarch_device.h): the host's part of the range argument
        fp.rcp_w = static_cast<float>(1.0 / static_cast<double>(c->W));
        fp.rcp_h = static_cast<float>(1.0 / static_cast<double>(c->H));
        bool vouch = c->W <= 16384u && c->H <= 16384u && !c->setup_ieee;
        for (int i = 0; i < 16; ++i) vouch = vouch && std::fabs(fp.ivp[i]) < 0x1p+60f;
        for (int i = 0; i < 3; ++i) {
            const float n0 = std::fabs(0.0f - fp.eye[i]), n1 = std::fabs(1.0f - fp.eye[i]);
            vouch = vouch && n0 >= 0x1p-40f && n0 <= 0x1p+40f && n1 >= 0x1p-40f && n1 <= 0x1p+40f;
        }
        fp.setup_lo = vouch ? 0x1p-40f : INFINITY;
    }
    fp.nx = c->nx; fp.ny = c->ny; fp.nz = c->nz;
    fp.tiles_x = c->tiles_x; fp.n_tiles = c->n_tiles;
    fp.tf_n = c->tf_n;
    set_reject_box(c, fp);
    const float sigma = 1.5f;            // wgsl:255
    for (int i = -2; i <= 2; ++i) {
        const float x = static_cast<float>(i) * 0.005f;
        fp.gauss_w[i + 2] = wgsl_exp(-(x * x) / (2.0f * sigma * sigma));
    }
    std::memcpy(fp.cone_cos, k_cone_cos, sizeof k_cone_cos);
    std::memcpy(fp.cone_sin, k_cone_sin, sizeof k_cone_sin);

    if (s.tables_dirty || s.tables_alpha_y != fp.alpha_y) {
        // New tables travel in stream order behind the frames that read the old ones.  The pinned staging slot must not be
        // rewritten before its copy has run: a ring of TABLE_RING slots, each with the event of its last copy.  Only a
        // caller that changes the step size or the transfer function TABLE_RING times while the device is that many frames
        // behind ever waits here.
        const int slot = s.tables_slot;
        s.tables_slot = (slot + 1) % FrameSlot::TABLE_RING;
        if (hipEventQuery(s.tables_ev[slot]) != hipSuccess) HIPCHK(c, hipEventSynchronize(s.tables_ev[slot]));
        build_tables(c, *s.h_tables[slot], fp.alpha_y);
        s.tables_now = *s.h_tables[slot];
        HIPCHK(c, hipMemcpyAsync(s.d_tables, s.h_tables[slot], sizeof(FrameTables), hipMemcpyHostToDevice, s.stream));
        HIPCHK(c, hipEventRecord(s.tables_ev[slot], s.stream));
        s.tables_dirty = false;
        s.tables_alpha_y = fp.alpha_y;
    }
    uint32_t tb = 256;
    for (int b = 255; b >= 0; --b)
        if (s.tables_now.rho[b] >= fp.thr) tb = static_cast<uint32_t>(b); else break;
    fp.thr_byte = tb;
    // continuous-rho modes (trilinear / smoothed) compare an interpolated value: give its rounding some room
    if (fp.flags & (F_LINEAR | F_GAUSSIAN)) {
        const float cons = fp.thr - std::fabs(fp.thr) * 1.0e-5f - 1.0e-7f;
        uint32_t tc = 256;
        for (int b = 255; b >= 0; --b)
            if (s.tables_now.rho[b] >= cons) tc = static_cast<uint32_t>(b); else break;
        s.thr_byte_cull = tc;
    } else {
        s.thr_byte_cull = tb;
    }
    if (view_changed) {
        s.view_serial.fetch_add(1, std::memory_order_relaxed);    // the lists stay valid (they are scheduling only); the feedback follows the view
        s.hull_dirty = true;                                      // hulls, AABB clip and tile mask belong to the view
    }
    return VOLYM_OK;
}

extern "C" {

int volym_update(volym_ctx* c, const volym_camera_uniforms* cam, const volym_parameter_uniforms* par)
{
    if (!c) return VOLYM_E_INVALID;
    if (!cam || !par) return fail(c, VOLYM_E_INVALID, "volym_update: NULL uniforms");
    if (!c->have_vol || !c->have_imp || !c->have_tf)
        return fail(c, VOLYM_E_STATE, "volym_update: set volume, importances and transfer function first");
    if (c->nx != c->inx || c->ny != c->iny || c->nz != c->inz)
        return fail(c, VOLYM_E_STATE, "volym_update: volume and importances differ in size");
    // The reference loops `while t < exit` with t += step on the GPU; a step that cannot advance t
    // would never terminate there.  Refuse such inputs instead of hanging the device.
    const float step = par->raymarching_step_size;
    if (!(step >= 1.0e-4f && step <= 1.0f)) return fail(c, VOLYM_E_INVALID, "volym_update: raymarching_step_size must be in [1e-4, 1]");
    if (!std::isfinite(par->density_threshold)) return fail(c, VOLYM_E_INVALID, "volym_update: density_threshold is not finite");
    if (par->importance_check_ahead_steps > 4096u) return fail(c, VOLYM_E_INVALID, "volym_update: importance_check_ahead_steps > 4096");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite((&cam->inverse_view_proj[0][0])[i])) return fail(c, VOLYM_E_INVALID, "volym_update: inverse_view_proj is not finite");
    for (int i = 0; i < 3; ++i)
        if (!(std::fabs(cam->camera_position[i]) <= 64.0f)) return fail(c, VOLYM_E_INVALID, "volym_update: |camera_position| must be <= 64 per axis");

    HIPCHK(c, hipSetDevice(c->device));
    const bool view_changed = !c->have_frame || std::memcmp(&c->cam_copy, cam, sizeof *cam) != 0 || std::memcmp(&c->par_copy, par, sizeof *par) != 0;
    for (int i = 0; i < c->n_slots(); ++i) {
        const int rc = update_slot(c, *c->slots[i], cam, par, view_changed);
        if (rc != VOLYM_OK) return rc;
    }
    c->cam_copy = *cam;
    c->par_copy = *par;
    c->have_frame = true;
    return VOLYM_OK;
}

}  // extern "C"

template <bool COUNT, bool TRACE = false>
static int launch_march(volym_ctx* c, FrameSlot& s)
{
    int rc = ensure_frame_resources(c, s);
    if (rc != VOLYM_OK) return rc;
    FrameParams fp = s.fp;
    fp.rank = c->rank; fp.world = c->world; fp.n_local = c->n_local;
    fp.mc_n = c->mc_n;
    fp.xcd_bands = c->xcd_bands;
    if (c->world == 1) fp.flags |= F_RASTER;
    if (c->write_f32 && c->world == 1) fp.flags |= F_WRITE_F32;
    if (c->n_local == 0) return VOLYM_OK;
    uint32_t grid = c->n_local;
    if (fp.xcd_bands) {
        const uint32_t chunks = 8u * fp.xcd_bands;
        const uint32_t per_chunk = (c->n_local + chunks - 1u) / chunks;
        grid = per_chunk * chunks;
    }
    uint32_t* const d_shard = c->shard_buf(s);
    uint32_t* const d_frame = c->frame_buf(s);
    Counters* cnt = (COUNT || (VOLYM_DEV_SWITCHES && (s.fp.dev & 512u))) ? s.d_counters : nullptr;
    uint4* trace = TRACE ? s.d_trace : nullptr;
    if (!COUNT && !TRACE && frame_uses_pool(c, fp.flags)) {
        // the ray pool (raymarch_pool.h): the common instantiation; every other flag set runs variant 2 below
        const uint32_t pgrid = std::min(256u, max_grid(c));         // (the lattice has 256 cells per superblock)
        uint32_t* dbg = s.pool_dbg ? s.d_pool_dbg : nullptr;
        if (c->bricked)
            hipLaunchKernelGGL((volym_raymarch_pool_kernel<true>), dim3(pgrid), dim3(PL_WAVES * 64), 0, s.stream, c->d_vol, s.d_tables, s.d_df, s.d_pool_sync, d_shard,
                               d_frame, s.d_f32, dbg, fp);
        else
            hipLaunchKernelGGL((volym_raymarch_pool_kernel<false>), dim3(pgrid), dim3(PL_WAVES * 64), 0, s.stream, c->d_vol, s.d_tables, s.d_df, s.d_pool_sync, d_shard,
                               d_frame, s.d_f32, dbg, fp);
        HIPCHK(c, hipGetLastError());
        s.pool_launched = true;
        return VOLYM_OK;
    }
    if (c->kernel_variant >= 2) {
        const bool plain = !COUNT && !TRACE;
        if (plain) feedback_poll(s);                      // adopt a list the feedback thread has finished
        const WorkList& wl = s.lists[s.cur];
        const uint32_t n_items = static_cast<uint32_t>(wl.entries.size());
        if (n_items == 0) return VOLYM_OK;
        // capture this launch's costs?  Only one capture is in flight; a list dealt from costs measured on this very view, on
        // whole 8x8 entries, is final
        const bool capture = plain && c->feedback && !c->feedback_frozen && s.fb_state.load(std::memory_order_acquire) == FrameSlot::FB_IDLE && (wl.view_serial != s.view_serial.load(std::memory_order_relaxed) || !wl.final_for_view);
        uint16_t* cost_out = capture ? s.d_cost : nullptr;
        const bool table = !(fp.flags & (F_LINEAR | F_GAUSSIAN));
        // IMP = false: opacity on and no importance colouring (the common cases), without (IR = false) or with (IR = true)
        // importance rendering; the instrumented launch always takes the general form
        const bool special = !COUNT && !(fp.flags & F_IMP_COLORING) && (fp.flags & F_OPACITY);
        const bool no_imp = special && !(fp.flags & F_IMP_RENDERING);
        const bool ir = special && (fp.flags & F_IMP_RENDERING);
        // Waves per workgroup of the instantiation (raymarch_pq.h WAVES).  Only the common instantiation fits the 128 VGPRs of a
        // 16-wave workgroup; the others either run 16 waves and keep 64-100 bytes per lane in scratch, or 12 waves without
        // scratch.  Measured (profiles/r02_kernel_resources.txt): while the volume is cache resident the fourth wave per SIMD
        // is worth more than the spills cost (importance 68 vs 71 us, smoothing 134 vs 148, trilinear 113 vs 127); on the
        // bricked 1024^3 volume with its label map (BASELINE configs[4] on one GPU) the 12-wave form wins (235 vs 259 us).
        const bool wide12 = c->wide_waves == 12 || (c->wide_waves == 0 && c->bricked && ir);
        const uint32_t waves = ((table && no_imp) || !wide12) ? PQ_WAVES : PQ_WAVES_WIDE;
        const uint32_t want = (n_items + waves - 1) / waves;
        const uint32_t pgrid = wl.grid ? wl.grid : std::max(1u, std::min(want, max_grid(c)));
#define VOLYM_PQ_LAUNCH_J(T, KS, I, B, R, WV, J)                                                                                 \
    hipLaunchKernelGGL((volym_raymarch_pq_kernel<T, COUNT && I, TRACE, KS, I, B, R, WV, J>), dim3(pgrid), dim3(WV * 64), 0, s.stream, c->d_vol,  \
                       c->d_imp, s.d_tables, s.d_df, reinterpret_cast<const uint2*>(s.d_list[s.cur]), n_items, cost_out, d_shard, d_frame, s.d_f32, cnt, trace, fp)
#define VOLYM_PQ_LAUNCH(T, KS, I, B, R, WV) VOLYM_PQ_LAUNCH_J(T, KS, I, B, R, WV, 0)
#if VOLYM_DEV_SWITCHES
#define VOLYM_PQ_LAUNCH_W(T, KS, I, B, R) do { if (wide12) VOLYM_PQ_LAUNCH(T, KS, I, B, R, PQ_WAVES_WIDE); else VOLYM_PQ_LAUNCH(T, KS, I, B, R, PQ_WAVES); } while (0)
#else
#define VOLYM_PQ_LAUNCH_W(T, KS, I, B, R) VOLYM_PQ_LAUNCH(T, KS, I, B, R, PQ_WAVES)
#endif
        // the cone look-ahead of the importance-rendering instantiation: its walks as jobs shared by the workgroup (raymarch_pq.h CJ)
        const bool cone_jobs = ir && (fp.flags & F_CONE) != 0u && !TRACE;
        // (dev, option 121: the straight look-ahead through the same ring, one lane per record -- measured: bonsai 79.6 us against 63.7,
        // teapot 92.4 against 79.7: a chain of 15 probes is too little work per record to pay for the ring; not in the product library)
        const bool straight_jobs = VOLYM_DEV_SWITCHES && ir && !(fp.flags & F_CONE) && !TRACE && c->straight_jobs;
        (void)straight_jobs;
        if (c->bricked) {
#if VOLYM_DEV_SWITCHES
            // (dev, option 122: north_star's LDS-staged bricks, measured in profiles/r03_lds_bricks_ab.txt; not in the product library)
            if (table && no_imp && c->lds_bricks && !COUNT && !TRACE)
                hipLaunchKernelGGL((volym_raymarch_pq_kernel<true, false, false, 4, false, true, false, PQ_WAVES, 0, true>), dim3(pgrid), dim3(PQ_WAVES * 64), 0, s.stream, c->d_vol,
                                   c->d_imp, s.d_tables, s.d_df, reinterpret_cast<const uint2*>(s.d_list[s.cur]), n_items, cost_out, d_shard, d_frame, s.d_f32, cnt, trace, fp);
            else
#endif
            if (table && no_imp) VOLYM_PQ_LAUNCH(true, 4, false, true, false, PQ_WAVES);
            else if (table && ir && cone_jobs) VOLYM_PQ_LAUNCH_J(true, 4, false, true, true, PQ_WAVES, 1);
#if VOLYM_DEV_SWITCHES
            else if (table && ir && straight_jobs) VOLYM_PQ_LAUNCH_J(true, 4, false, true, true, PQ_WAVES, 2);
#endif
            else if (table && ir) { if (wide12) VOLYM_PQ_LAUNCH(true, 4, false, true, true, PQ_WAVES_WIDE); else VOLYM_PQ_LAUNCH(true, 4, false, true, true, PQ_WAVES); }
            else if (table) VOLYM_PQ_LAUNCH_W(true, 4, true, true, false);
            else VOLYM_PQ_LAUNCH_W(false, 1, true, true, false);
        } else {
            // the headline instantiation's twin for 256 texels on every axis (raymarch_pq.h CUBE256): plain launches only
            const bool cube256 = table && no_imp && plain && c->texel_bytes && fp.nx == 256u && fp.ny == 256u && fp.nz == 256u;
            if (plain) c->last_march_cube256 = cube256;
            if (cube256)
                hipLaunchKernelGGL((volym_raymarch_cube256_kernel<true, false, false, 4, false, false, false, PQ_WAVES, 0, false, true>), dim3(pgrid), dim3(PQ_WAVES * 64), 0, s.stream, c->d_vol, c->d_imp, s.d_tables, s.d_df,
                                   reinterpret_cast<const uint2*>(s.d_list[s.cur]), n_items, cost_out, d_shard, d_frame, s.d_f32, cnt, trace, fp);
            else if (table && no_imp) VOLYM_PQ_LAUNCH(true, 4, false, false, false, PQ_WAVES);
            else if (table && ir && cone_jobs) VOLYM_PQ_LAUNCH_J(true, 4, false, false, true, PQ_WAVES, 1);
#if VOLYM_DEV_SWITCHES
            else if (table && ir && straight_jobs) VOLYM_PQ_LAUNCH_J(true, 4, false, false, true, PQ_WAVES, 2);
#endif
            else if (table && ir) VOLYM_PQ_LAUNCH_W(true, 4, false, false, true);
            else if (table) VOLYM_PQ_LAUNCH_W(true, 4, true, false, false);
            else VOLYM_PQ_LAUNCH_W(false, 1, true, false, false);
        }
#undef VOLYM_PQ_LAUNCH_W
#undef VOLYM_PQ_LAUNCH
#undef VOLYM_PQ_LAUNCH_J
        HIPCHK(c, hipGetLastError());
        if (capture) {
            // costs -> pinned host memory on the copy stream, behind this launch; the feedback thread takes it from there
            HIPCHK(c, hipEventRecord(s.ev_march, s.stream));
            HIPCHK(c, hipStreamWaitEvent(s.copy_stream, s.ev_march, 0));
            const size_t cost_bytes = static_cast<size_t>((n_items + 1u) & ~1u) * sizeof(uint16_t) + static_cast<size_t>(pgrid) * (waves + 1u) * sizeof(uint32_t);
            HIPCHK(c, hipMemcpyAsync(s.h_cost_pinned, s.d_cost, cost_bytes, hipMemcpyDeviceToHost, s.copy_stream));
            HIPCHK(c, hipEventRecord(s.ev_cost, s.copy_stream));
            FbJob& job = s.fb_job;
            job.list = s.cur;
            job.n_entries = n_items;
            job.launch.view_serial = s.view_serial.load(std::memory_order_relaxed);
            job.launch.captured_has_dp = wl.has_dp;
            job.launch.continuous = (fp.flags & (F_LINEAR | F_GAUSSIAN)) != 0u;
            job.launch.plain = table && no_imp;           // the common instantiation: the split threshold's floor was measured for it
            job.launch.max_grid = max_grid(c);
            job.launch.waves = waves;
            job.launch.grid = pgrid;
            job.set = c->list_settings;
            job.t_us[0] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
            {
                std::lock_guard<std::mutex> lk(s.fb_mu);
                s.fb_state.store(FrameSlot::FB_CAPTURED, std::memory_order_release);
            }
            s.fb_cv.notify_all();
        }
        return VOLYM_OK;
    }
#define VOLYM_DIRECT_LAUNCH(V, B)                                                                                                \
    hipLaunchKernelGGL((volym_raymarch_kernel<V, COUNT, TRACE, B>), dim3(grid), dim3(256), 0, s.stream, c->d_vol, c->d_imp, s.d_tables, \
                       s.d_df, d_shard, d_frame, s.d_f32, cnt, trace, fp)
    if (c->kernel_variant >= 1) { if (c->bricked) VOLYM_DIRECT_LAUNCH(1, true); else VOLYM_DIRECT_LAUNCH(1, false); }
    else { if (c->bricked) VOLYM_DIRECT_LAUNCH(0, true); else VOLYM_DIRECT_LAUNCH(0, false); }
#undef VOLYM_DIRECT_LAUNCH
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym::ctx_launch_march(volym_ctx* c) { return launch_march<false>(c, c->slot0()); }

extern "C" {

int volym_compute_pass(volym_ctx* c)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_frame) return fail(c, VOLYM_E_STATE, "volym_compute_pass: call volym_update first");
    HIPCHK(c, hipSetDevice(c->device));
    c->last = c->slots[1] ? static_cast<int>(c->flight_parity++ & 1u) : 0;    // frames in flight: the slots take turns
    c->frame_rendered = true;
    return launch_march<false>(c, *c->slots[c->last]);
}

// Back-pressure of a frame loop: the reference's loop cannot run ahead of the device by more than its swap chain holds
// (surface.get_current_texture() blocks, src/event_loop.rs:114).  Call once per frame after volym_compute_pass: marks the
// work enqueued so far and waits until the mark made `max_in_flight` calls ago has been reached.
int volym_throttle(volym_ctx* c, uint32_t max_in_flight)
{
    if (!c) return VOLYM_E_INVALID;
    if (max_in_flight == 0 || max_in_flight >= volym_ctx::THROTTLE_RING) return fail(c, VOLYM_E_INVALID, "volym_throttle: max_in_flight must be 1..8");
    HIPCHK(c, hipSetDevice(c->device));
    // The ring holds one slot more than the deepest wait (9 slots, max_in_flight <= 8): the mark made max_in_flight calls ago
    // is never the slot recorded by this call, and the slot recorded here was last recorded 9 calls ago -- an earlier call has
    // already waited for a later mark than that one (marks complete in stream order).
    const uint32_t slot = c->throttle_head % volym_ctx::THROTTLE_RING;
    // a pacing mark: nothing is read on the strength of it, so no system-scope fence (cache write-back and invalidation) between
    // two frames -- with the default event the marches of a paced loop ran 6 us apart (scripts/turntable_trace.py)
    if (!c->throttle_ev[slot] && hipEventCreateWithFlags(&c->throttle_ev[slot], hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
        (void)hipGetLastError();
        c->throttle_ev[slot] = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&c->throttle_ev[slot], hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(c->throttle_ev[slot], c->slots[c->last]->stream));   // the frame just enqueued
    c->throttle_head++;
    if (c->throttle_head > max_in_flight) {
        const uint32_t old = (c->throttle_head - 1u - max_in_flight) % volym_ctx::THROTTLE_RING;
        if (c->throttle_ev[old]) HIPCHK(c, hipEventSynchronize(c->throttle_ev[old]));
    }
    return VOLYM_OK;
}

// The ray-pool kernel (variant 3) bounds every wait it contains and reports a wait that ran out (a bug, never an input) in
// d_pool_sync[2]; the blocking calls look at it, so that a broken frame is an error and not a picture.  Stream is idle here.
static int check_pool_error(volym_ctx* c, FrameSlot& s)
{
    if (!s.pool_launched) return VOLYM_OK;
    uint32_t bits = 0;
    HIPCHK(c, hipMemcpy(&bits, s.d_pool_sync + 2, sizeof bits, hipMemcpyDeviceToHost));
    if (bits != 0u) {
        (void)hipMemset(s.d_pool_sync, 0, 4 * sizeof(uint32_t));
        return fail(c, VOLYM_E_HIP, "ray-pool kernel gave up waiting (error bits " + std::to_string(bits) + "): the frame is incomplete");
    }
    return VOLYM_OK;
}

int volym_sync(volym_ctx* c)
{
    if (!c) return VOLYM_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = c->n_slots() - 1; i >= 0; --i) {
        HIPCHK(c, hipStreamSynchronize(c->slots[i]->stream));
        const int rc = check_pool_error(c, *c->slots[i]);
        if (rc != VOLYM_OK) return rc;
    }
    return VOLYM_OK;
}

int volym_settle(volym_ctx* c)
{
    if (!c) return VOLYM_E_INVALID;
    for (int i = c->n_slots() - 1; i >= 0; --i) {
        FrameSlot& s = *c->slots[i];
        feedback_quiesce(s);
        if (!s.fb_job.error.empty()) { const std::string m = s.fb_job.error; s.fb_job.error.clear(); return fail(c, VOLYM_E_HIP, m); }
        // ... and run the feedback to its fixed point for the current view: frames of this view (what volym_compute_pass
        // enqueues) until the list in use is final -- measuring list, deal, re-balancing rounds (raymarch.hip, "cost feedback")
        if (!c->have_frame || c->kernel_variant < 2 || frame_uses_pool(c, s.fp.flags) || !c->feedback || c->feedback_frozen) continue;
        for (int round = 0; round < 12; ++round) {
            const WorkList& wl = s.lists[s.cur];
            if (wl.entries.empty() || (wl.view_serial == s.view_serial.load(std::memory_order_relaxed) && wl.final_for_view)) break;
            int rc = launch_march<false>(c, s);
            if (rc != VOLYM_OK) return rc;
            feedback_quiesce(s);
            if (!s.fb_job.error.empty()) { const std::string m = s.fb_job.error; s.fb_job.error.clear(); return fail(c, VOLYM_E_HIP, m); }
        }
    }
    return VOLYM_OK;
}

int volym_read_rgba8(volym_ctx* c, uint8_t* out)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = *c->slots[c->last];
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->frame_buf(s), static_cast<size_t>(c->W) * c->H * 4, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return check_pool_error(c, s);
}

int volym_tile_bounds_size(volym_ctx* c, uint32_t* tiles_x8, uint32_t* tiles_y8, uint32_t* mask_words)
{
    if (!c || !tiles_x8 || !tiles_y8 || !mask_words) return VOLYM_E_INVALID;
    *tiles_x8 = c->tiles_x * 2u; *tiles_y8 = c->tiles_y * 2u; *mask_words = c->tile_mask_words;
    return VOLYM_OK;
}

int volym_read_tile_bounds(volym_ctx* c, uint32_t* mask_bits, float* near, float* far)
{
    if (!c) return VOLYM_E_INVALID;
    if (!mask_bits || !near || !far) return fail(c, VOLYM_E_INVALID, "volym_read_tile_bounds: NULL output");
    FrameSlot& s = *c->slots[c->last];
    if (!(s.fp.cull & CULL_TILE_MASK) || !s.fp.tile_mask || s.mask_pending || s.hull_dirty)
        return fail(c, VOLYM_E_STATE, "volym_read_tile_bounds: the view of the latest pass has no tile mask (it gets one with its second frame)");
    const uint32_t words = c->tile_mask_words, n_t8 = 32u * words;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint32_t> enc;
    const bool depth = (s.fp.cull & CULL_TILE_DEPTH) != 0u && s.fp.tile_depth;
    // (the launches of this view read the mask and keep the other buffer zeroed: the words are the mask kernel's)
    HIPCHK(c, hipMemcpyAsync(mask_bits, s.fp.tile_mask, static_cast<size_t>(words) * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    if (depth) {
        enc.resize(2u * static_cast<size_t>(n_t8));
        HIPCHK(c, hipMemcpyAsync(enc.data(), s.fp.tile_depth, enc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    }
    HIPCHK(c, hipStreamSynchronize(s.stream));
    for (uint32_t t = 0; t < n_t8; ++t) {
        near[t] = 0.0f; far[t] = INFINITY;                              // no bounds: the rays keep their whole length
        if (!depth) continue;
        const uint32_t ne = ~enc[t], fe = enc[n_t8 + t];
        if (fe == 0u) { near[t] = INFINITY; far[t] = 0.0f; continue; }  // no cell projects onto the tile: no sample is left
        std::memcpy(&near[t], &ne, 4); std::memcpy(&far[t], &fe, 4);
    }
    return VOLYM_OK;
}

int volym_read_rgba32f(volym_ctx* c, float* out)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = *c->slots[c->last];
    if (!c->write_f32 || !s.d_f32 || c->world != 1)
        return fail(c, VOLYM_E_STATE, "volym_read_rgba32f: needs VOLYM_OPT_WRITE_F32 = 1, world == 1 and a rendered frame");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, s.d_f32, static_cast<size_t>(c->W) * c->H * sizeof(float4), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return VOLYM_OK;
}

// ---- blit: the step after the path (src/render_pipeline.rs:88-130, shaders/render.wgsl:39-43) -------------------------
int volym_blit(volym_ctx* c, void* target_rgba8, uint32_t out_w, uint32_t out_h)
{
    if (!c) return VOLYM_E_INVALID;
    c->last_blit = c->last;
    FrameSlot& s = *c->slots[c->last_blit];
    if (out_w == 0 || out_h == 0 || out_w > 32768 || out_h > 32768) return fail(c, VOLYM_E_INVALID, "volym_blit: target must be 1..32768 in each dimension");
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t* dst = static_cast<uint32_t*>(target_rgba8);
    if (!dst) {
        // our own target: sized on first use / on a size change (a set-up step: this is the one blocking path of the call)
        const size_t need = static_cast<size_t>(out_w) * out_h;
        const int rc = s.blit.reserve(c, s.stream, need, "blit target");
        if (rc != VOLYM_OK) return rc;
        dst = s.blit.ptr;
        s.blit_w = out_w; s.blit_h = out_h;
        s.blit.count = need;
    }
    hipLaunchKernelGGL(volym_blit_kernel, dim3((out_w + 63u) / 64u, (out_h + 3u) / 4u), dim3(64, 4), 0, s.stream, c->frame_buf(s), c->W, c->H, dst, out_w, out_h);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_read_blit(volym_ctx* c, uint8_t* out)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = *c->slots[c->last_blit];
    if (s.blit.count == 0u) return fail(c, VOLYM_E_STATE, "volym_read_blit: no volym_blit into the context's own target yet");
    return s.blit.read(c, s.stream, out, s.blit.count);
}

uint32_t volym_local_tiles(const volym_ctx* c) { return c ? c->n_local : 0u; }
size_t volym_shard_bytes(const volym_ctx* c) { return c ? static_cast<size_t>(c->shard_tiles) * 1024u : 0u; }
// the buffers of the latest pass, as volym_read_rgba8 reads them
void* volym_shard_device_ptr(volym_ctx* c) { return c ? c->shard_buf(*c->slots[c->last]) : nullptr; }
void* volym_frame_device_ptr(volym_ctx* c) { return c ? c->frame_buf(*c->slots[c->last]) : nullptr; }

int volym_bind_output(volym_ctx* c, void* shard_rgba8, void* frame_rgba8)
{
    if (!c) return VOLYM_E_INVALID;
    // takes effect for launches enqueued after this call; earlier launches keep their pointers.  Every slot renders into the
    // same buffers (NULL: each slot its own)
    c->bound_shard = static_cast<uint32_t*>(shard_rgba8);
    c->bound_frame = static_cast<uint32_t*>(frame_rgba8);
    return VOLYM_OK;
}

int volym_read_shard(volym_ctx* c, uint8_t* out)
{
    if (c && c->slots[1]) return refuse_two_slots(c, "volym_read_shard");
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    // the padding tile of a short shard is never written by the kernel: define it
    const size_t used = static_cast<size_t>(c->n_local) * 1024u, total = volym_shard_bytes(c);
    HIPCHK(c, hipMemcpyAsync(out, c->shard_buf(s), used, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    if (total > used) std::memset(out + used, 0, total - used);
    return VOLYM_OK;
}

size_t volym_packed_shard_bytes(const volym_ctx* c, uint32_t tiles)
{
    if (!c) return 0u;
    return pack_header_bytes(c->shard_tiles) + static_cast<size_t>(std::min(tiles, c->shard_tiles)) * 1024u;
}

int volym_pack_shard(volym_ctx* c, void* packed, size_t capacity_bytes)
{
    if (c && c->slots[1]) return refuse_two_slots(c, "volym_pack_shard");
    if (!c || !packed) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    const size_t header = pack_header_bytes(c->shard_tiles);
    if (capacity_bytes < header) return fail(c, VOLYM_E_INVALID, "volym_pack_shard: the buffer does not even hold the header (volym_packed_shard_bytes)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->n_local == 0) return VOLYM_OK;
    const uint32_t max_slots = static_cast<uint32_t>(std::min<size_t>((capacity_bytes - header) / 1024u, c->shard_tiles));
    hipLaunchKernelGGL(volym_pack_shard_kernel, dim3(c->n_local), dim3(64), 0, s.stream, c->shard_buf(s), static_cast<uint8_t*>(packed), c->n_local,
                       c->shard_tiles, max_slots, s.d_pack_counters, s.pack_parity);
    HIPCHK(c, hipGetLastError());
    s.pack_parity ^= 1u;
    return VOLYM_OK;
}

int volym_packed_tiles(volym_ctx* c, uint32_t* tiles_used, uint32_t* overflowed)
{
    if (c && c->slots[1]) return refuse_two_slots(c, "volym_packed_tiles");
    if (!c || !tiles_used) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t h[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h, s.d_pack_counters, sizeof(h), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    *tiles_used = h[s.pack_parity ^ 1u];        // the counter the last launch used
    if (overflowed) *overflowed = h[2];
    return VOLYM_OK;
}

int volym_assemble_packed(volym_ctx* c, const void* gathered, size_t stride_bytes)
{
    if (c && c->slots[1]) return refuse_two_slots(c, "volym_assemble_packed");
    if (!c || !gathered) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    if (stride_bytes < pack_header_bytes(c->shard_tiles)) return fail(c, VOLYM_E_INVALID, "volym_assemble_packed: stride smaller than the header");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(volym_assemble_packed_kernel, dim3(c->n_tiles), dim3(256), 0, s.stream, static_cast<const uint8_t*>(gathered), stride_bytes,
                       c->frame_buf(s), c->W, c->H, c->tiles_x, c->n_tiles, c->world, c->shard_tiles);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_assemble(volym_ctx* c, const void* gathered)
{
    if (c && c->slots[1]) return refuse_two_slots(c, "volym_assemble");
    if (!c || !gathered) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(volym_assemble_kernel, dim3(c->n_tiles), dim3(256), 0, s.stream, static_cast<const uint32_t*>(gathered),
                       c->frame_buf(s), c->W, c->H, c->tiles_x, c->n_tiles, c->world, c->shard_tiles);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

int volym_assemble_host(volym_ctx* c, const uint8_t* gathered_host)
{
    if (c && c->slots[1]) return refuse_two_slots(c, "volym_assemble_host");
    if (!c || !gathered_host) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = volym_shard_bytes(c) * c->world;
    const int rc = s.gather_tmp.reserve(c, s.stream, bytes, "gather");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(s.gather_tmp.ptr, gathered_host, bytes, hipMemcpyHostToDevice, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    return volym_assemble(c, s.gather_tmp.ptr);
}

int volym_stats_pass(volym_ctx* c, volym_stats* out)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    if (!c->have_frame) return fail(c, VOLYM_E_STATE, "volym_stats_pass: call volym_update first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(s.d_counters, 0, sizeof(Counters), s.stream));
    int rc = launch_march<true>(c, s);
    if (rc != VOLYM_OK) return rc;
    Counters h;
    HIPCHK(c, hipMemcpyAsync(&h, s.d_counters, sizeof h, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    out->n_vol = h.n_vol; out->n_imp = h.n_imp; out->n_steps = h.n_steps; out->n_dense = h.n_dense; out->n_hit = h.n_hit;
    // every pixel of an owned tile that lies inside the frame launches a ray (wgsl:217-219)
    uint64_t rays = 0;
    for (uint32_t k = c->rank; k < c->n_tiles; k += c->world) {
        const uint32_t tx = k % c->tiles_x, ty = k / c->tiles_x;
        const uint32_t w = std::min(16u, c->W - tx * 16u), h2 = std::min(16u, c->H - ty * 16u);
        rays += static_cast<uint64_t>(w) * h2;
    }
    out->n_rays = rays;
    return VOLYM_OK;
}

// Both forms of the ray set-up (raymarch_device.h make_ray) for every pixel of the current frame, compared bit for bit on the
// device.  out[0]: rays whose shared-reciprocal set-up (as the march kernels run it, fallback included) differs from the plain
// divisions in any bit of direction / entry / exit / hit; out[1]: rays of waves that took the fallback; out[2]: rays.
int volym_selftest_ray_setup(volym_ctx* c, unsigned long long out[3])
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    if (!c->have_frame) return fail(c, VOLYM_E_STATE, "volym_selftest_ray_setup: call volym_update first");
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(Counters) >= 3 * sizeof(unsigned long long), "counters");
    HIPCHK(c, hipMemsetAsync(s.d_counters, 0, sizeof(Counters), s.stream));
    const dim3 grid((c->W + 63u) / 64u, (c->H + 3u) / 4u);
    volym_ray_setup_selftest_kernel<<<grid, 256, 0, s.stream>>>(s.fp, reinterpret_cast<unsigned long long*>(s.d_counters));
    HIPCHK(c, hipGetLastError());
    Counters h;
    HIPCHK(c, hipMemcpyAsync(&h, s.d_counters, sizeof h, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    out[0] = h.n_vol; out[1] = h.n_imp; out[2] = h.n_steps;
    return VOLYM_OK;
}

// Both forms of the texel selection of a 256-texel axis (raymarch_device.h texel256_insert), compared on the device over every float
// of magnitude in [2^-10, 512) and the special values.  out: volym_texel256_selftest_kernel's five counts.
int volym_selftest_texel256(volym_ctx* c, unsigned long long out[5])
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    static_assert(sizeof(Counters) == 5 * sizeof(unsigned long long), "counters");
    HIPCHK(c, hipMemsetAsync(s.d_counters, 0, sizeof(Counters), s.stream));
    volym_texel256_selftest_kernel<<<4096, 256, 0, s.stream>>>(reinterpret_cast<unsigned long long*>(s.d_counters));
    HIPCHK(c, hipGetLastError());
    Counters h;
    HIPCHK(c, hipMemcpyAsync(&h, s.d_counters, sizeof h, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    out[0] = h.n_vol; out[1] = h.n_imp; out[2] = h.n_steps; out[3] = h.n_dense; out[4] = h.n_hit;
    return VOLYM_OK;
}

int volym_texel_bytes_in_use(volym_ctx* c)
{
    return c && c->last_march_cube256 ? 1 : 0;
}

int volym_time_batch(volym_ctx* c, uint32_t n, float* ms_total)
{
    if (!c || !ms_total || n == 0 || n > 1000000) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    if (!c->have_frame) return fail(c, VOLYM_E_STATE, "volym_time_batch: call volym_update first");
    HIPCHK(c, hipSetDevice(c->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { if (e0) (void)hipEventDestroy(e0); return fail(c, VOLYM_E_HIP, "hipEventCreate failed"); }
    int rc = ensure_frame_resources(c, s);
    if (rc == VOLYM_OK) {
        (void)hipEventRecord(e0, s.stream);
        for (uint32_t i = 0; i < n && rc == VOLYM_OK; ++i) rc = launch_march<false>(c, s);
        (void)hipEventRecord(e1, s.stream);
        if (hipStreamSynchronize(s.stream) != hipSuccess && rc == VOLYM_OK) rc = fail(c, VOLYM_E_HIP, "hipStreamSynchronize failed");
        if (rc == VOLYM_OK && hipEventElapsedTime(ms_total, e0, e1) != hipSuccess) rc = fail(c, VOLYM_E_HIP, "hipEventElapsedTime failed");
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rc;
}

int volym_time_passes(volym_ctx* c, uint32_t n, float* ms_each)
{
    if (!c || !ms_each || n == 0 || n > 100000) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    if (!c->have_frame) return fail(c, VOLYM_E_STATE, "volym_time_passes: call volym_update first");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<hipEvent_t> ev(n + 1, nullptr);
    int rc = VOLYM_OK;
    for (uint32_t i = 0; i <= n && rc == VOLYM_OK; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = fail(c, VOLYM_E_HIP, "hipEventCreate failed");
    if (rc == VOLYM_OK) rc = ensure_frame_resources(c, s);
    if (rc == VOLYM_OK) {
        (void)hipEventRecord(ev[0], s.stream);
        for (uint32_t i = 0; i < n && rc == VOLYM_OK; ++i) {
            rc = launch_march<false>(c, s);
            if (hipEventRecord(ev[i + 1], s.stream) != hipSuccess && rc == VOLYM_OK) rc = fail(c, VOLYM_E_HIP, "hipEventRecord failed");
        }
        if (hipStreamSynchronize(s.stream) != hipSuccess && rc == VOLYM_OK) rc = fail(c, VOLYM_E_HIP, "hipStreamSynchronize failed");
        if (rc == VOLYM_OK)
            for (uint32_t i = 0; i < n; ++i)
                if (hipEventElapsedTime(&ms_each[i], ev[i], ev[i + 1]) != hipSuccess) { rc = fail(c, VOLYM_E_HIP, "hipEventElapsedTime failed"); break; }
    }
    for (auto e : ev) if (e) (void)hipEventDestroy(e);
    return rc;
}

#if VOLYM_DEV_SWITCHES
// ---- development build only (make DEV=1): not declared in the public headers, not in the product library ------------
// per-item costs (uint16) as the feedback thread last saw them; out needs 4 * n_local entries
// development: per-wave timeline of the NEXT ray-pool launches (on != 0) / read the last one back (blocking)
int volym_dev_pool_timeline(volym_ctx* c, int on, uint32_t* out, uint32_t max_words)
{
    if (!c) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    const uint32_t words = std::min(max_words, static_cast<uint32_t>(max_grid(c)) * PL_WAVES * 24u);
    if (out && words) HIPCHK(c, hipMemcpy(out, s.d_pool_dbg, static_cast<size_t>(words) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    s.pool_dbg = on != 0;
    return static_cast<int>(words);
}

// development: the raw counters (fp.dev & 512: the cone-job debug counts of the plain launches since the last reset); reset != 0 zeroes them
int volym_dev_counters(volym_ctx* c, unsigned long long out[5], int reset)
{
    if (!c) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    if (out) HIPCHK(c, hipMemcpy(out, s.d_counters, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(c, hipMemset(s.d_counters, 0, sizeof(Counters)));
    return VOLYM_OK;
}

int volym_dev_read_costs(volym_ctx* c, uint16_t* out, uint32_t max_items)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    feedback_quiesce(s);
    const uint32_t n = c->n_local * 4u;
    if (max_items < n || s.item_cost.size() < n) return VOLYM_E_INVALID;
    std::memcpy(out, s.item_cost.data(), n * sizeof(uint16_t));
    return static_cast<int>(n);
}

// wall-clock stamps (us) of the last finished feedback job: capture enqueued, worker woke, costs arrived, costs mapped to
// items, list dealt, list uploaded
int volym_dev_feedback_timing(volym_ctx* c, double out[6])
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    feedback_quiesce(s);
    for (int i = 0; i < 6; ++i) out[i] = s.fb_job.t_us[i];
    return VOLYM_OK;
}

// the work list the next launch will read; returns the number of entries
int volym_dev_read_order(volym_ctx* c, uint32_t* out, uint32_t max_items)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    feedback_quiesce(s);
    const WorkList& wl = s.lists[s.cur];
    if (max_items < wl.entries.size()) return VOLYM_E_INVALID;
    std::memcpy(out, wl.entries.data(), wl.entries.size() * sizeof(uint32_t));
    return static_cast<int>(wl.entries.size());
}

// One instrumented launch that records, per wave, {start tick, duration ticks (100 MHz), loop iterations, ...} (variant 2: four
// uint4 per wave, the others two; scripts/wave_trace.py); returns the number of records or a negative error.
int volym_dev_wave_trace(volym_ctx* c, uint32_t* out, uint32_t max_records)
{
    if (!c || !out) return VOLYM_E_INVALID;
    FrameSlot& s = c->slot0();
    if (!c->have_frame) return fail(c, VOLYM_E_STATE, "volym_dev_wave_trace: call volym_update first");
    HIPCHK(c, hipSetDevice(c->device));
    // a lone launch on an idle GPU runs at idle clocks: trace the 31st of 31 back-to-back passes
    int rc = VOLYM_OK;
    for (int i = 0; i < 30 && rc == VOLYM_OK; ++i) rc = launch_march<false, false>(c, s);
    if (rc != VOLYM_OK) return rc;
    feedback_quiesce(s);
    // records: per wave of the grid that is really launched (variant 2: the list's grid, four each; variants 0/1: 4 waves per tile, two each)
    const WorkList& wl = s.lists[s.cur];
    const uint32_t n_items = static_cast<uint32_t>(wl.entries.size());
    const uint32_t pgrid = wl.grid ? wl.grid : std::max(1u, std::min((n_items + PQ_WAVES - 1) / PQ_WAVES, max_grid(c)));
    const uint32_t waves = c->kernel_variant >= 2 ? pgrid * PQ_WAVES : (c->n_local + 64u * 8u) * 4u;   // PQ_WAVES >= every instantiation's WAVES
    const uint32_t records = waves * (c->kernel_variant >= 2 ? 4u : 2u);
    if (max_records < records) return fail(c, VOLYM_E_INVALID, "volym_dev_wave_trace: buffer too small");
    HIPCHK(c, hipMalloc(&s.d_trace, static_cast<size_t>(records) * sizeof(uint4)));
    HIPCHK(c, hipMemsetAsync(s.d_trace, 0, static_cast<size_t>(records) * sizeof(uint4), s.stream));
    rc = launch_march<false, true>(c, s);
    if (rc == VOLYM_OK) {
        hipError_t e = hipMemcpyAsync(out, s.d_trace, static_cast<size_t>(records) * sizeof(uint4), hipMemcpyDeviceToHost, s.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
        if (e != hipSuccess) rc = fail(c, VOLYM_E_HIP, hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(s.stream);
    (void)hipFree(s.d_trace);
    s.d_trace = nullptr;
    return rc == VOLYM_OK ? static_cast<int>(records) : rc;
}
#endif

}  // extern "C"

#include "mgpu.inc"
