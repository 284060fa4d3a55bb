// libvolym_hip.so: the bytes of the scene.  Volume, label and importance uploads, the device layout, the macro cells, and the
// one transition (retarget) that keeps density and importances cut to the crop box, the clip plane and the segment mask; the C ABI entry
// points of all of these.  The frame loop (raymarch.hip) reads what this unit writes; what the two need from each other is
// declared in context.hpp.  Everything here is blocking set-up path.  The measure pass (measure.hip), which only reads these bytes, and
// the label edits (relabel.hip, brush.hip, lasso.hip, smooth.hip), which rewrite labels in place and carry density and importances along
// by the same invariant, are units of their own: the six functions they need of this one are declared in scene_bytes.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "scene_bytes.hpp"
#include "scene_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

// ---- device layout and uploads ----------------------------------------------------------------------------------------

// Bricks pay once the volume outgrows the L2s (measured: from 512^3 on; see raymarch_device.h); volume and importances of
// the same dimensions get the same answer.
static bool want_bricked(const volym_ctx* c, uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (c->layout_choice >= 0) return c->layout_choice == 1;
    return static_cast<uint64_t>(nx) * ny * nz > c->brick_from_bytes;
}

// bytes of a volume in the device layout (without the 16 bytes every allocation of one adds)
static uint64_t layout_bytes(bool bricked, uint32_t nx, uint32_t ny, uint32_t nz)
{
    return bricked ? static_cast<uint64_t>(brick_count(nx)) * brick_count(ny) * brick_count(nz) * 64u : static_cast<uint64_t>(nx) * ny * nz;
}

// A buffer for nb layout bytes and the 16 zeroed bytes every volume ends in: the trilinear fetch reads voxel pairs (one byte past
// the last voxel is touched) and the chunk kernels walk whole 16-byte chunks.  On failure *p is NULL.
static hipError_t alloc_layout(uint8_t** p, uint64_t nb)
{
    hipError_t e = hipMalloc(p, nb + 16u);
    if (e == hipSuccess) e = hipMemset(*p + nb, 0, 16);
    if (e != hipSuccess) { (void)hipFree(*p); *p = nullptr; }
    return e;
}

// grid of the kernels that stream a layout in 16-byte chunks, one chunk per lane and step
uint32_t volym::stream_grid(const volym_ctx* c, uint64_t n_chunks)
{
    const uint64_t g = std::min<uint64_t>((n_chunks + 255u) / 256u, static_cast<uint64_t>(c->n_cus) * 8u);
    return static_cast<uint32_t>(std::max<uint64_t>(g, 1u));
}

static int upload_volume(volym_ctx* c, uint8_t** dst, const uint8_t* src, uint32_t nx, uint32_t ny, uint32_t nz)
{
    const bool bricked = want_bricked(c, nx, ny, nz);
    if (!src || nx == 0 || ny == 0 || nz == 0) return fail(c, VOLYM_E_INVALID, "volume: NULL data or zero dimension");
    const uint64_t n = static_cast<uint64_t>(nx) * ny * nz;
    const uint64_t nb = layout_bytes(bricked, nx, ny, nz);
    if (nx > 4096 || ny > 4096 || nz > 4096 || nb > 0xffffffffull)
        return fail(c, VOLYM_E_INVALID, "volume: each dimension <= 4096 and the brick-padded size < 2^32");
    const int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    ++c->scene_serial;          // density or labels are replaced, or (importances) the labels are about to go: a surface pass is stale
    if (*dst) { HIPCHK(c, hipFree(*dst)); *dst = nullptr; }
    uint8_t* staging = nullptr;
    hipError_t e = alloc_layout(dst, nb);
    if (e == hipSuccess && bricked) e = hipMalloc(&staging, n);
    if (e != hipSuccess) { (void)hipFree(staging); return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(volume): ") + hipGetErrorString(e)); }
    e = hipMemcpy(bricked ? staging : *dst, src, n, hipMemcpyHostToDevice);
    if (e == hipSuccess && bricked) {
        const hipStream_t stream = c->slot0().stream;
        hipLaunchKernelGGL(volym_rebrick_kernel, dim3(static_cast<uint32_t>((nb + 255u) / 256u)), dim3(256), 0, stream, staging, *dst, nx, ny, nz);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(c, VOLYM_E_HIP, std::string("volume upload: ") + hipGetErrorString(e));
    return VOLYM_OK;
}

// ---- macro cells ------------------------------------------------------------------------------------------------------

extern "C" {

int volym_cells_meeting_box(uint32_t n_cells, uint32_t dim, uint32_t lo, uint32_t hi, uint32_t* c0, uint32_t* c1)
{
    if (!c0 || !c1 || n_cells == 0u || n_cells > 4096u || dim == 0u || dim > 65536u) return VOLYM_E_INVALID;
    // mc_voxel_lo and mc_voxel_hi do not decrease with the cell: the cells that meet [lo, hi) are consecutive
    uint32_t a = n_cells, b = 0;
    if (lo < hi)
        for (uint32_t k = 0; k < n_cells; ++k)
            if (mc_voxel_lo(k, dim, n_cells) < hi && mc_voxel_hi(k, dim, n_cells) > lo) { a = std::min(a, k); b = k + 1u; }
    *c0 = a < b ? a : 0u; *c1 = a < b ? b : 0u;
    return VOLYM_OK;
}

uint32_t volym_bounds_cells_for(const uint32_t dims[3], uint32_t macro_cells)
{
    if (!dims) return macro_cells;
    const uint32_t longest = std::max(dims[0], std::max(dims[1], dims[2]));
    uint32_t n = 1;
    while (n < VOLYM_BOUNDS_CELLS_DEFAULT_MAX && 4u * n <= longest) n *= 2u;         // the largest power of two with 2 * n <= longest, at most the cap
    return std::max(n, macro_cells);
}

}  // extern "C"

static int launch_fine_grid(volym_ctx* c);

// the maxima of one range of cells, on slot 0's stream
static int launch_macro_cells(volym_ctx* c, const CellRange& r)
{
    hipLaunchKernelGGL(volym_macrocell_kernel, dim3(r.cn[0] * r.cn[1] * r.cn[2]), dim3(256), 0, c->slot0().stream, c->d_vol, c->d_mc, c->nx, c->ny, c->nz, c->mc_n,
                       c->bricked ? 1u : 0u, r);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

// the fine maxima (the grid of the tile mask and the depth bounds) of one range of fine cells, on slot 0's stream
static int launch_fine_cells(volym_ctx* c, const CellRange& r)
{
    const uint32_t total = r.cn[0] * r.cn[1] * r.cn[2];
    hipLaunchKernelGGL(volym_fine_cell_kernel, dim3((total + 255u) / 256u), dim3(256), 0, c->slot0().stream, c->d_vol, c->d_mc_fine, c->nx, c->ny, c->nz, c->fine_n,
                       c->bricked ? 1u : 0u, r);
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

// The cells of a grid of n_cells per axis whose voxel range (slack included) meets box {x0, y0, z0, x1, y1, z1}; false: none
static bool cells_meeting_box(const volym_ctx* c, uint32_t n_cells, const uint32_t box[6], CellRange& r)
{
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    for (int a = 0; a < 3; ++a) {
        uint32_t c0 = 0, c1 = 0;
        (void)volym_cells_meeting_box(n_cells, dims[a], box[a], box[3 + a], &c0, &c1);
        if (c0 >= c1) return false;
        r.c0[a] = c0; r.cn[a] = c1 - c0;
    }
    return true;
}

// The host's copy of the maxima (behind the launches on slot 0's stream that wrote them) and the occupied-cell AABB for every
// threshold byte.  Blocks.
static int read_macro_cells(volym_ctx* c)
{
    const uint32_t n = c->mc_n, cells = n * n * n;
    const hipStream_t stream = c->slot0().stream;
    c->h_mc.resize(cells);
    HIPCHK(c, hipMemcpyAsync(c->h_mc.data(), c->d_mc, cells, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    // AABB of the cells whose maximum reaches b, for every b: boxes of the cells with maximum exactly v, then a suffix union
    int box[257][6];
    for (int v = 0; v <= 256; ++v) { box[v][0] = box[v][1] = box[v][2] = 1 << 30; box[v][3] = box[v][4] = box[v][5] = -1; }
    for (uint32_t z = 0; z < n; ++z)
        for (uint32_t y = 0; y < n; ++y)
            for (uint32_t x = 0; x < n; ++x) {
                int* b = box[c->h_mc[(z * n + y) * n + x]];
                const int p[3] = {static_cast<int>(x), static_cast<int>(y), static_cast<int>(z)};
                for (int i = 0; i < 3; ++i) { b[i] = std::min(b[i], p[i]); b[3 + i] = std::max(b[3 + i], p[i]); }
            }
    int run[6] = {1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
    for (int i = 0; i < 6; ++i) c->aabb_tab[256][i] = i < 3 ? 0 : -1;         // threshold byte 256: nothing is dense
    for (int v = 255; v >= 0; --v) {
        for (int i = 0; i < 3; ++i) { run[i] = std::min(run[i], box[v][i]); run[3 + i] = std::max(run[3 + i], box[v][3 + i]); }
        for (int i = 0; i < 6; ++i) c->aabb_tab[v][i] = run[3] < 0 ? (i < 3 ? 0 : -1) : run[i];
    }
    return VOLYM_OK;
}

// Macro-cell maxima, their host copy and the occupied-cell AABB for every threshold byte (set-up path: blocks).
int volym::build_macro_cells(volym_ctx* c)
{
    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    // (every slot is idle: nothing reads the shared maxima or a slot's distance field).  Until every buffer below is rebuilt
    // there is no volume to march: a failure leaves the context asking for volym_set_volume and volym_update again
    const bool had_frame = c->have_frame;
    c->have_vol = c->have_frame = false;
    if (c->d_mc) { HIPCHK(c, hipFree(c->d_mc)); c->d_mc = nullptr; }
    const uint32_t n = c->mc_n, cells = n * n * n;
    hipError_t e = hipMalloc(&c->d_mc, cells);
    for (int i = 0; i < c->n_slots(); ++i) {
        FrameSlot& s = *c->slots[i];
        if (s.d_df) { HIPCHK(c, hipFree(s.d_df)); s.d_df = nullptr; }
        if (e == hipSuccess) e = hipMalloc(&s.d_df, (cells / 2u + 15u) / 16u * 16u);
        s.df_thr_byte = 0xffffffffu;
        s.hull_dirty = true;
    }
    if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(macro cells): ") + hipGetErrorString(e));
    rc = launch_macro_cells(c, CellRange{{0u, 0u, 0u}, {n, n, n}});
    if (rc == VOLYM_OK) rc = launch_fine_grid(c);
    if (rc == VOLYM_OK) rc = read_macro_cells(c);         // (waits for the stream: the fine maxima are there too)
    if (rc != VOLYM_OK) return rc;
    c->have_vol = true;
    c->have_frame = had_frame;
    return VOLYM_OK;
}

// The grid of the per-view tile mask and depth bounds for the volume's dimensions, mc_n and VOLYM_OPT_BOUNDS_CELLS: d_mc_fine and
// fine_n, or no grid of its own (d_mc_fine NULL, fine_n = mc_n) where the two coincide.  Every slot is idle.  Enqueues on slot
// 0's stream and does not wait.
static int launch_fine_grid(volym_ctx* c)
{
    if (c->d_mc_fine) { HIPCHK(c, hipFree(c->d_mc_fine)); c->d_mc_fine = nullptr; }
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    uint32_t n = c->bounds_cells < 0 ? volym_bounds_cells_for(dims, c->mc_n) : static_cast<uint32_t>(c->bounds_cells);
    n = std::max(n, c->mc_n);                        // (0, the macro-cell grid; an explicit value from before mc_n grew)
    c->fine_n = n;
    for (int i = 0; i < c->n_slots(); ++i) c->slots[i]->hull_dirty = true;
    if (n == c->mc_n) return VOLYM_OK;
    const hipError_t e = hipMalloc(&c->d_mc_fine, static_cast<size_t>(n) * n * n);
    if (e != hipSuccess) { c->d_mc_fine = nullptr; c->fine_n = c->mc_n; return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(fine cells): ") + hipGetErrorString(e)); }
    return launch_fine_cells(c, CellRange{{0u, 0u, 0u}, {n, n, n}});
}

// VOLYM_OPT_BOUNDS_CELLS changed: the fine grid alone, for the volume the context holds (set-up path: blocks)
int volym::build_fine_cells(volym_ctx* c)
{
    int rc = quiesce_slots(c);
    if (rc == VOLYM_OK) rc = launch_fine_grid(c);
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->slot0().stream));       // every slot's next view reads the new grid
    return VOLYM_OK;
}

// The maxima of the macro cells and of the fine cells whose voxel range (slack included) meets one of n boxes of rewritten texels
// (the others cover no texel that changed), the macro cells' host copy and the occupied-cell boxes; every slot's distance field and hulls become stale.
static int refresh_macro_cells(volym_ctx* c, const uint32_t (*boxes)[6], uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        CellRange r;
        // (the fine cells nest in the macro cells, voxel ranges included: where no macro cell meets the box, no fine cell does)
        if (!cells_meeting_box(c, c->mc_n, boxes[i], r)) continue;
        int rc = launch_macro_cells(c, r);
        if (rc == VOLYM_OK && c->d_mc_fine && cells_meeting_box(c, c->fine_n, boxes[i], r)) rc = launch_fine_cells(c, r);
        if (rc != VOLYM_OK) return rc;
    }
    const int rc = read_macro_cells(c);
    if (rc != VOLYM_OK) return rc;
    for (int i = 0; i < c->n_slots(); ++i) { c->slots[i]->df_thr_byte = 0xffffffffu; c->slots[i]->hull_dirty = true; }
    return VOLYM_OK;
}

// ---- crop box, clip plane and segment visibility on the device --------------------------------------------------------
// A frame with crop box B, clip plane P and mask `visible` is the frame of the scene whose density and importance bytes are 0
// outside B, on the cut side of P and in every texel of a hidden label.  The march kernels know nothing of any of them: they
// read d_vol and d_imp, and the set-up calls rewrite those from an uncropped source so that the invariant of context.hpp holds
// for the scene's (box, plane, mask).  One function does that, retarget: it moves the buffers from the invariant of one
// (box, plane, mask) to that of another and rewrites only the texels whose state can differ between the two -- the slabs
// between the boxes (volym_crop_slabs: at most six, one per face that moved), the boxes of the labels whose flag flipped
// (volym_visibility_boxes; volym_visibility_kernel skips every chunk in there that holds no texel of such a label) and the box
// of the texels the two planes classify differently (volym_clip_plane_box; volym_clip_plane_kernel skips every chunk in there
// in which no texel changes side).  Everything derived from the bytes follows: the macro cells the
// rewritten boxes touch, the occupied-cell boxes, every slot's distance field, hulls, tile mask and depth bounds (rebuilt by
// the next launch), the look-ahead's reject box, the work lists.

extern "C" {

int volym_crop_slabs(const uint32_t old_lo[3], const uint32_t old_hi[3], const uint32_t new_lo[3], const uint32_t new_hi[3], uint32_t slabs[6][6],
                     uint32_t* n_slabs)
{
    if (!old_lo || !old_hi || !new_lo || !new_hi || !slabs || !n_slabs) return VOLYM_E_INVALID;
    bool old_empty = false, new_empty = false;
    for (int a = 0; a < 3; ++a) {
        if (old_lo[a] > old_hi[a] || new_lo[a] > new_hi[a]) return VOLYM_E_INVALID;
        old_empty = old_empty || old_lo[a] == old_hi[a];
        new_empty = new_empty || new_lo[a] == new_hi[a];
    }
    uint32_t n = 0;
    auto push = [&](const uint32_t lo[3], const uint32_t hi[3]) {
        for (int a = 0; a < 3; ++a) if (lo[a] >= hi[a]) return;
        for (int a = 0; a < 3; ++a) { slabs[n][a] = lo[a]; slabs[n][3 + a] = hi[a]; }
        ++n;
    };
    if (old_empty || new_empty) {
        // to or from nothing: the other box is the whole difference
        if (!new_empty) push(new_lo, new_hi);
        if (!old_empty) push(old_lo, old_hi);
    } else {
        // a texel of one box that is not in the other lies, on some axis, between the two positions of a face; on the other axes
        // it lies within its own box, so within the union of the two extents
        uint32_t ulo[3], uhi[3];
        for (int a = 0; a < 3; ++a) { ulo[a] = std::min(old_lo[a], new_lo[a]); uhi[a] = std::max(old_hi[a], new_hi[a]); }
        for (int a = 0; a < 3; ++a) {
            uint32_t lo[3] = {ulo[0], ulo[1], ulo[2]}, hi[3] = {uhi[0], uhi[1], uhi[2]};
            lo[a] = std::min(old_lo[a], new_lo[a]); hi[a] = std::max(old_lo[a], new_lo[a]);
            push(lo, hi);
            lo[a] = std::min(old_hi[a], new_hi[a]); hi[a] = std::max(old_hi[a], new_hi[a]);
            push(lo, hi);
        }
    }
    *n_slabs = n;
    return VOLYM_OK;
}

int volym_visibility_boxes(const uint8_t flipped[256], const uint64_t counts[256], const int32_t label_boxes[256][6], const uint32_t crop_lo[3],
                           const uint32_t crop_hi[3], uint32_t boxes[VOLYM_VISIBILITY_MAX_BOXES][6], uint32_t* n_boxes)
{
    if (!flipped || !counts || !label_boxes || !crop_lo || !crop_hi || !boxes || !n_boxes) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a) if (crop_lo[a] > crop_hi[a]) return VOLYM_E_INVALID;
    auto volume = [](const uint32_t b[6]) { return static_cast<uint64_t>(b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]); };
    auto hull = [](const uint32_t p[6], const uint32_t q[6], uint32_t out[6]) {
        for (int a = 0; a < 3; ++a) { out[a] = std::min(p[a], q[a]); out[3 + a] = std::max(p[3 + a], q[3 + a]); }
    };
    uint32_t n = 0;
    for (int l = 0; l < 256; ++l) {
        if (!flipped[l] || counts[l] == 0u) continue;
        uint32_t b[6];
        bool empty = false;
        for (int a = 0; a < 3; ++a) {
            if (label_boxes[l][a] < 0 || label_boxes[l][3 + a] < label_boxes[l][a]) return VOLYM_E_INVALID;
            b[a] = std::max(static_cast<uint32_t>(label_boxes[l][a]), crop_lo[a]);
            b[3 + a] = std::min(static_cast<uint32_t>(label_boxes[l][3 + a]) + 1u, crop_hi[a]);
            empty = empty || b[a] >= b[3 + a];
        }
        if (empty) continue;
        // into the first box whose hull with this one holds no more texels than the two apart; else a box of its own while there
        // is room; else into the box that grows least
        uint32_t h[6], best = n;
        uint64_t best_growth = ~0ull;
        for (uint32_t i = 0; i < n; ++i) {
            hull(boxes[i], b, h);
            const uint64_t hv = volume(h), vi = volume(boxes[i]);
            if (hv <= vi + volume(b)) { best = i; break; }
            if (n == VOLYM_VISIBILITY_MAX_BOXES && hv - vi < best_growth) { best_growth = hv - vi; best = i; }
        }
        if (best == n) { std::memcpy(boxes[n++], b, sizeof b); continue; }
        hull(boxes[best], b, h);
        std::memcpy(boxes[best], h, sizeof h);
    }
    // boxes that grew may now pay to merge with each other
    for (bool merged = true; merged;) {
        merged = false;
        for (uint32_t i = 0; i < n && !merged; ++i)
            for (uint32_t j = i + 1u; j < n && !merged; ++j) {
                uint32_t h[6];
                hull(boxes[i], boxes[j], h);
                if (volume(h) > volume(boxes[i]) + volume(boxes[j])) continue;
                std::memcpy(boxes[i], h, sizeof h);
                std::memcpy(boxes[j], boxes[n - 1u], sizeof h);
                --n;
                merged = true;
            }
    }
    *n_boxes = n;
    return VOLYM_OK;
}

static bool valid_plane(const int32_t n[3], int32_t d)
{
    for (int a = 0; a < 3; ++a) if (n[a] < -VOLYM_CLIP_PLANE_MAX || n[a] > VOLYM_CLIP_PLANE_MAX) return false;
    return n[0] != 0 || n[1] != 0 || n[2] != 0 || d == 0;
}

static int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// the texels x of [lo, hi) with n0 * x <= r, as an interval [x0, x1) (x0 == x1 == lo: none)
static void kept_run(int64_t n0, int64_t r, int64_t lo, int64_t hi, int64_t& x0, int64_t& x1)
{
    x0 = lo; x1 = hi;
    if (n0 > 0) x1 = std::min(hi, floor_div(r, n0) + 1);
    else if (n0 < 0) x0 = std::max(lo, -floor_div(r, -n0));        // x >= ceil(r / n0) = -floor(r / -n0)
    else if (r < 0) x1 = lo;
    if (x1 <= x0) x0 = x1 = lo;
}

int volym_clip_plane_box(const int32_t old_n[3], int32_t old_d, const int32_t new_n[3], int32_t new_d, const uint32_t lo[3], const uint32_t hi[3],
                         uint32_t box[6], uint32_t* n_boxes)
{
    if (!old_n || !new_n || !lo || !hi || !box || !n_boxes) return VOLYM_E_INVALID;
    if (!valid_plane(old_n, old_d) || !valid_plane(new_n, new_d)) return VOLYM_E_INVALID;
    for (int a = 0; a < 3; ++a) if (lo[a] > hi[a] || hi[a] > 65536u) return VOLYM_E_INVALID;
    *n_boxes = 0;
    const bool equal = old_d == new_d && old_n[0] == new_n[0] && old_n[1] == new_n[1] && old_n[2] == new_n[2];
    if (equal || lo[0] == hi[0] || lo[1] == hi[1] || lo[2] == hi[2]) return VOLYM_OK;
    // Shrink [lo, hi) from every face while the outer slice there is one over which both predicates are constant and equal: a
    // texel the planes classify differently lies in no such slice, so it stays inside.  n . t over a slice is linear, so its
    // extremes are exact: the predicate is true throughout when the maximum is <= d, false throughout when the minimum is > d.
    // A slice of a narrower box may be clean where that of the wider one was not: repeat until no face moves.
    uint32_t b[6] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    const auto state = [&](const int32_t n[3], int32_t d, int a, uint32_t i) {
        int64_t mn = static_cast<int64_t>(n[a]) * i, mx = mn;
        for (int o = 0; o < 3; ++o) {
            if (o == a) continue;
            const int64_t p = static_cast<int64_t>(n[o]) * b[o], q = static_cast<int64_t>(n[o]) * (b[3 + o] - 1u);
            mn += std::min(p, q); mx += std::max(p, q);
        }
        return mx <= d ? 1 : mn > d ? 0 : 2;
    };
    const auto clean = [&](int a, uint32_t i) {
        const int so = state(old_n, old_d, a, i);
        return so != 2 && so == state(new_n, new_d, a, i);
    };
    for (bool moved = true; moved;) {
        moved = false;
        for (int a = 0; a < 3; ++a) {
            while (b[a] < b[3 + a] && clean(a, b[a])) { ++b[a]; moved = true; }
            while (b[a] < b[3 + a] && clean(a, b[3 + a] - 1u)) { --b[3 + a]; moved = true; }
            if (b[a] == b[3 + a]) return VOLYM_OK;
        }
    }
    // Two planes may still keep the same texels there (3x <= 2 and x <= 0): no box then.  Exact, a row at a time along the longest
    // axis, where each plane keeps an interval; it ends at the first row whose two intervals differ.
    int ax = 0;
    for (int a = 1; a < 3; ++a) if (b[3 + a] - b[a] > b[3 + ax] - b[ax]) ax = a;
    const int u = (ax + 1) % 3, v = (ax + 2) % 3;
    for (uint32_t j = b[v]; j < b[3 + v]; ++j)
        for (uint32_t i = b[u]; i < b[3 + u]; ++i) {
            const int64_t ro = static_cast<int64_t>(old_d) - static_cast<int64_t>(old_n[u]) * i - static_cast<int64_t>(old_n[v]) * j;
            const int64_t rn = static_cast<int64_t>(new_d) - static_cast<int64_t>(new_n[u]) * i - static_cast<int64_t>(new_n[v]) * j;
            int64_t o0, o1, n0, n1;
            kept_run(old_n[ax], ro, b[ax], b[3 + ax], o0, o1);
            kept_run(new_n[ax], rn, b[ax], b[3 + ax], n0, n1);
            if (o0 == n0 && o1 == n1) continue;
            std::memcpy(box, b, sizeof b);
            *n_boxes = 1;
            return VOLYM_OK;
        }
    return VOLYM_OK;
}

}  // extern "C"

static bool crop_active(const volym_ctx* c)
{
    return c->crop_lo[0] != 0u || c->crop_lo[1] != 0u || c->crop_lo[2] != 0u || c->crop_hi[0] != c->nx || c->crop_hi[1] != c->ny || c->crop_hi[2] != c->nz;
}

static bool plane_active(const volym_ctx* c) { return c->clip_n[0] != 0 || c->clip_n[1] != 0 || c->clip_n[2] != 0; }

bool volym::imp_croppable(const volym_ctx* c)
{
    return c->have_vol && c->have_imp && c->d_imp && c->inx == c->nx && c->iny == c->ny && c->inz == c->nz;
}

static bool imp_from_labels(const volym_ctx* c) { return c->d_labels && c->have_seg_table; }

// a hidden label that has voxels (hiding label values no voxel carries changes no byte)
bool volym::mask_active(const volym_ctx* c)
{
    for (int l = 0; l < 256; ++l) if (c->seg_hidden[l] && c->label_count[l] != 0u) return true;
    return false;
}

// A buffer the march reads and the untouched bytes it is cut from.  table != NULL: src holds labels, mapped through it.
struct Derived { uint8_t* dst; const uint8_t* src; const uint8_t* table; bool bricked; };

static Derived density_of(const volym_ctx* c) { return {c->d_vol, c->d_vol0, nullptr, c->bricked}; }

// the importances' uncut bytes: the labels through seg_table when a table has been set since the labels, else the copy d_imp0
static Derived importances_of(const volym_ctx* c)
{
    if (imp_from_labels(c)) return {c->d_imp, c->d_labels, c->seg_table, c->imp_bricked};
    return {c->d_imp, c->d_imp0, nullptr, c->imp_bricked};
}

// The part of the scene state the invariant depends on: crop box [lo, hi), clip plane (kept: n . t <= d) and mask (hidden[l] is
// 0 or 1).
namespace volym { struct SceneCut { uint32_t lo[3], hi[3]; int32_t n[3], d; uint8_t hidden[256]; }; }

static bool same_plane(const SceneCut& a, const SceneCut& b) { return a.d == b.d && a.n[0] == b.n[0] && a.n[1] == b.n[1] && a.n[2] == b.n[2]; }

// the walk of the rewrite kernels over one box [box[0..2], box[3..5]) of a volume in the given layout; returns its items.
// moved_from: the box is that of a plane edit, and the walk also carries the plane the bytes were clipped to before.
uint64_t volym::make_crop_slab(const volym_ctx* c, bool bricked, const uint32_t box[6], const SceneCut* moved_from, CropSlab& s)
{
    s = CropSlab{};
    for (int a = 0; a < 3; ++a) { s.lo[a] = box[a]; s.hi[a] = box[3 + a]; s.box_lo[a] = c->crop_lo[a]; s.box_hi[a] = c->crop_hi[a]; }
    for (int a = 0; a < 3; ++a) { s.pn[a] = c->clip_n[a]; s.qn[a] = moved_from ? moved_from->n[a] : 0; }
    s.pd = c->clip_d; s.qd = moved_from ? moved_from->d : 0;
    s.planes = plane_active(c) || moved_from ? 1u : 0u;
    uint64_t items;
    if (bricked) {
        for (int a = 0; a < 3; ++a) { s.b_lo[a] = s.lo[a] >> 2; s.b_n[a] = ((s.hi[a] + 3u) >> 2) - s.b_lo[a]; }
        items = 4ull * s.b_n[0] * s.b_n[1] * s.b_n[2];
    } else {
        const bool rows = s.lo[0] == 0u && s.hi[0] == c->nx, slices = rows && s.lo[1] == 0u && s.hi[1] == c->ny;
        uint64_t run = s.hi[0] - s.lo[0];
        s.runs_y = s.hi[1] - s.lo[1]; s.runs_z = s.hi[2] - s.lo[2];
        if (rows) { run *= s.runs_y; s.runs_y = 1u; }
        if (slices) { run *= s.runs_z; s.runs_z = 1u; }
        s.run_len = static_cast<uint32_t>(run);                       // (a volume has fewer than 2^32 bytes: upload_volume)
        s.chunks_per_run = static_cast<uint32_t>((run + 15u) / 16u) + 1u;
        items = static_cast<uint64_t>(s.chunks_per_run) * s.runs_y * s.runs_z;
    }
    return items;
}

// d.dst = (inside(c->crop) && kept by c->clip && !c->seg_hidden[label]) ? value(d.src) : 0 over one box of texels, on slot 0's
// stream.  flipped: only the chunks that hold a texel of such a label are rewritten.  moved_from: only the chunks in which a
// texel lies on different sides of that cut's plane and the context's.  Both NULL: every chunk, by volym_crop_slab_kernel while
// no segment is hidden (a context that hides nothing runs what it always ran), else by the kernel that reads the labels as
// well, with every label marked flipped.
static int rewrite(volym_ctx* c, const Derived& d, const uint32_t box[6], const uint8_t* flipped, const SceneCut* moved_from)
{
    CropSlab s;
    const uint64_t items = make_crop_slab(c, d.bricked, box, moved_from, s);
    if (items == 0u) return VOLYM_OK;
    LabelTable t = {}, m = {};
    if (d.table) std::memcpy(t.v, d.table, 256);
    const hipStream_t stream = c->slot0().stream;
    const dim3 grid(stream_grid(c, items));
    const uint4* src = reinterpret_cast<const uint4*>(d.src);
    uint4* dst = reinterpret_cast<uint4*>(d.dst);
    const uint32_t bricked = d.bricked ? 1u : 0u, n_items = static_cast<uint32_t>(items);
    if (moved_from) {
        const bool masked = mask_active(c);
        for (int l = 0; l < 256; ++l) m.v[l] = c->seg_hidden[l] ? 0u : 1u;
        const auto kernel = d.table ? (masked ? volym_clip_plane_kernel<true, true> : volym_clip_plane_kernel<true, false>)
                                    : (masked ? volym_clip_plane_kernel<false, true> : volym_clip_plane_kernel<false, false>);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, reinterpret_cast<const uint4*>(c->d_labels), src, dst, t, m, s, c->nx, c->ny, c->nz, bricked, n_items);
    } else if (!flipped && !mask_active(c)) {
        const auto kernel = d.table ? volym_crop_slab_kernel<true> : volym_crop_slab_kernel<false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, src, dst, t, s, c->nx, c->ny, c->nz, bricked, n_items);
    } else {
        for (int l = 0; l < 256; ++l) m.v[l] = static_cast<uint8_t>((c->seg_hidden[l] ? 0u : 1u) | ((!flipped || flipped[l]) ? 2u : 0u));
        // (with a table the labels are the source themselves)
        const auto kernel = d.table ? volym_visibility_kernel<true> : volym_visibility_kernel<false>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, reinterpret_cast<const uint4*>(c->d_labels), src, dst, t, m, s, c->nx, c->ny, c->nz, bricked, n_items);
    }
    HIPCHK(c, hipGetLastError());
    return VOLYM_OK;
}

// The uncropped copies a cut needs and the context does not hold yet.  Only called while the bytes they are copied from are
// uncut (the box is the whole volume and nothing is hidden, or the buffer has just been uploaded).  Device-to-device on slot
// 0's stream (the slots are at rest): a device-to-device copy is not waited for by the host and the slots' streams do not wait
// for the NULL stream, so only stream order puts the copy before the kernels that rewrite its source, and the
// hipStreamSynchronize that ends retarget covers it.
int volym::ensure_uncropped_copies(volym_ctx* c, bool vol)
{
    if (vol && !c->d_vol0) {
        const uint64_t nb = layout_bytes(c->bricked, c->nx, c->ny, c->nz) + 16u;
        hipError_t e = hipMalloc(&c->d_vol0, nb);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_vol0, c->d_vol, nb, hipMemcpyDeviceToDevice, c->slot0().stream);
        if (e != hipSuccess) { (void)hipFree(c->d_vol0); c->d_vol0 = nullptr; return fail(c, VOLYM_E_NOMEM, std::string("crop box (density copy): ") + hipGetErrorString(e)); }
    }
    if (imp_croppable(c) && !imp_from_labels(c) && !c->d_imp0) {
        hipError_t e = hipMalloc(&c->d_imp0, c->imp_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(c->d_imp0, c->d_imp, c->imp_bytes, hipMemcpyDeviceToDevice, c->slot0().stream);
        if (e != hipSuccess) { (void)hipFree(c->d_imp0); c->d_imp0 = nullptr; return fail(c, VOLYM_E_NOMEM, std::string("crop box (importance copy): ") + hipGetErrorString(e)); }
    }
    return VOLYM_OK;
}

// imp_box0_* of importances mapped from the labels: the union of the boxes of the labels the table makes important and the
// mask shows -- what important_texel_box would find in the mapped bytes, or a box around it
static void segment_important_box(volym_ctx* c)
{
    int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {-1, -1, -1};
    for (int l = 0; l < 256; ++l) {
        if (c->seg_table[l] < 128u || c->seg_hidden[l] || c->label_count[l] == 0u) continue;
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c->label_box[l][a]); hi[a] = std::max(hi[a], c->label_box[l][3 + a]); }
    }
    for (int a = 0; a < 3; ++a) {
        if (hi[0] < 0) { c->imp_box0_lo[a] = 1; c->imp_box0_hi[a] = 0; continue; }
        c->imp_box0_lo[a] = lo[a]; c->imp_box0_hi[a] = hi[a];
    }
}

// imp_box_* = the uncropped importances' box cut to the crop box: the cropped importances have nothing important outside it
static void crop_important_box(volym_ctx* c)
{
    bool none = c->imp_box0_lo[0] > c->imp_box0_hi[0];
    for (int a = 0; a < 3; ++a) {
        c->imp_box_lo[a] = c->imp_box0_lo[a]; c->imp_box_hi[a] = c->imp_box0_hi[a];
        if (none || !imp_croppable(c)) continue;
        c->imp_box_lo[a] = std::max(c->imp_box_lo[a], static_cast<int>(c->crop_lo[a]));
        c->imp_box_hi[a] = std::min(c->imp_box_hi[a], static_cast<int>(c->crop_hi[a]) - 1);
        none = c->imp_box_lo[a] > c->imp_box_hi[a];
    }
    if (none) for (int a = 0; a < 3; ++a) { c->imp_box_lo[a] = 1; c->imp_box_hi[a] = 0; }
    // the frames enqueued from here on march the new box, with or without a volym_update in between
    for (int i = 0; i < c->n_slots(); ++i) set_reject_box(c, c->slots[i]->fp);
}

static SceneCut current_cut(const volym_ctx* c)
{
    SceneCut s;
    for (int a = 0; a < 3; ++a) { s.lo[a] = c->crop_lo[a]; s.hi[a] = c->crop_hi[a]; s.n[a] = c->clip_n[a]; }
    s.d = c->clip_d;
    std::memcpy(s.hidden, c->seg_hidden, sizeof s.hidden);
    return s;
}

static SceneCut all_visible(SceneCut s)
{
    std::memset(s.hidden, 0, sizeof s.hidden);
    return s;
}

// the whole volume, no plane, nothing hidden: the bytes as they were uploaded
static SceneCut uncut(const volym_ctx* c)
{
    SceneCut s = all_visible(current_cut(c));
    s.lo[0] = s.lo[1] = s.lo[2] = 0u;
    s.hi[0] = c->nx; s.hi[1] = c->ny; s.hi[2] = c->nz;
    s.n[0] = s.n[1] = s.n[2] = s.d = 0;
    return s;
}

// The box inside both cuts' crop boxes that holds every texel their planes classify differently (outside `from`'s box a texel
// of `to`'s lies in a slab).  moved false: there is no such texel.  A transition works it out once (two planes that keep the
// same texels cost volym_clip_plane_box a pass over the rows of the box).
struct PlaneMove { bool moved; uint32_t box[6]; };

static PlaneMove plane_move(const SceneCut& from, const SceneCut& to)
{
    PlaneMove m = {};
    if (same_plane(from, to)) return m;
    uint32_t lo[3], hi[3], n = 0;
    for (int a = 0; a < 3; ++a) { lo[a] = std::max(from.lo[a], to.lo[a]); hi[a] = std::max(std::min(from.hi[a], to.hi[a]), lo[a]); }
    (void)volym_clip_plane_box(from.n, from.d, to.n, to.d, lo, hi, m.box, &n);
    m.moved = n != 0u;
    return m;
}

// Does some texel of a buffer that takes part (the importances; with vol the density too) differ between the two?  Not without
// a volume (after a failed edit the bytes belong to no state and only volym_set_volume mends them), not for importances of other
// dimensions than the volume's (they are never cut), not for the same box, planes that keep the same texels of it and flags that
// differ only in labels without voxels.
static bool cuts_differ(const volym_ctx* c, const SceneCut& from, const SceneCut& to, const PlaneMove& plane, bool vol)
{
    if (!c->have_vol || !(vol || imp_croppable(c))) return false;
    for (int a = 0; a < 3; ++a) if (from.lo[a] != to.lo[a] || from.hi[a] != to.hi[a]) return true;
    if (plane.moved) return true;
    for (int l = 0; l < 256; ++l) if (from.hidden[l] != to.hidden[l] && c->label_count[l] != 0u) return true;
    return false;
}

// The one function that keeps the invariant of context.hpp.  Precondition: the importances (with vol: and the density) hold it
// for `from`.  Postcondition: they hold it for `to`, which is the context's crop box, clip plane and mask, and everything derived
// from the bytes is up to date.  Blocking set-up path; while `to` hides a label the caller has checked that the labels fit the
// volume.  Every chunk that is stored is stored by the full rule of `to`, so the three groups of boxes may overlap and their order
// does not matter.  A failure before the first launch leaves the context as it was; one after it leaves bytes that belong to
// neither state: the context then asks for volym_set_volume again (have_vol false), or, where only the importances were being
// rewritten, for the importances.  rewrote (if not NULL): whether any byte could differ, i.e. whether the transition ran.
static int retarget(volym_ctx* c, const SceneCut& from, const SceneCut& to, bool vol, bool* rewrote = nullptr)
{
    const PlaneMove plane = plane_move(from, to);
    const bool idle = !cuts_differ(c, from, to, plane, vol);
    if (rewrote) *rewrote = !idle;
    if (!idle) {
        int rc = quiesce_slots(c);
        if (rc == VOLYM_OK) rc = ensure_uncropped_copies(c, vol);      // in stream order in front of the rewrites
        if (rc != VOLYM_OK) return rc;
        if (vol) ++c->scene_serial;                                    // density bytes change: a surface pass is stale
    }
    for (int a = 0; a < 3; ++a) { c->crop_lo[a] = to.lo[a]; c->crop_hi[a] = to.hi[a]; c->clip_n[a] = to.n[a]; }
    c->clip_d = to.d;
    std::memcpy(c->seg_hidden, to.hidden, sizeof c->seg_hidden);
    if (idle) {
        crop_important_box(c);       // (host arithmetic: fresh importances on a plain context get their box and reject boxes here)
        return VOLYM_OK;
    }
    const auto work = [&]() -> int {
        // the slabs between the two boxes, then the boxes of the flipped labels inside both (outside `from`'s box a texel of
        // `to`'s lies in a slab and has its final bytes already), then the box of the texels that change side of the plane
        uint32_t boxes[6 + VOLYM_VISIBILITY_MAX_BOXES + 1][6], n_slabs = 0, n_flipped = 0, lo[3], hi[3];
        uint8_t flipped[256];
        (void)volym_crop_slabs(from.lo, from.hi, to.lo, to.hi, boxes, &n_slabs);
        for (int l = 0; l < 256; ++l) flipped[l] = from.hidden[l] != to.hidden[l];
        for (int a = 0; a < 3; ++a) { lo[a] = std::max(from.lo[a], to.lo[a]); hi[a] = std::max(std::min(from.hi[a], to.hi[a]), lo[a]); }
        (void)volym_visibility_boxes(flipped, c->label_count, c->label_box, lo, hi, boxes + n_slabs, &n_flipped);
        const uint32_t n_cut = n_slabs + n_flipped;
        const uint32_t n = n_cut + (plane.moved ? 1u : 0u);
        if (plane.moved) std::memcpy(boxes[n_cut], plane.box, sizeof plane.box);
        const bool imp = imp_croppable(c);
        int rc = VOLYM_OK;
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t* f = i < n_slabs || i >= n_cut ? nullptr : flipped;
            const SceneCut* moved_from = i < n_cut ? nullptr : &from;
            if (vol) rc = rewrite(c, density_of(c), boxes[i], f, moved_from);
            if (rc == VOLYM_OK && imp) rc = rewrite(c, importances_of(c), boxes[i], f, moved_from);
            if (rc != VOLYM_OK) return rc;
        }
        if (vol && n != 0u) {
            rc = refresh_macro_cells(c, boxes, n);
            if (rc != VOLYM_OK) return rc;
        }
        HIPCHK(c, hipStreamSynchronize(c->slot0().stream));       // every slot's next frame reads the new bytes
        if (imp_from_labels(c)) segment_important_box(c);          // (uploaded importances keep their box: it is conservative)
        crop_important_box(c);
        return rebuild_lists(c);
    };
    const int rc = work();
    if (rc != VOLYM_OK) {
        if (vol) c->have_vol = c->have_frame = false;
        else c->have_imp = false;
    }
    return rc;
}

// d_imp has just been filled with complete importances: cut them to the scene's box, plane and mask.  The work lists start over
// in any case (the costs describe the old importances; a transition that ran has rebuilt them).
static int cut_fresh_importances(volym_ctx* c)
{
    bool rewrote = false;
    int rc = retarget(c, uncut(c), current_cut(c), false, &rewrote);
    if (rc == VOLYM_OK && !rewrote) rc = rebuild_lists(c);
    if (rc != VOLYM_OK) c->have_imp = false;
    return rc;
}

// ---- segment importances on the device ---------------------------------------------------------------------------------
// The reference maps labels to importances on the host once (importance.rs:148-158) and uploads the result; an edit of one
// segment's importance would pay that again (a host pass, an upload and a host scan of the whole volume).  Here the labels stay
// on the device: volym_set_labels uploads them once and counts, per label value, its voxels and their texel AABB;
// volym_set_segment_importances maps them through a 256-byte table into d_imp (one HBM stream) and takes the important-texel
// box as the union of the boxes of the labels the table makes important -- exactly what important_texel_box would find.

// dst (in the labels' layout) = table[labels], on slot 0's stream; waits for it
static int launch_segment_map(volym_ctx* c, const uint8_t table[256], uint8_t* dst)
{
    LabelTable t;
    std::memcpy(t.v, table, 256);
    const uint64_t n_chunks = (layout_bytes(c->labels_bricked, c->lnx, c->lny, c->lnz) + 15u) / 16u;
    const hipStream_t stream = c->slot0().stream;
    hipLaunchKernelGGL(volym_segment_map_kernel, dim3(stream_grid(c, n_chunks)), dim3(256), 0, stream, reinterpret_cast<const uint4*>(c->d_labels),
                       reinterpret_cast<uint4*>(dst), t, c->lnx, c->lny, c->lnz, c->labels_bricked ? 1u : 0u, static_cast<uint32_t>(n_chunks));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(stream));       // every slot's next frame reads the new bytes
    return VOLYM_OK;
}

// AABB (texel indices) of the importances a look-ahead probe counts as important (byte >= 128, wgsl:133, :155).  Host scan,
// eight bytes at a time (bit 7 of a byte <=> the byte is >= 128); set-up path.
static void important_texel_box(const uint8_t* imp, uint32_t nx, uint32_t ny, uint32_t nz, int (&lo)[3], int (&hi)[3])
{
    int x0 = INT32_MAX, y0 = INT32_MAX, z0 = INT32_MAX, x1 = -1, y1 = -1, z1 = -1;
    for (uint32_t z = 0; z < nz; ++z)
        for (uint32_t y = 0; y < ny; ++y) {
            const uint8_t* row = imp + (static_cast<size_t>(z) * ny + y) * nx;
            int first = -1, last = -1;
            uint32_t x = 0;
            for (; x + 8u <= nx; x += 8u) {
                uint64_t w;
                std::memcpy(&w, row + x, 8);
                w &= 0x8080808080808080ull;
                if (!w) continue;
                if (first < 0) first = static_cast<int>(x) + (__builtin_ctzll(w) >> 3);
                last = static_cast<int>(x) + 7 - (__builtin_clzll(w) >> 3);
            }
            for (; x < nx; ++x)
                if (row[x] & 0x80u) { if (first < 0) first = static_cast<int>(x); last = static_cast<int>(x); }
            if (first < 0) continue;
            x0 = std::min(x0, first); x1 = std::max(x1, last);
            y0 = std::min(y0, static_cast<int>(y)); y1 = std::max(y1, static_cast<int>(y));
            z0 = std::min(z0, static_cast<int>(z)); z1 = std::max(z1, static_cast<int>(z));
        }
    if (x1 < 0) { lo[0] = lo[1] = lo[2] = 1; hi[0] = hi[1] = hi[2] = 0; return; }
    lo[0] = x0; lo[1] = y0; lo[2] = z0; hi[0] = x1; hi[1] = y1; hi[2] = z1;
}

// label_count and label_box of the labels on the device: one pass of volym_label_stats_kernel on slot 0's stream, waited for.  On
// failure the two are left as they were.
static hipError_t scan_label_stats(volym_ctx* c)
{
    const uint64_t n_chunks = (layout_bytes(c->labels_bricked, c->lnx, c->lny, c->lnz) + 15u) / 16u;
    // counts, then boxes: lo = INT_MAX, hi = -1 until a voxel says otherwise
    std::vector<unsigned char> init(256 * sizeof(unsigned long long) + 256 * 6 * sizeof(int));
    int* boxes = reinterpret_cast<int*>(init.data() + 256 * sizeof(unsigned long long));
    for (int l = 0; l < 256; ++l)
        for (int i = 0; i < 6; ++i) boxes[l * 6 + i] = i < 3 ? INT32_MAX : -1;
    unsigned char* d_stats = nullptr;
    const hipStream_t stream = c->slot0().stream;
    hipError_t e = hipMalloc(&d_stats, init.size());
    if (e == hipSuccess) e = hipMemcpy(d_stats, init.data(), init.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(volym_label_stats_kernel, dim3(stream_grid(c, n_chunks)), dim3(256), 0, stream, reinterpret_cast<const uint4*>(c->d_labels),
                           reinterpret_cast<unsigned long long*>(d_stats), reinterpret_cast<int*>(d_stats + 256 * sizeof(unsigned long long)),
                           c->lnx, c->lny, c->lnz, c->labels_bricked ? 1u : 0u, static_cast<uint32_t>(n_chunks));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(init.data(), d_stats, init.size(), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_stats);
    if (e != hipSuccess) return e;
    std::memcpy(c->label_count, init.data(), sizeof c->label_count);
    std::memcpy(c->label_box, boxes, sizeof c->label_box);
    return hipSuccess;
}

// The counterpart of retarget for a change of labels under a (box, plane, mask) that stays -- an edit, an undo, a redo -- once the
// labels are stored and `res` names the labels that left and arrived and the hull of the changed texels (changed != 0).
// Precondition: density and importances held the invariant of context.hpp for the labels as they were.  Postcondition: they hold it
// for the labels as they are, label_count and label_box describe those, and everything derived from the bytes is up to date.
int volym::follow_labels(volym_ctx* c, const volym_relabel_result& res, const char* who)
{
    // counts and boxes first: mask_active and volym_visibility_boxes read them
    const hipError_t es = scan_label_stats(c);
    if (es != hipSuccess) return fail(c, VOLYM_E_HIP, std::string(who) + " (label statistics): " + hipGetErrorString(es));
    ++c->scene_serial;                                                    // labels changed: a surface pass is stale
    // A texel's bytes differ from the rule's only where its old and its new label differ in what they give: visibility for the
    // density, visibility and the table's byte for importances mapped from the labels.  Every such texel carries a label that
    // arrived, inside the result's box: the visibility kernel stores the chunks that hold one, whole, by the rule.
    uint8_t flipped[256];
    bool hidden_moved = false;
    for (int l = 0; l < 256; ++l) {
        flipped[l] = res.left[l] != 0u || res.arrived[l] != 0u;
        hidden_moved = hidden_moved || (flipped[l] && c->seg_hidden[l]);
    }
    int rc = VOLYM_OK;
    if (hidden_moved) rc = rewrite(c, density_of(c), res.box, flipped, nullptr);
    if (rc == VOLYM_OK && imp_croppable(c) && (imp_from_labels(c) || hidden_moved)) rc = rewrite(c, importances_of(c), res.box, flipped, nullptr);
    if (rc == VOLYM_OK && hidden_moved) rc = refresh_macro_cells(c, &res.box, 1u);
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->slot0().stream));                   // every slot's next frame reads the new bytes
    if (imp_from_labels(c)) segment_important_box(c);
    crop_important_box(c);
    return rebuild_lists(c);
}

// ---- C ABI: what each call makes of the scene's (box, plane, mask) ----------------------------------------------------
//   volym_set_crop_box(lo, hi)                  current -> (lo, hi), current plane and mask density and importances
//   volym_set_clip_plane(n, d)                  current -> current box and mask, (n, d)     density and importances
//   volym_set_segment_visibility(v)             current -> current box and plane, ~v        density and importances
//   volym_set_volume, before the upload         current -> whole volume, no plane, no mask  importances (the density is replaced)
//   volym_set_labels, volym_set_importances,
//     before they replace anything              current -> current box and plane, no mask   density and importances
//   volym_set_importances and
//     volym_set_segment_importances, after
//     the new bytes are in d_imp                whole volume, no plane, no mask -> current  importances

extern "C" {

int volym_set_crop_box(volym_ctx* c, const uint32_t lo[3], const uint32_t hi[3])
{
    if (!c) return VOLYM_E_INVALID;
    if (!lo || !hi) return fail(c, VOLYM_E_INVALID, "volym_set_crop_box: NULL box");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_set_crop_box: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    SceneCut to = current_cut(c);
    for (int a = 0; a < 3; ++a) {
        if (lo[a] > hi[a] || hi[a] > dims[a]) return fail(c, VOLYM_E_INVALID, "volym_set_crop_box: need lo <= hi <= volume size on every axis");
        to.lo[a] = lo[a]; to.hi[a] = hi[a];
    }
    return retarget(c, current_cut(c), to, true);
}

int volym_get_crop_box(volym_ctx* c, uint32_t lo[3], uint32_t hi[3])
{
    if (!c) return VOLYM_E_INVALID;
    if (!lo || !hi) return fail(c, VOLYM_E_INVALID, "volym_get_crop_box: NULL output");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_get_crop_box: no volume");
    for (int a = 0; a < 3; ++a) { lo[a] = c->crop_lo[a]; hi[a] = c->crop_hi[a]; }
    return VOLYM_OK;
}

int volym_set_clip_plane(volym_ctx* c, const int32_t n[3], int32_t d)
{
    if (!c) return VOLYM_E_INVALID;
    if (!n) return fail(c, VOLYM_E_INVALID, "volym_set_clip_plane: NULL normal");
    if (!valid_plane(n, d)) return fail(c, VOLYM_E_INVALID, "volym_set_clip_plane: need |n[a]| <= 4096 on every axis, and d == 0 with n == (0, 0, 0)");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_set_clip_plane: no volume (volym_set_volume first)");
    SceneCut to = current_cut(c);
    for (int a = 0; a < 3; ++a) to.n[a] = n[a];
    to.d = d;
    return retarget(c, current_cut(c), to, true);
}

int volym_get_clip_plane(volym_ctx* c, int32_t n[3], int32_t* d)
{
    if (!c) return VOLYM_E_INVALID;
    if (!n || !d) return fail(c, VOLYM_E_INVALID, "volym_get_clip_plane: NULL output");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_get_clip_plane: no volume");
    for (int a = 0; a < 3; ++a) n[a] = c->clip_n[a];
    *d = c->clip_d;
    return VOLYM_OK;
}

int volym_set_segment_visibility(volym_ctx* c, const uint8_t visible[256])
{
    if (!c) return VOLYM_E_INVALID;
    if (!visible) return fail(c, VOLYM_E_INVALID, "volym_set_segment_visibility: NULL table");
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_set_segment_visibility: no volume (volym_set_volume first)");
    if (!c->d_labels) return fail(c, VOLYM_E_STATE, "volym_set_segment_visibility: no labels (volym_set_labels first; volym_set_importances drops them)");
    if (c->lnx != c->nx || c->lny != c->ny || c->lnz != c->nz)
        return fail(c, VOLYM_E_STATE, "volym_set_segment_visibility: the labels' dimensions are not the volume's");
    if (c->labels_bricked != c->bricked || (imp_croppable(c) && c->imp_bricked != c->labels_bricked))
        return fail(c, VOLYM_E_STATE, "volym_set_segment_visibility: volume, importances and labels were uploaded under different VOLYM_OPT_VOLUME_LAYOUT settings");
    SceneCut to = current_cut(c);
    for (int l = 0; l < 256; ++l) to.hidden[l] = visible[l] ? 0u : 1u;
    return retarget(c, current_cut(c), to, true);
}

int volym_get_segment_visibility(volym_ctx* c, uint8_t visible[256])
{
    if (!c) return VOLYM_E_INVALID;
    if (!visible) return fail(c, VOLYM_E_INVALID, "volym_get_segment_visibility: NULL output");
    for (int l = 0; l < 256; ++l) visible[l] = c->seg_hidden[l] ? 0u : 1u;
    return VOLYM_OK;
}

int volym_set_volume(volym_ctx* c, const uint8_t* voxels, uint32_t nx, uint32_t ny, uint32_t nz, int filter)
{
    if (!c) return VOLYM_E_INVALID;
    if (filter != VOLYM_FILTER_NEAREST && filter != VOLYM_FILTER_LINEAR)
        return fail(c, VOLYM_E_INVALID, "volym_set_volume: filter must be VOLYM_FILTER_NEAREST or VOLYM_FILTER_LINEAR");
    clear_label_history(c);                 // (a step belongs to the scene it was recorded in)
    // The box goes back to the whole volume and the mask to all visible: the importances get their cut texels back (the density
    // is replaced below).  This runs before upload_volume has looked at its arguments: a call that then fails leaves box and mask
    // reset and no volume (have_vol false), which is what a failed volym_set_volume leaves in any case.
    int rc = retarget(c, current_cut(c), uncut(c), false);
    if (rc == VOLYM_OK) rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    // (d_imp is uncropped now, and the copies are made again by the next cut: a context that does not cut holds none)
    if (c->d_vol0) { HIPCHK(c, hipFree(c->d_vol0)); c->d_vol0 = nullptr; }
    if (c->d_imp0) { HIPCHK(c, hipFree(c->d_imp0)); c->d_imp0 = nullptr; }
    c->measure.count = 0;                   // (a result describes the volume it was measured in)
    free_surface(c);                        // (and so do a surface's summary, row offsets and faces, which are sized by it)
    free_components(c);                     // (and the components' snapshot: its ids address texels of the old volume)
    free_distance(c);                       // (and the distance map, for the same reason)
    free_nearest(c);                        // (and the nearest pass's sites)
    free_geodesic(c);                       // (and the geodesic pass's keys)
    free_cost(c);                           // (and the cost pass's keys and bytes)
    free_interpolate(c);                    // (and the interpolate pass's maps)
    rc = upload_volume(c, &c->d_vol, voxels, nx, ny, nz);
    if (rc != VOLYM_OK) { c->have_vol = false; return rc; }
    c->nx = nx; c->ny = ny; c->nz = nz; c->filter = filter;
    for (int a = 0; a < 3; ++a) { c->crop_lo[a] = 0u; c->clip_n[a] = 0; }
    c->clip_d = 0;
    c->crop_hi[0] = nx; c->crop_hi[1] = ny; c->crop_hi[2] = nz;
    c->bricked = want_bricked(c, nx, ny, nz);
    rc = build_macro_cells(c);             // (sets have_vol)
    if (rc != VOLYM_OK) { c->have_vol = false; return rc; }
    return rebuild_lists(c);
}

int volym_set_importances(volym_ctx* c, const uint8_t* importances, uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (!c) return VOLYM_E_INVALID;
    clear_label_history(c);
    // the labels go, and the mask with them: density and importances get their hidden texels back (the importances are replaced
    // below).  A call that then fails on its arguments leaves the mask reset.
    int rc = retarget(c, current_cut(c), all_visible(current_cut(c)), true);
    if (rc != VOLYM_OK) return rc;
    rc = upload_volume(c, &c->d_imp, importances, nx, ny, nz);
    if (rc != VOLYM_OK) { c->have_imp = false; c->imp_bytes = 0; return rc; }
    c->imp_bytes = layout_bytes(want_bricked(c, nx, ny, nz), nx, ny, nz) + 16u;
    // the importances are the caller's now: a segment table has no labels to map any more
    if (c->d_labels) { HIPCHK(c, hipFree(c->d_labels)); c->d_labels = nullptr; }
    c->have_seg_table = false;
    if (c->d_imp0) { HIPCHK(c, hipFree(c->d_imp0)); c->d_imp0 = nullptr; }      // (of the importances this call replaced)
    c->imp_bricked = want_bricked(c, nx, ny, nz);
    important_texel_box(importances, nx, ny, nz, c->imp_box0_lo, c->imp_box0_hi);
    c->inx = nx; c->iny = ny; c->inz = nz;
    c->have_imp = true;
    return cut_fresh_importances(c);         // the crop box belongs to the scene: these importances are cropped like the last
}

int volym_set_labels(volym_ctx* c, const uint8_t* labels, uint32_t nx, uint32_t ny, uint32_t nz)
{
    if (!c) return VOLYM_E_INVALID;
    clear_label_history(c);
    // new labels mean new segments: all visible, and density and importances get their hidden texels back while the labels
    // that say which they are still exist
    int rc = retarget(c, current_cut(c), all_visible(current_cut(c)), true);
    if (rc != VOLYM_OK) return rc;
    if (imp_from_labels(c) && (crop_active(c) || plane_active(c)) && imp_croppable(c) && !c->d_imp0) {
        // the importances stay as they are, cropped and clipped, and the labels they were mapped from go: keep their uncropped bytes.  (A change
        // of the source, not of box or mask: it stands beside the transition, not in it.)
        rc = quiesce_slots(c);
        if (rc != VOLYM_OK) return rc;
        const hipError_t e = alloc_layout(&c->d_imp0, c->imp_bytes - 16u);
        if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(importances): ") + hipGetErrorString(e));
        rc = launch_segment_map(c, c->seg_table, c->d_imp0);
        if (rc != VOLYM_OK) return rc;
    }
    c->have_seg_table = false;
    rc = upload_volume(c, &c->d_labels, labels, nx, ny, nz);      // (quiesces the slots first)
    if (rc != VOLYM_OK) { if (c->d_labels) (void)hipFree(c->d_labels); c->d_labels = nullptr; return rc; }
    c->lnx = nx; c->lny = ny; c->lnz = nz;
    c->labels_bricked = want_bricked(c, nx, ny, nz);
    const hipError_t e = scan_label_stats(c);
    if (e != hipSuccess) {
        (void)hipFree(c->d_labels); c->d_labels = nullptr;
        return fail(c, VOLYM_E_HIP, std::string("volym_set_labels: ") + hipGetErrorString(e));
    }
    return VOLYM_OK;
}

int volym_set_segment_importances(volym_ctx* c, const uint8_t table[256])
{
    if (!c) return VOLYM_E_INVALID;
    if (!table) return fail(c, VOLYM_E_INVALID, "volym_set_segment_importances: NULL table");
    if (!c->d_labels) return fail(c, VOLYM_E_STATE, "volym_set_segment_importances: no labels (volym_set_labels first; volym_set_importances drops them)");
    int rc = quiesce_slots(c);
    if (rc != VOLYM_OK) return rc;
    const uint64_t nb = layout_bytes(c->labels_bricked, c->lnx, c->lny, c->lnz);
    if (c->imp_bytes != nb + 16u) {
        // the importances take the labels' dimensions and layout: a new allocation
        c->have_imp = false;
        if (c->d_imp) { HIPCHK(c, hipFree(c->d_imp)); c->d_imp = nullptr; }
        c->imp_bytes = 0;
        const hipError_t e = alloc_layout(&c->d_imp, nb);
        if (e != hipSuccess) return fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(importances): ") + hipGetErrorString(e));
        c->imp_bytes = nb + 16u;
    }
    rc = launch_segment_map(c, table, c->d_imp);
    if (rc != VOLYM_OK) return rc;
    c->inx = c->lnx; c->iny = c->lny; c->inz = c->lnz;
    c->have_imp = true;
    // from here on the labels and this table are the uncropped importances
    std::memcpy(c->seg_table, table, 256);
    c->have_seg_table = true;
    segment_important_box(c);                // (of the visible segments)
    c->imp_bricked = c->labels_bricked;
    if (c->d_imp0) { HIPCHK(c, hipFree(c->d_imp0)); c->d_imp0 = nullptr; }
    // the crop box and the mask (if any) cut the new importances, and the frames enqueued from here on march the new reject box, with or
    // without a volym_update in between
    return cut_fresh_importances(c);
}

int volym_label_counts(volym_ctx* c, uint64_t counts[256])
{
    if (!c) return VOLYM_E_INVALID;
    if (!counts) return fail(c, VOLYM_E_INVALID, "volym_label_counts: NULL output");
    if (!c->d_labels) return fail(c, VOLYM_E_STATE, "volym_label_counts: no labels");
    std::memcpy(counts, c->label_count, sizeof c->label_count);
    return VOLYM_OK;
}

}  // extern "C"
