// libvolym_hip.so: the geodesic pass (volym_geodesic_pass, volym_geodesic_check, the reads, volym_geodesic_at and the two device
// pointers) and the flood by it (volym_flood_labels, volym_flood_check; flood_by_map, which cost.hip calls with its own map), beside
// the kernels they launch (geodesic_kernels.h).  The pass
// is a read-only pass like the distance pass, its results a snapshot that later edits of the scene leave valid -- but it BLOCKS: the
// host enqueues the rounds of the relaxation in batches on slot 0's stream and reads 4 bytes after each, the tiles still marked.
// The flood is an edit like the others and goes through label_edit.hpp's transition.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

#include "label_edit.hpp"
#include "geodesic_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_geodesic_summary) == 8u * GEODESIC_SUMMARY_WORDS && offsetof(volym_geodesic_summary, n_reached) == 8u * GS_N_REACHED &&
              offsetof(volym_geodesic_summary, max_steps) == 8u * GS_MAX && offsetof(volym_geodesic_summary, max_at) == 8u * GS_MAX + 4u &&
              offsetof(volym_geodesic_summary, cell) == 8u * GS_CELL && offsetof(volym_geodesic_summary, cell_medium) == 8u * GS_CELL_MEDIUM &&
              offsetof(volym_geodesic_summary, hist) == 8u * GS_HIST, "volym_geodesic_summary is the 773 words the kernels index");
static_assert(sizeof(volym_geodesic) == 1324 && offsetof(volym_geodesic, seed) == 36 && offsetof(volym_geodesic, through) == 292 &&
              offsetof(volym_geodesic, max_steps) == 548 && offsetof(volym_geodesic, points) == 556, "volym_geodesic has no padding");
static_assert(sizeof(volym_flood) == 812 && offsetof(volym_flood, give) == 36 && offsetof(volym_flood, take) == 292 && offsetof(volym_flood, to) == 548 &&
              offsetof(volym_flood, steps_lo) == 804, "volym_flood has no padding");
static_assert(VOLYM_FLOOD_UNCUT == VOLYM_RELABEL_UNCUT, "edit_density reads the flag of either");
static_assert((VOLYM_GEODESIC_STEPS_MAX << 8 | 0xffu) < GEODESIC_OPEN - 256u, "a key and a key + 256 stay below OPEN");

// Rounds per batch, between two reads of the count of marked tiles.  A read costs a stream synchronisation, a round past the last
// active one only an empty launch, so a batch of several rounds wins while the relaxation is long and loses little when it is
// short.  VOLYM_GEODESIC_BATCH (1..1024) overrides it for scripts/geodesic_timing.py, which is where 8 was chosen.
constexpr uint32_t GEODESIC_BATCH = 8u;

static uint32_t batch_rounds()
{
    if (const char* e = std::getenv("VOLYM_GEODESIC_BATCH")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 1024) return static_cast<uint32_t>(v);
    }
    return GEODESIC_BATCH;
}

void volym::free_geodesic(volym_ctx* c)
{
    c->geodesic.release();
    c->geodesic_map.release();
    c->geodesic_tiles.release();
}

static bool have_pass(const volym_ctx* c) { return c->geodesic.count != 0u; }

// A flood request as an edit: the table only marks the labels that give, the receiving labels are {to[g] : take[g]}.  The map is
// volym_flood_labels' own or, for volym_spread_labels (cost.hip), the cost pass's: the same format, so the same kernel.
int volym::flood_by_map(volym_ctx* c, const volym_flood* f, const uint32_t* keys, const uint32_t pass_box[6], const char* who, volym_relabel_result& res)
{
    const bool dry = (f->flags & VOLYM_FLOOD_DRY_RUN) != 0u, uncut_bytes = (f->flags & VOLYM_FLOOD_UNCUT) != 0u;
    FloodRule rule = {};
    rule.min_byte = f->min_byte; rule.max_byte = f->max_byte;
    rule.steps_lo = f->steps_lo; rule.steps_hi = f->steps_hi;
    rule.store = dry ? 0u : 1u;
    std::memcpy(rule.box, pass_box, sizeof rule.box);
    std::memcpy(rule.take, f->take, 256);
    std::memcpy(rule.to, f->to, 256);
    uint8_t marks[256], receives[256] = {};
    for (int l = 0; l < 256; ++l) { marks[l] = static_cast<uint8_t>(f->give[l] ? l ^ 1 : l); if (f->take[l]) receives[f->to[l]] = 1u; }
    const LabelEdit edit = {f->box, marks, dry, who, receives};
    return edit_labels(c, edit, res, [&](hipStream_t stream, dim3 grid, const RelabelOut& out, const LabelTable& to, const CropSlab& s, uint32_t items,
                                         const LabelJournal* journal) {
        launch_edit(c, volym_geodesic_flood_kernel, volym_geodesic_flood_journal_kernel, stream, grid, out, to, s, rule, items, journal, edit_density(c, uncut_bytes), keys);
    });
}

extern "C" {

int volym_geodesic_check(const volym_geodesic* g, const uint32_t dims[3])
{
    if (!g || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(g->box, dims)) return VOLYM_E_INVALID;
    if (!box_at_most(g->box, VOLYM_GEODESIC_BOX_MAX)) return VOLYM_E_INVALID;
    if (g->flags & ~static_cast<uint32_t>(VOLYM_GEODESIC_UNCUT)) return VOLYM_E_INVALID;
    if (g->min_byte > g->max_byte || g->max_byte > 255u) return VOLYM_E_INVALID;
    if (g->max_steps > VOLYM_GEODESIC_STEPS_MAX) return VOLYM_E_INVALID;
    if (g->n_points > VOLYM_GEODESIC_POINTS_MAX) return VOLYM_E_INVALID;
    for (uint32_t p = 0; p < g->n_points; ++p)
        for (int a = 0; a < 3; ++a)
            if (g->points[p][a] < g->box[a] || g->points[p][a] >= g->box[3 + a]) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_geodesic_pass(volym_ctx* c, const volym_geodesic* q)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_geodesic_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_geodesic whole = {};                   // the whole volume, window 1..255, every label but 0 a seed, label 0 the medium, no points
    whole_volume_box(dims, whole.box);
    whole.min_byte = 1u; whole.max_byte = 255u;
    std::memset(whole.seed + 1, 1, 255);
    whole.through[0] = 1u;
    if (!q) q = &whole;
    if (volym_geodesic_check(q, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_geodesic_pass: need lo <= hi <= volume size on every axis, at most 2^31 - 2 texels in the box, no flag but UNCUT, "
                                        "min_byte <= max_byte <= 255, max_steps <= 2^24 - 3 and at most 64 points, all inside the box");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_geodesic_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    const uint32_t n_texels = static_cast<uint32_t>(box_texels(q->box));      // (checked: at most 2^31 - 2)
    const bool empty = n_texels == 0u;
    GeoTiles g = {};
    g.w = q->box[3] - q->box[0]; g.h = q->box[4] - q->box[1]; g.d = q->box[5] - q->box[2];
    g.ntx = (g.w + GEO_TX - 1u) / GEO_TX; g.nty = (g.h + GEO_TY - 1u) / GEO_TY; g.ntz = (g.d + GEO_TZ - 1u) / GEO_TZ;
    g.n_tiles = empty ? 0u : g.ntx * g.nty * g.ntz;                           // (no more than the box has texels)
    g.max_key = (q->max_steps ? q->max_steps : VOLYM_GEODESIC_STEPS_MAX) << 8 | 0xffu;
    const size_t n_state = GT_HEADER + 4u * static_cast<size_t>(g.n_tiles);

    // (set-up steps.  Whatever grows voids the snapshot first; should an allocation fail none is left)
    if (c->geodesic.capacity < 1u || n_texels > c->geodesic_map.capacity || n_state > c->geodesic_tiles.capacity) {
        c->geodesic.count = 0;
        rc = c->geodesic.reserve(c, stream, 1, "geodesic summary");
        if (rc == VOLYM_OK) rc = c->geodesic_map.reserve(c, stream, n_texels, "geodesic key map");
        if (rc == VOLYM_OK) rc = c->geodesic_tiles.reserve(c, stream, n_state, "geodesic tile state");
        if (rc != VOLYM_OK) { free_geodesic(c); return rc; }
    }
    unsigned long long* const summary = reinterpret_cast<unsigned long long*>(c->geodesic.ptr);
    uint32_t* const state = c->geodesic_tiles.ptr;
    uint32_t* const keys = c->geodesic_map.ptr;
    c->geodesic.count = 0;                               // (until the pass has run to its end: a failure below leaves no snapshot)
    const uint32_t n_state_zero = GT_HEADER + 2u * g.n_tiles;                 // the header and the flags; the lists are written before they are read
    hipLaunchKernelGGL(volym_geodesic_zero_kernel, dim3(std::max(1u, std::min((n_state_zero + 255u) / 256u, static_cast<uint32_t>(c->n_cus) * 8u))), dim3(256), 0, stream,
                       summary, state, n_state_zero);
    HIPCHK(c, hipGetLastError());
    if (!empty) {
        const bool uncut = (q->flags & VOLYM_GEODESIC_UNCUT) != 0u;
        const BoxWalkArgs a = box_walk_args(c, q->box, q->min_byte, uncut && c->d_vol0 ? c->d_vol0 : c->d_vol, with_labels);
        GeoRequest req = {};
        std::memcpy(req.seed, q->seed, 256);
        std::memcpy(req.through, q->through, 256);
        req.max_byte = q->max_byte; req.n_points = q->n_points;
        std::memcpy(req.points, q->points, sizeof(uint32_t) * 3u * q->n_points);
        const dim3 walk(walk_grid(c, a.n_rows)), block(256);
        hipLaunchKernelGGL(with_labels ? volym_geodesic_init_kernel<true> : volym_geodesic_init_kernel<false>, walk, block, 0, stream, a, req, g, keys, state, summary);
        HIPCHK(c, hipGetLastError());

        // The rounds, in batches; after each the 4 bytes that say how many tiles the batch's last round marked.  The guard: every round
        // that marks a tile has lowered a word for good, and each active round finalises at least one more layer of the box.
        const dim3 relax_grid(std::min(g.n_tiles, static_cast<uint32_t>(c->n_cus) * 8u));
        const uint64_t guard = static_cast<uint64_t>(n_texels) + 2u;
        const uint32_t batch = batch_rounds();
        uint64_t round = 0;
        for (;;) {
            for (uint32_t b = 0; b < batch; ++b, ++round) {
                hipLaunchKernelGGL(volym_geodesic_relax_kernel, relax_grid, block, 0, stream, g, keys, state, static_cast<uint32_t>(round % 6u));
                HIPCHK(c, hipGetLastError());
            }
            uint32_t marked = 0;
            rc = read_back(c, stream, &marked, state + GT_COUNT + round % 3u, sizeof marked);
            if (rc != VOLYM_OK) return rc;
            if (marked == 0u) break;
            if (round > guard) return fail(c, VOLYM_E_HIP, "volym_geodesic_pass: the relaxation did not settle within (texels of the box + 2) rounds");
        }
        c->geodesic_rounds = round;
        hipLaunchKernelGGL(volym_geodesic_finish_kernel, walk, block, 0, stream, g.w, a.n_rows, keys, state, summary);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(volym_geodesic_pack_kernel, dim3(1), dim3(64), 0, stream, a, static_cast<const uint32_t*>(state), summary);
        HIPCHK(c, hipGetLastError());
    }
    c->geodesic.count = 1;
    c->geodesic_map.count = n_texels;
    std::memcpy(c->geodesic_box, q->box, sizeof c->geodesic_box);
    return VOLYM_OK;
}

int volym_read_geodesic(volym_ctx* c, struct volym_geodesic_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_geodesic: NULL output");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_read_geodesic: no volym_geodesic_pass since the volume was set");
    return c->geodesic.read(c, c->slot0().stream, out, 1);
}

int volym_read_geodesic_map(volym_ctx* c, const uint32_t sub[6], uint32_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_volume(c, "volym_read_geodesic_map", "volym_geodesic_pass", have_pass(c), c->geodesic_box, c->geodesic_map.ptr, sub, out);
}

int volym_geodesic_at(volym_ctx* c, uint32_t x, uint32_t y, uint32_t z, struct volym_geodesic_site* out)
{
    if (!c) return VOLYM_E_INVALID;
    uint32_t key = GEODESIC_NONE;
    const int rc = read_box_texel(c, "volym_geodesic_at", "volym_geodesic_pass", have_pass(c), c->geodesic_box, c->geodesic_map.ptr, x, y, z, out ? &key : nullptr);
    if (rc != VOLYM_OK) return rc;
    *out = key == GEODESIC_NONE ? volym_geodesic_site{GEODESIC_NONE, 0u} : volym_geodesic_site{key >> 8, key & 0xffu};
    return VOLYM_OK;
}

void* volym_geodesic_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->geodesic.ptr : nullptr; }
void* volym_geodesic_map_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->geodesic_map.ptr : nullptr; }

int volym_flood_check(const volym_flood* f, const uint32_t dims[3])
{
    if (!f || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(f->box, dims)) return VOLYM_E_INVALID;
    if (f->flags & ~static_cast<uint32_t>(VOLYM_FLOOD_UNCUT | VOLYM_FLOOD_DRY_RUN)) return VOLYM_E_INVALID;
    if (f->min_byte > f->max_byte || f->max_byte > 255u) return VOLYM_E_INVALID;
    if (f->steps_lo > f->steps_hi) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_flood_labels(volym_ctx* c, const volym_flood* f, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!f) return fail(c, VOLYM_E_INVALID, "volym_flood_labels: NULL request");
    const int ok = editable_state(c, "volym_flood_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_flood_check(f, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_flood_labels: need lo <= hi <= volume size on every axis, known flags, min_byte <= max_byte <= 255 and steps_lo <= steps_hi");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_flood_labels: no volym_geodesic_pass since the volume was set");
    for (int a = 0; a < 3; ++a)
        if (f->box[a] < c->geodesic_box[a] || f->box[3 + a] > c->geodesic_box[3 + a])
            return fail(c, VOLYM_E_INVALID, "volym_flood_labels: a box that reaches outside the box of the geodesic pass");
    HIPCHK(c, hipSetDevice(c->device));
    volym_relabel_result res;
    const int rc = flood_by_map(c, f, c->geodesic_map.ptr, c->geodesic_box, "volym_flood_labels", res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

#if VOLYM_DEV_SWITCHES
// scripts/geodesic_timing.py: out = {the rounds the latest pass enqueued, the tiles it relaxed in all}.  Blocks.
int volym_dev_geodesic_counts(volym_ctx* c, unsigned long long out[2])
{
    if (!c || !out) return VOLYM_E_INVALID;
    if (!have_pass(c) || c->geodesic_tiles.capacity < GT_HEADER) return fail(c, VOLYM_E_STATE, "volym_dev_geodesic_counts: no volym_geodesic_pass since the volume was set");
    out[0] = c->geodesic_rounds;
    return read_back(c, c->slot0().stream, &out[1], c->geodesic_tiles.ptr + GT_RELAXED, sizeof out[1]);
}
#endif

}  // extern "C"
