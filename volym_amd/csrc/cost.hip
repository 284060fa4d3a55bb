// libvolym_hip.so: the cost pass (volym_cost_pass, volym_cost_check, the reads, volym_cost_at and the two device pointers) beside the
// kernels it launches (cost_kernels.h), and the spread by it (volym_spread_labels, volym_spread_check).  The pass is the geodesic
// pass's sibling with weighted steps: a read-only pass whose results are a snapshot of its own, and it BLOCKS: the host enqueues the
// rounds of the relaxation in batches on slot 0's stream and reads 4 bytes after each, the tiles still marked.  The spread is the
// flood's edit read from this pass's map: the same kernel, launched by geodesic.hip's flood_by_map, so this unit holds no copy of it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

#include "label_edit.hpp"
#include "cost_kernels.h"

using namespace volym;

static int fail(volym_ctx* c, int code, const std::string& msg) { return ctx_fail(c, code, msg); }
#define HIPCHK(ctx, expr) VOLYM_HIPCHK(ctx, expr)

static_assert(sizeof(volym_cost_summary) == 8u * COST_SUMMARY_WORDS && offsetof(volym_cost_summary, n_reached) == 8u * CS_N_REACHED &&
              offsetof(volym_cost_summary, max_cost) == 8u * CS_MAX && offsetof(volym_cost_summary, max_at) == 8u * CS_MAX + 4u &&
              offsetof(volym_cost_summary, cell) == 8u * CS_CELL && offsetof(volym_cost_summary, cell_medium) == 8u * CS_CELL_MEDIUM &&
              offsetof(volym_cost_summary, hist) == 8u * CS_HIST, "volym_cost_summary is the 773 words the kernels index");
static_assert(sizeof(volym_cost) == 1336 && offsetof(volym_cost, seed) == 36 && offsetof(volym_cost, through) == 292 && offsetof(volym_cost, max_cost) == 548 &&
              offsetof(volym_cost, points) == 556 && offsetof(volym_cost, step_cost) == 1324 && offsetof(volym_cost, hist_shift) == 1332, "volym_cost has no padding");
// the spread is handed to the flood's host function as a volym_flood: the same fields in the same places, the same flags, the same NONE
static_assert(sizeof(volym_spread) == sizeof(volym_flood) && offsetof(volym_spread, give) == offsetof(volym_flood, give) &&
              offsetof(volym_spread, take) == offsetof(volym_flood, take) && offsetof(volym_spread, to) == offsetof(volym_flood, to) &&
              offsetof(volym_spread, cost_lo) == offsetof(volym_flood, steps_lo) && offsetof(volym_spread, cost_hi) == offsetof(volym_flood, steps_hi),
              "volym_spread is laid out as volym_flood");
static_assert(VOLYM_SPREAD_UNCUT == VOLYM_FLOOD_UNCUT && VOLYM_SPREAD_DRY_RUN == VOLYM_FLOOD_DRY_RUN && VOLYM_COST_NONE == VOLYM_GEODESIC_NONE,
              "the flood's kernel reads the cost map as it reads its own");

// Rounds per batch, between two reads of the count of marked tiles (geodesic.hip has the trade).  VOLYM_COST_BATCH (1..1024)
// overrides it in the development build for scripts/cost_timing.py, whose sweep chooses the value.
constexpr uint32_t COST_BATCH = 8u;

static uint32_t batch_rounds()
{
#if VOLYM_DEV_SWITCHES
    if (const char* e = std::getenv("VOLYM_COST_BATCH")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 1024) return static_cast<uint32_t>(v);
    }
#endif
    return COST_BATCH;
}

void volym::free_cost(volym_ctx* c)
{
    c->cost.release();
    c->cost_map.release();
    c->cost_bytes.release();
    c->cost_tiles.release();
}

static bool have_pass(const volym_ctx* c) { return c->cost.count != 0u; }

extern "C" {

int volym_cost_check(const volym_cost* q, const uint32_t dims[3])
{
    if (!q || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(q->box, dims)) return VOLYM_E_INVALID;
    if (!box_at_most(q->box, VOLYM_COST_BOX_MAX)) return VOLYM_E_INVALID;
    if (q->flags & ~static_cast<uint32_t>(VOLYM_COST_UNCUT)) return VOLYM_E_INVALID;
    if (q->min_byte > q->max_byte || q->max_byte > 255u) return VOLYM_E_INVALID;
    if (q->step_cost < 1u || q->step_cost > 255u || q->contrast_cost > 255u) return VOLYM_E_INVALID;
    if (q->max_cost > VOLYM_COST_MAX) return VOLYM_E_INVALID;
    if (q->hist_shift > VOLYM_COST_HIST_SHIFT_MAX) return VOLYM_E_INVALID;
    if (q->n_points > VOLYM_COST_POINTS_MAX) return VOLYM_E_INVALID;
    for (uint32_t p = 0; p < q->n_points; ++p)
        for (int a = 0; a < 3; ++a)
            if (q->points[p][a] < q->box[a] || q->points[p][a] >= q->box[3 + a]) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_cost_pass(volym_ctx* c, const volym_cost* q)
{
    if (!c) return VOLYM_E_INVALID;
    if (!c->have_vol) return fail(c, VOLYM_E_STATE, "volym_cost_pass: no volume (volym_set_volume first)");
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    volym_cost whole = {};                       // the whole volume, window 1..255, every label but 0 a seed, label 0 the medium, no points
    whole_volume_box(dims, whole.box);
    whole.min_byte = 1u; whole.max_byte = 255u;
    std::memset(whole.seed + 1, 1, 255);
    whole.through[0] = 1u;
    whole.step_cost = 1u; whole.contrast_cost = 16u; whole.hist_shift = 4u;
    if (!q) q = &whole;
    if (volym_cost_check(q, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_cost_pass: need lo <= hi <= volume size on every axis, at most 2^31 - 2 texels in the box, no flag but UNCUT, "
                                        "min_byte <= max_byte <= 255, step_cost in 1..255, contrast_cost <= 255, max_cost <= 2^24 - 3, hist_shift <= 16 and at "
                                        "most 64 points, all inside the box");
    const bool with_labels = labels_fit(c);
    int rc = check_labels_layout(c, "volym_cost_pass");
    if (rc != VOLYM_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t stream = c->slot0().stream;
    const uint32_t n_texels = static_cast<uint32_t>(box_texels(q->box));      // (checked: at most 2^31 - 2)
    const bool empty = n_texels == 0u;
    CostTiles g = {};
    g.w = q->box[3] - q->box[0]; g.h = q->box[4] - q->box[1]; g.d = q->box[5] - q->box[2];
    g.ntx = (g.w + COST_TX - 1u) / COST_TX; g.nty = (g.h + COST_TY - 1u) / COST_TY; g.ntz = (g.d + COST_TZ - 1u) / COST_TZ;
    g.n_tiles = empty ? 0u : g.ntx * g.nty * g.ntz;                           // (no more than the box has texels)
    g.max_key = (q->max_cost ? q->max_cost : VOLYM_COST_MAX) << 8 | 0xffu;
    g.step_cost = q->step_cost; g.contrast_cost = q->contrast_cost;
    const size_t n_state = CT_HEADER + 4u * static_cast<size_t>(g.n_tiles);

    // (set-up steps.  Whatever grows voids the snapshot first; should an allocation fail none is left)
    if (c->cost.capacity < 1u || n_texels > c->cost_map.capacity || n_texels > c->cost_bytes.capacity || n_state > c->cost_tiles.capacity) {
        c->cost.count = 0;
        rc = c->cost.reserve(c, stream, 1, "cost summary");
        if (rc == VOLYM_OK) rc = c->cost_map.reserve(c, stream, n_texels, "cost key map");
        if (rc == VOLYM_OK) rc = c->cost_bytes.reserve(c, stream, n_texels, "cost byte map");
        if (rc == VOLYM_OK) rc = c->cost_tiles.reserve(c, stream, n_state, "cost tile state");
        if (rc != VOLYM_OK) { free_cost(c); return rc; }
    }
    unsigned long long* const summary = reinterpret_cast<unsigned long long*>(c->cost.ptr);
    uint32_t* const state = c->cost_tiles.ptr;
    uint32_t* const keys = c->cost_map.ptr;
    uint8_t* const bytes = c->cost_bytes.ptr;
    c->cost.count = 0;                                   // (until the pass has run to its end: a failure below leaves no snapshot)
    const uint32_t n_state_zero = CT_HEADER + 2u * g.n_tiles;                 // the header and the flags; the lists are written before they are read
    hipLaunchKernelGGL(volym_cost_zero_kernel, dim3(std::max(1u, std::min((n_state_zero + 255u) / 256u, static_cast<uint32_t>(c->n_cus) * 8u))), dim3(256), 0, stream,
                       summary, state, n_state_zero);
    HIPCHK(c, hipGetLastError());
    c->cost_rounds = 0;
    if (!empty) {
        const bool uncut = (q->flags & VOLYM_COST_UNCUT) != 0u;
        const BoxWalkArgs a = box_walk_args(c, q->box, q->min_byte, uncut && c->d_vol0 ? c->d_vol0 : c->d_vol, with_labels);
        CostRequest req = {};
        std::memcpy(req.seed, q->seed, 256);
        std::memcpy(req.through, q->through, 256);
        req.max_byte = q->max_byte; req.n_points = q->n_points;
        std::memcpy(req.points, q->points, sizeof(uint32_t) * 3u * q->n_points);
        const dim3 walk(walk_grid(c, a.n_rows)), block(256);
        hipLaunchKernelGGL(with_labels ? volym_cost_init_kernel<true> : volym_cost_init_kernel<false>, walk, block, 0, stream, a, req, g, keys, bytes, state, summary);
        HIPCHK(c, hipGetLastError());

        // The rounds, in batches; after each the 4 bytes that say how many tiles the batch's last round marked.  The guard bounds
        // rounds, not lowerings: after round r every texel is final that some cheapest chain reaches across at most r tile faces
        // (cost_kernels.h has the induction), and such a chain crosses fewer faces than the box has texels.
        const dim3 relax_grid(std::min(g.n_tiles, static_cast<uint32_t>(c->n_cus) * 8u));
        const uint64_t guard = static_cast<uint64_t>(n_texels) + 2u;
        const uint32_t batch = batch_rounds();
        uint64_t round = 0;
        for (;;) {
            for (uint32_t b = 0; b < batch; ++b, ++round) {
                hipLaunchKernelGGL(volym_cost_relax_kernel, relax_grid, block, 0, stream, g, keys, static_cast<const uint8_t*>(bytes), state, static_cast<uint32_t>(round % 6u));
                HIPCHK(c, hipGetLastError());
            }
            uint32_t marked = 0;
            rc = read_back(c, stream, &marked, state + CT_COUNT + round % 3u, sizeof marked);
            if (rc != VOLYM_OK) return rc;
            if (marked == 0u) break;
            if (round > guard) return fail(c, VOLYM_E_HIP, "volym_cost_pass: the relaxation did not settle within (texels of the box + 2) rounds");
        }
        c->cost_rounds = round;
        hipLaunchKernelGGL(volym_cost_finish_kernel, walk, block, 0, stream, g.w, a.n_rows, q->hist_shift, keys, state, summary);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(volym_cost_pack_kernel, dim3(1), dim3(64), 0, stream, a, static_cast<const uint32_t*>(state), summary);
        HIPCHK(c, hipGetLastError());
    }
    c->cost.count = 1;
    c->cost_map.count = n_texels;
    c->cost_bytes.count = n_texels;
    std::memcpy(c->cost_box, q->box, sizeof c->cost_box);
    return VOLYM_OK;
}

int volym_read_cost(volym_ctx* c, struct volym_cost_summary* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return fail(c, VOLYM_E_INVALID, "volym_read_cost: NULL output");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_read_cost: no volym_cost_pass since the volume was set");
    return c->cost.read(c, c->slot0().stream, out, 1);
}

int volym_read_cost_map(volym_ctx* c, const uint32_t sub[6], uint32_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    return read_box_volume(c, "volym_read_cost_map", "volym_cost_pass", have_pass(c), c->cost_box, c->cost_map.ptr, sub, out);
}

int volym_cost_at(volym_ctx* c, uint32_t x, uint32_t y, uint32_t z, struct volym_cost_site* out)
{
    if (!c) return VOLYM_E_INVALID;
    uint32_t key = COST_NONE;
    const int rc = read_box_texel(c, "volym_cost_at", "volym_cost_pass", have_pass(c), c->cost_box, c->cost_map.ptr, x, y, z, out ? &key : nullptr);
    if (rc != VOLYM_OK) return rc;
    *out = key == COST_NONE ? volym_cost_site{COST_NONE, 0u} : volym_cost_site{key >> 8, key & 0xffu};
    return VOLYM_OK;
}

void* volym_cost_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->cost.ptr : nullptr; }
void* volym_cost_map_device_ptr(volym_ctx* c) { return (c && have_pass(c)) ? c->cost_map.ptr : nullptr; }

int volym_spread_check(const volym_spread* s, const uint32_t dims[3])
{
    if (!s || !dims) return VOLYM_E_INVALID;
    if (!box_in_volume(s->box, dims)) return VOLYM_E_INVALID;
    if (s->flags & ~static_cast<uint32_t>(VOLYM_SPREAD_UNCUT | VOLYM_SPREAD_DRY_RUN)) return VOLYM_E_INVALID;
    if (s->min_byte > s->max_byte || s->max_byte > 255u) return VOLYM_E_INVALID;
    if (s->cost_lo > s->cost_hi) return VOLYM_E_INVALID;
    return VOLYM_OK;
}

int volym_spread_labels(volym_ctx* c, const volym_spread* s, struct volym_relabel_result* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!s) return fail(c, VOLYM_E_INVALID, "volym_spread_labels: NULL request");
    const int ok = editable_state(c, "volym_spread_labels");
    if (ok != VOLYM_OK) return ok;
    const uint32_t dims[3] = {c->nx, c->ny, c->nz};
    if (volym_spread_check(s, dims) != VOLYM_OK)
        return fail(c, VOLYM_E_INVALID, "volym_spread_labels: need lo <= hi <= volume size on every axis, known flags, min_byte <= max_byte <= 255 and cost_lo <= cost_hi");
    if (!have_pass(c)) return fail(c, VOLYM_E_STATE, "volym_spread_labels: no volym_cost_pass since the volume was set");
    for (int a = 0; a < 3; ++a)
        if (s->box[a] < c->cost_box[a] || s->box[3 + a] > c->cost_box[3 + a])
            return fail(c, VOLYM_E_INVALID, "volym_spread_labels: a box that reaches outside the box of the cost pass");
    HIPCHK(c, hipSetDevice(c->device));
    volym_flood f;                                       // (laid out alike: the assertions above)
    std::memcpy(&f, s, sizeof f);
    volym_relabel_result res;
    const int rc = flood_by_map(c, &f, c->cost_map.ptr, c->cost_box, "volym_spread_labels", res);
    if (rc == VOLYM_OK && out) *out = res;
    return rc;
}

#if VOLYM_DEV_SWITCHES
// scripts/cost_timing.py: out = {the rounds the latest pass enqueued, the tiles it relaxed in all}.  Blocks.
int volym_dev_cost_counts(volym_ctx* c, unsigned long long out[2])
{
    if (!c || !out) return VOLYM_E_INVALID;
    if (!have_pass(c) || c->cost_tiles.capacity < CT_HEADER) return fail(c, VOLYM_E_STATE, "volym_dev_cost_counts: no volym_cost_pass since the volume was set");
    out[0] = c->cost_rounds;
    return read_back(c, c->slot0().stream, &out[1], c->cost_tiles.ptr + CT_RELAXED, sizeof out[1]);
}
#endif

}  // extern "C"
