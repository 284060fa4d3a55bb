// The work-list scheduler of variant 2 (worklist.hpp): geometric list, deal, re-balancing, device form, costs by item.
// Plain C++: no HIP header, no context.
#include "worklist.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "../../include/volym_hip.h"

#ifndef VOLYM_DEV_SWITCHES
#define VOLYM_DEV_SWITCHES 0
#endif

using namespace volym;

// the entry code's fields at their extremes, there and back
static_assert(wl_code(wl_with_prio(wl_item(0x0fffffffu), 3u)) == 0x0fffffffu && wl_prio(wl_with_prio(wl_item(0x0fffffffu), 3u)) == 3u, "whole item");
static_assert(wl_is_quarter(wl_quarter(0x03ffffffu, 3u)) && !wl_is_super(wl_quarter(0x03ffffffu, 3u)) && wl_quarter_item(wl_quarter(0x03ffffffu, 3u)) == 0x03ffffffu &&
              wl_quarter_index(wl_quarter(0x03ffffffu, 3u)) == 3u && wl_local_tile(wl_quarter(0x03ffffffu, 3u)) == 0x00ffffffu, "quarter");
static_assert(wl_is_super(wl_super(0x00ffffffu)) && !wl_is_quarter(wl_super(0x00ffffffu)) && wl_super_tile(wl_super(0x00ffffffu)) == 0x00ffffffu &&
              wl_local_tile(wl_code(wl_with_prio(wl_super(0x00ffffffu), 3u))) == 0x00ffffffu, "super fill");
static_assert(!wl_is_quarter(wl_item(0u)) && !wl_is_super(wl_item(0u)) && wl_local_tile(wl_item(7u)) == 1u, "item");

// geometric list: the 8x8-pixel wave tiles of this rank's 16x16 tiles (item = local_tile*4 + sub), by Chebyshev
// distance of the tile centre from the screen centre.  The orbit camera always targets the volume centre
// (src/camera.rs:23), so the long rays are the central ones: they start first.
std::vector<uint32_t> volym::build_geometric(const ShardGrid& g)
{
    std::vector<std::pair<uint32_t, uint32_t>> keyed;
    keyed.reserve(static_cast<size_t>(g.n_local) * 4);
    for (uint32_t lt = 0; lt < g.n_local; ++lt) {
        const uint32_t tile = lt * g.world + g.rank;
        const uint32_t tx = tile % g.tiles_x, ty = tile / g.tiles_x;
        for (uint32_t sub = 0; sub < 4; ++sub) {
            const int x0 = static_cast<int>(tx * 16u + (sub & 1u) * 8u), y0 = static_cast<int>(ty * 16u + (sub >> 1) * 8u);
            if (x0 >= static_cast<int>(g.W) || y0 >= static_cast<int>(g.H)) {
                if (g.world == 1) continue;          // wholly outside the frame: nothing to store in raster mode
            }
            const int dx = std::abs(2 * x0 + 8 - static_cast<int>(g.W)), dy = std::abs(2 * y0 + 8 - static_cast<int>(g.H));
            // rings of 16 pixels; inside a ring a hash decides, so that a workgroup (which takes every G-th item)
            // does not sit at the same angular position on every ring
            const uint32_t item = lt * 4u + sub;
            uint32_t h = item * 0x9E3779B1u;
            h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
            keyed.emplace_back((static_cast<uint32_t>(std::max(dx, dy)) / 32u) << 20 | (h & 0xfffffu), item);
        }
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<uint32_t> geometric(keyed.size());
    for (size_t i = 0; i < keyed.size(); ++i) geometric[i] = keyed[i].second;
    return geometric;
}

// Deal `item_cost` into a list (feedback thread; also the caller's thread inside blocking set-up calls).
void volym::deal_list(const ShardGrid& g, const ListSettings& set, const CapturedLaunch& job, bool moving, const std::vector<uint16_t>& measured_cost,
                      std::vector<uint8_t>& item_is_dp, const std::vector<uint32_t>& geometric, WorkList& out)
{
    const uint32_t n_local = g.n_local;
    const uint32_t waves = job.waves;
    // The costs were measured on an earlier frame; when the camera moves, what was expensive there is expensive a tile or two
    // further on here.  A maximum filter over the neighbouring 8x8 items (radius set.dilate) makes the list hold for a
    // while: the price is a few tiles split or started early that did not need it.
    std::vector<uint16_t> item_cost(measured_cost);
    // Has the camera moved since the captured frame (`moving`)?  Then the list will be read on yet another view: dilate the costs and
    // keep split tiles split (hysteresis).  A view that stands still gets exactly what its own costs say -- but only costs
    // MEASURED on whole 8x8 entries say it well (a split tile reports an estimate).  So when the captured list held split
    // tiles, the first deal for a standing view is a measuring list without any split, and the deal after it is final.
    const bool measuring = !moving && job.captured_has_dp && set.dp_min_cost < 0;
    const int dilate = set.dilate >= 0 ? set.dilate : (moving ? 1 : 0);
    if (dilate > 0) {
        const uint32_t gw = g.tiles_x * 2u, gh = g.tiles_y * 2u;
        std::vector<uint16_t> grid(static_cast<size_t>(gw) * gh, 0), tmp(static_cast<size_t>(gw) * gh, 0);
        auto cell_of = [&](uint32_t item) {
            const uint32_t tile = (item >> 2) * g.world + g.rank, sub = item & 3u;
            return static_cast<size_t>((tile / g.tiles_x) * 2u + (sub >> 1)) * gw + (tile % g.tiles_x) * 2u + (sub & 1u);
        };
        for (uint32_t item : geometric) grid[cell_of(item)] = measured_cost[item];
        const int r = dilate;
        for (uint32_t y = 0; y < gh; ++y)
            for (uint32_t x = 0; x < gw; ++x) {
                uint16_t m = 0;
                for (int d = -r; d <= r; ++d) { const int xx = static_cast<int>(x) + d; if (xx >= 0 && xx < static_cast<int>(gw)) m = std::max(m, grid[static_cast<size_t>(y) * gw + xx]); }
                tmp[static_cast<size_t>(y) * gw + x] = m;
            }
        for (uint32_t y = 0; y < gh; ++y)
            for (uint32_t x = 0; x < gw; ++x) {
                uint16_t m = 0;
                for (int d = -r; d <= r; ++d) { const int yy = static_cast<int>(y) + d; if (yy >= 0 && yy < static_cast<int>(gh)) m = std::max(m, tmp[static_cast<size_t>(yy) * gw + x]); }
                grid[static_cast<size_t>(y) * gw + x] = m;
            }
        for (uint32_t item : geometric) item_cost[item] = grid[cell_of(item)];
    }
    // Tiles above the threshold are split into four 4x4 quarter tiles marched depth-parallel (raymarch_pq.h): their cost is
    // a long chain of dependent samples, which four lanes per ray walk ~4x faster, on four waves.  Which tiles?  Those that
    // would keep one wave busy for more than ~1.5x a wave's fair share of the frame (sum of costs / resident waves): below
    // that they hide in the bulk and splitting only adds work.  A tile that is split stays split until its estimated cost
    // falls below 0.7x the threshold (its cost is an estimate while it is split).
    uint64_t total_cost = 0;
    for (uint32_t item : geometric) total_cost += item_cost[item];
    const uint32_t resident_waves = std::max(1u, job.max_grid * waves);
    // Measured over four scenes (profiles/r03_dp_scene_sweep.txt: bonsai, teapot, a dense ball, thin vessels; 1080p, where the
    // split matters -- at 3840x2160 every setting gives the same frame time): the common instantiation wants 1.7-1.9x (bonsai
    // 33.9 us at 1.9x against 34.3 with r02's rule, teapot 44.9 against 51.9, ball 54.1 against 60.9; the vessels do not
    // care); r02's 1.5x with an absolute floor of 104 units was the optimum of the bonsai alone and cost the other scenes
    // 10-17 %.  The look-ahead instantiations keep 1.5x, the continuous-rho modes 1.2x (their classic loop speculates only
    // two samples deep, a depth-parallel item four), as measured in r01 / r02.  A list dealt for a moving camera is read on later
    // views: there the lower threshold (more tiles split than the captured view needed) is the better one (turntable at 0.25
    // degrees per frame: 53.4 us at 1.5x, 57.0 at 1.9x).
    const uint64_t tenths = set.dp_min_cost < -1 ? static_cast<uint64_t>(-set.dp_min_cost) : (job.continuous ? 12u : (job.plain && !moving) ? 19u : 15u);
    const uint64_t floor_cost = set.dp_floor;                                   // 64 units: a tile below that is never worth four waves
    const uint32_t adaptive = static_cast<uint32_t>(std::max<uint64_t>(floor_cost, tenths * total_cost / (10u * resident_waves) + 16));
    const uint32_t dp_thr = set.dp_min_cost < 0 ? adaptive : static_cast<uint32_t>(set.dp_min_cost);
#if VOLYM_DEV_SWITCHES
    if (std::getenv("VOLYM_TRIM_LOG"))
        std::fprintf(stderr, "deal: total cost %llu, fair share %llu, floor %llu, split threshold %u (moving %d measuring %d)\n", static_cast<unsigned long long>(total_cost),
                     static_cast<unsigned long long>(total_cost / resident_waves), static_cast<unsigned long long>(floor_cost), dp_thr, moving ? 1 : 0, measuring ? 1 : 0);
#endif
    const bool dp_ok = set.dp_min_cost != 0 && !measuring;
    std::vector<std::pair<uint32_t, uint32_t>> keyed;      // (cost share, entry)
    keyed.reserve(geometric.size() * 2);
    bool has_dp = false;
    // 16x16 tiles whose four sub-tiles were all constant become one "super" fill item
    std::vector<uint8_t> all_fill(n_local, 1), seen(n_local, 0), cnt(n_local, 0);
    for (uint32_t item : geometric) { if (item_cost[item] != 0) all_fill[item >> 2] = 0; cnt[item >> 2]++; }
    for (uint32_t lt = 0; lt < n_local; ++lt) if (cnt[lt] != 4) all_fill[lt] = 0;   // sub-tiles outside the frame are not listed
    for (uint32_t item : geometric) {
        const uint32_t k = item_cost[item];
        if (set.super_fill && all_fill[item >> 2]) {
            if (!seen[item >> 2]) { seen[item >> 2] = 1; keyed.emplace_back(0u, wl_super(item >> 2)); }
            item_is_dp[item] = 0;
            continue;
        }
        if (set.dev_drop_tenths && static_cast<uint64_t>(k) * 10u * resident_waves >= static_cast<uint64_t>(set.dev_drop_tenths) * total_cost) { item_is_dp[item] = 0; continue; }   // dev: what if the longest tiles were not there?
        const bool split = dp_ok && (k >= dp_thr || (moving && item_is_dp[item] && set.dp_min_cost < 0 && 10u * k >= 7u * dp_thr));
        has_dp = has_dp || split;
        item_is_dp[item] = split ? 1 : 0;
        if (split)
            for (uint32_t qd = 0; qd < 4; ++qd) keyed.emplace_back((k * set.dp_share_pct + 99u) / 100u, wl_quarter(item, qd));
        else
            keyed.emplace_back(k, wl_item(item));
    }
    {
        // stable counting sort by decreasing cost share (shares are small integers): the feedback thread's latency is what
        // a moving camera sees as the age of its list
        uint32_t kmax = 0;
        for (const auto& kv : keyed) kmax = std::max(kmax, kv.first);
        std::vector<uint32_t> start(static_cast<size_t>(kmax) + 2u, 0);
        for (const auto& kv : keyed) start[kmax - kv.first + 1u]++;
        for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
        std::vector<std::pair<uint32_t, uint32_t>> sorted(keyed.size());
        for (const auto& kv : keyed) sorted[start[kmax - kv.first]++] = kv;
        keyed.swap(sorted);
    }
    if (set.only_quarters) {     // dev experiment: how long do the depth-parallel items take with the machine to themselves?
        std::vector<std::pair<uint32_t, uint32_t>> q;
        for (const auto& kv : keyed) if (wl_is_quarter(kv.second)) q.push_back(kv);
        keyed.swap(q);
    }
    // issue priority from the entry's cost relative to a wave's fair share of the frame
    const uint64_t fair = std::max<uint64_t>(1, total_cost / resident_waves);
    const bool prio_ok = set.prio_tenths[0] > 0 && static_cast<uint64_t>(n_local) * 16u < (1u << WL_PRIO_SHIFT);
    const uint32_t n_keyed = static_cast<uint32_t>(keyed.size());
    const uint32_t G = std::max(1u, std::min((n_keyed + waves - 1) / waves, job.max_grid));
    // Workgroup b reads entries b, b + G, ... of the list.  The entries, in order of decreasing cost, are dealt in
    // boustrophedon order over the workgroups (0..G-1, G-1..0, ...): the sums differ by about one entry of the current size,
    // as with a longest-processing-time heap, in one pass (the feedback thread's latency is the age of a moving camera's
    // list).  Rounds are list rows: entry i sits in row i / G.
    const size_t rows = (static_cast<size_t>(n_keyed) + G - 1) / G;
    out.entries.assign(static_cast<size_t>(G) * rows, PQ_NO_ITEM);
    out.shares.assign(static_cast<size_t>(G) * rows, 0);
    for (uint32_t i = 0; i < n_keyed; ++i) {
        const std::pair<uint32_t, uint32_t>& kv = keyed[i];
        uint32_t prio = 0;
        if (prio_ok && kv.first) {
            const uint64_t k10 = static_cast<uint64_t>(kv.first) * 10u;
            prio = k10 >= set.prio_tenths[2] * fair ? 3u : k10 >= set.prio_tenths[1] * fair ? 2u : k10 >= set.prio_tenths[0] * fair ? 1u : 0u;
        }
        const uint32_t row = i / G, j = i - row * G;
        const size_t pos = static_cast<size_t>(row) * G + ((row & 1u) ? G - 1u - j : j);
        out.entries[pos] = wl_with_prio(kv.second, prio);
        out.shares[pos] = static_cast<uint16_t>(std::min(65535u, kv.first));
    }
    out.grid = G;
    out.view_serial = job.view_serial;
    out.has_dp = has_dp;
    out.trimmable = !moving && !measuring;
    out.trim_round = 0;
    out.final_for_view = out.trimmable && set.trim_rounds == 0;
}

// Re-balance a standing view's list from the times its workgroups took (feedback thread).  The counted costs predict a
// workgroup's time to within a few percent (profiles/r02_wave_trace.txt: end times spread over ~4 us of 33, and the spread
// repeats from frame to frame); the frame ends with the LAST workgroup.  So: every workgroup's measured duration gives its
// own rate (time per unit of cost, for the entries it holds); workgroups that ended after the mean hand entries worth
// `damp` x their excess to a pool, and the pool goes, largest first, to whichever workgroup is predicted to end first.
// Scheduling only: the pixels do not change.  Measured (scripts/trim_rounds.py, 1080p bonsai): 33.95 us without, 33.6-33.7 us
// with 1..8 rounds -- the spread of the end times halves (28.0..34.1 -> 29.7..32.3 us) but their MEAN rises as it does: the
// workgroups that used to finish early no longer leave the others a quieter machine.  In alternating 20 000-frame runs of two
// builds the gain is 0.1 us (33.17 -> 33.07), and one run in six came out at 33.85: a list trimmed from a capture that caught a
// hiccup is final, and wrong, for as long as the view stands.  A deterministic list is worth more than 0.3 %: OFF by default
// (ListSettings::trim_rounds = 0; VOLYM_OPT_REBALANCE_ROUNDS turns it on).
bool volym::trim_list(const ListSettings& set, const CapturedLaunch& job, size_t capacity, const WorkList& in, const uint32_t* times, WorkList& out)
{
    const uint32_t G = in.grid, waves = job.waves;
    if (G == 0 || G != job.grid || in.entries.size() % G != 0 || in.shares.size() != in.entries.size()) return false;
    const size_t rows = in.entries.size() / G;
    const uint32_t* starts = times + static_cast<size_t>(G) * waves;
    const uint32_t ref = starts[0];
    int32_t t0 = 0;
    for (uint32_t b = 0; b < G; ++b) t0 = std::min(t0, static_cast<int32_t>(starts[b] - ref));
    struct Ent { uint32_t w, code; };
    std::vector<std::vector<Ent>> wg(G);
    std::vector<double> dur(G), weight(G, 0.0), rate(G), pred(G);
    double mean = 0.0;
    for (uint32_t b = 0; b < G; ++b) {
        int32_t end = 0;
        for (uint32_t w = 0; w < waves; ++w) end = std::max(end, static_cast<int32_t>(times[static_cast<size_t>(b) * waves + w] - ref));
        dur[b] = std::max(1.0, static_cast<double>(end - t0));
        wg[b].reserve(rows + 8);
        for (size_t r = 0; r < rows; ++r) {
            const size_t pos = r * G + b;
            if (in.entries[pos] == PQ_NO_ITEM) continue;
            wg[b].push_back(Ent{in.shares[pos] + 1u, in.entries[pos]});
            weight[b] += in.shares[pos] + 1u;
        }
        mean += dur[b];
    }
    mean /= G;
    if (mean > 1.0e6) return false;                        // a second: not a frame's times (counter wrap, garbage)
    const double damp = 0.8;
    std::vector<Ent> pool;
    for (uint32_t b = 0; b < G; ++b) {
        rate[b] = dur[b] / std::max(1.0, weight[b]);
        pred[b] = dur[b];
        double excess = damp * (dur[b] - mean);
        if (excess <= 0.0) continue;
        // largest entries that fit first (the list of a workgroup is in order of decreasing share); constant tiles stay
        std::vector<Ent> keep;
        keep.reserve(wg[b].size());
        for (const Ent& e : wg[b]) {
            const double t = e.w * rate[b];
            if (e.w > 1u && t <= excess) { pool.push_back(e); excess -= t; pred[b] -= t; }
            else keep.push_back(e);
        }
        wg[b].swap(keep);
    }
    std::stable_sort(pool.begin(), pool.end(), [](const Ent& a, const Ent& b) { return a.w > b.w; });
    for (const Ent& e : pool) {
        uint32_t best = 0;
        double best_t = 1.0e300;
        for (uint32_t b = 0; b < G; ++b) { const double t = pred[b] + e.w * rate[b]; if (t < best_t) { best_t = t; best = b; } }
        pred[best] = best_t;
        wg[best].push_back(e);
    }
#if VOLYM_DEV_SWITCHES
    if (std::getenv("VOLYM_TRIM_LOG")) {
        double mx = 0, mn = 1e300, pmx = 0, pmn = 1e300;
        for (uint32_t b = 0; b < G; ++b) { mx = std::max(mx, dur[b]); mn = std::min(mn, dur[b]); pmx = std::max(pmx, pred[b]); pmn = std::min(pmn, pred[b]); }
        std::fprintf(stderr, "trim round %u: workgroup durations min %.2f mean %.2f max %.2f us; %zu entries moved; predicted min %.2f max %.2f\n", in.trim_round + 1, mn / 100, mean / 100,
                     mx / 100, pool.size(), pmn / 100, pmx / 100);
        double xs[8] = {}, xw[8] = {}; uint32_t xn[8] = {};
        for (uint32_t b = 0; b < G; ++b) { xs[b & 7u] += dur[b]; xw[b & 7u] += weight[b]; xn[b & 7u]++; }
        std::fprintf(stderr, "   by XCD (workgroup %% 8): mean duration");
        for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %.2f", xs[k] / std::max(1u, xn[k]) / 100);
        std::fprintf(stderr, " ; mean weight");
        for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %.0f", xw[k] / std::max(1u, xn[k]));
        std::fprintf(stderr, "\n");
    }
#endif
    size_t rows_out = 0;
    for (uint32_t b = 0; b < G; ++b) {
        std::stable_sort(wg[b].begin(), wg[b].end(), [](const Ent& a, const Ent& b2) { return a.w > b2.w; });
        rows_out = std::max(rows_out, wg[b].size());
    }
    if (static_cast<size_t>(G) * rows_out > capacity) return false;
    out.entries.assign(static_cast<size_t>(G) * rows_out, PQ_NO_ITEM);
    out.shares.assign(static_cast<size_t>(G) * rows_out, 0);
    for (uint32_t b = 0; b < G; ++b)
        for (size_t r = 0; r < wg[b].size(); ++r) {
            out.entries[r * G + b] = wg[b][r].code;
            out.shares[r * G + b] = static_cast<uint16_t>(wg[b][r].w - 1u);
        }
    out.grid = G;
    out.view_serial = in.view_serial;
    out.has_dp = in.has_dp;
    out.trimmable = true;
    out.trim_round = in.trim_round + 1;
    out.final_for_view = out.trim_round >= set.trim_rounds;
    return true;
}

// device form of a list: {entry, x | y << 16 of the entry's 16x16 tile} (the kernel does no integer division)
void volym::list_to_device_form(const ShardGrid& g, const std::vector<uint32_t>& entries, uint32_t* out)
{
    for (size_t i = 0; i < entries.size(); ++i) {
        const uint32_t raw_p = entries[i];
        uint32_t xy = 0;
        if (raw_p != PQ_NO_ITEM) {
            const uint32_t tile = wl_local_tile(wl_code(raw_p)) * g.world + g.rank;
            xy = (tile % g.tiles_x) | ((tile / g.tiles_x) << 16);
        }
        out[2 * i] = raw_p;
        out[2 * i + 1] = xy;
    }
}

// costs by list position -> costs by item
void volym::costs_to_items(const WorkList& list, const uint16_t* cost, uint32_t n_entries, std::vector<uint16_t>& item_cost)
{
    std::vector<uint32_t> q_max(item_cost.size(), 0);
    std::vector<uint8_t> q_seen(item_cost.size(), 0);
    for (uint32_t p = 0; p < n_entries && p < list.entries.size(); ++p) {
        const uint32_t raw_p = list.entries[p];
        if (raw_p == PQ_NO_ITEM) continue;
        const uint32_t raw = wl_code(raw_p);
        const uint32_t k = cost[p];
        if (wl_is_quarter(raw)) {                                 // depth-parallel quarter: the tile's cost is 5 + the slowest quarter
            const uint32_t item = wl_quarter_item(raw);
            if (item < item_cost.size()) { q_max[item] = std::max(q_max[item], k); q_seen[item] = 1; }
        } else if (wl_is_super(raw)) {                      // super fill: zero, or the sum of four marched sub-tiles
            const uint32_t lt = wl_super_tile(raw);
            for (uint32_t sub = 0; sub < 4; ++sub)
                if (lt * 4u + sub < item_cost.size()) item_cost[lt * 4u + sub] = static_cast<uint16_t>(k == 0 ? 0u : std::max(1u, k / 4u));
        } else if (raw < item_cost.size()) {
            item_cost[raw] = static_cast<uint16_t>(k);
        }
    }
    for (size_t i = 0; i < item_cost.size(); ++i)
        if (q_seen[i]) item_cost[i] = static_cast<uint16_t>(std::min(65535u, 5u + q_max[i]));
}

// ---- the seam for tests/test_worklist.py (worklist.hpp) ----
static WorkList list_in(const volym_wl_list& l)
{
    WorkList w;
    w.entries.assign(l.entries, l.entries + l.n);
    w.shares.assign(l.shares, l.shares + l.n);
    w.grid = l.grid; w.trim_round = l.trim_round; w.view_serial = l.view_serial;
    w.has_dp = l.has_dp != 0; w.trimmable = l.trimmable != 0; w.final_for_view = l.final_for_view != 0;
    return w;
}

static int list_out(const WorkList& w, volym_wl_list* l)
{
    if (w.entries.size() > l->capacity || w.shares.size() != w.entries.size()) return VOLYM_E_INVALID;
    std::copy(w.entries.begin(), w.entries.end(), l->entries);
    std::copy(w.shares.begin(), w.shares.end(), l->shares);
    l->n = static_cast<uint32_t>(w.entries.size());
    l->grid = w.grid; l->trim_round = w.trim_round; l->view_serial = w.view_serial;
    l->has_dp = w.has_dp; l->trimmable = w.trimmable; l->final_for_view = w.final_for_view;
    return VOLYM_OK;
}

static bool arrays(const volym_wl_list* l) { return l && l->entries && l->shares; }

extern "C" {

int volym_wl_build_geometric(const ShardGrid* g, uint32_t* out, uint32_t capacity, uint32_t* n_out)
{
    if (!g || !out || !n_out) return VOLYM_E_INVALID;
    const std::vector<uint32_t> v = build_geometric(*g);
    if (v.size() > capacity) return VOLYM_E_INVALID;
    std::copy(v.begin(), v.end(), out);
    *n_out = static_cast<uint32_t>(v.size());
    return VOLYM_OK;
}

int volym_wl_deal_list(const ShardGrid* g, const ListSettings* set, const CapturedLaunch* job, int moving, const uint16_t* cost, uint8_t* item_is_dp, uint32_t n_items,
                       const uint32_t* geometric, uint32_t n_geometric, volym_wl_list* out)
{
    if (!g || !set || !job || !cost || !item_is_dp || !geometric || !arrays(out)) return VOLYM_E_INVALID;
    std::vector<uint8_t> is_dp(item_is_dp, item_is_dp + n_items);
    WorkList w;
    deal_list(*g, *set, *job, moving != 0, std::vector<uint16_t>(cost, cost + n_items), is_dp, std::vector<uint32_t>(geometric, geometric + n_geometric), w);
    std::copy(is_dp.begin(), is_dp.end(), item_is_dp);
    return list_out(w, out);
}

int volym_wl_trim_list(const ListSettings* set, const CapturedLaunch* job, uint32_t capacity, const volym_wl_list* in, const uint32_t* times, volym_wl_list* out)
{
    if (!set || !job || !arrays(in) || !times || !arrays(out)) return VOLYM_E_INVALID;
    WorkList w;
    if (!trim_list(*set, *job, capacity, list_in(*in), times, w)) return 0;      // (1: trimmed into `out`)
    const int rc = list_out(w, out);
    return rc == VOLYM_OK ? 1 : rc;
}

int volym_wl_list_to_device_form(const ShardGrid* g, const uint32_t* entries, uint32_t n, uint32_t* out)
{
    if (!g || !entries || !out) return VOLYM_E_INVALID;
    list_to_device_form(*g, std::vector<uint32_t>(entries, entries + n), out);
    return VOLYM_OK;
}

int volym_wl_costs_to_items(const volym_wl_list* list, const uint16_t* cost, uint32_t n_entries, uint16_t* item_cost, uint32_t n_items)
{
    if (!arrays(list) || !cost || !item_cost) return VOLYM_E_INVALID;
    std::vector<uint16_t> v(item_cost, item_cost + n_items);
    costs_to_items(list_in(*list), cost, n_entries, v);
    std::copy(v.begin(), v.end(), item_cost);
    return VOLYM_OK;
}

}  // extern "C"
