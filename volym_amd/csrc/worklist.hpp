// Internal: the work-list scheduler of variant 2 -- what list the persistent workgroups read.  Host only: plain integer and
// double arithmetic over values, no HIP, no context (the thread that runs it and the capture that feeds it are raymarch.hip's,
// "cost feedback").
//
// The kernel's persistent workgroups read a list of items; the frame time is set by how well that list balances the few
// hundred tiles whose rays take ~10x the average number of dependent samples.  Only a rendered frame knows which they
// are, so a launch can be asked to report a counted cost per list entry; those costs become the next list: most expensive
// entries first and dealt longest-processing-time first to the workgroups, the most expensive tiles split into four
// depth-parallel quarter items, constant 16x16 tiles merged into super-fill items (the entry's code: worklist_entry.h).
// Lists are scheduling only: every list renders the same pixels, so a list measured on a neighbouring view is a good list
// for this one.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "worklist_entry.h"

namespace volym {

// One work list as the kernel reads it: workgroup b takes entries b, b + grid, ... (raymarch_pq.h).
struct WorkList {
    std::vector<uint32_t> entries;   // host copy (the feedback thread maps list positions back to tiles)
    uint32_t grid = 0;               // workgroups the list was dealt to (0: the geometric list, any grid)
    uint64_t view_serial = 0;        // the view whose measured costs produced it (0: none, geometric order)
    bool has_dp = false;             // holds depth-parallel entries (their costs come back as estimates)
    bool trimmable = false;          // dealt for a standing view from costs measured on whole entries
    uint32_t trim_round = 0;         // times the list was re-balanced from measured workgroup times since it was dealt
    bool final_for_view = false;     // trimmable and trimmed as often as asked: no more captures
    std::vector<uint16_t> shares;    // by list position: the cost share the entry was dealt with (trimmable lists)
};

// The screen grid of one shard: local 16x16 tile lt is tile lt * world + rank of the tiles_x x tiles_y grid over W x H pixels.
struct ShardGrid {
    uint32_t W = 0, H = 0, tiles_x = 0, tiles_y = 0;
    uint32_t rank = 0, world = 1, n_local = 0;
};

// The scheduling settings: what volym_set_option writes and a capture copies for the feedback thread.
struct ListSettings {
    int dp_min_cost = -1;                  // split threshold: < 0 adaptive (-N: N/10 x a wave's fair share; -1: by mode), 0 no split, else the cost
    uint32_t dp_share_pct = 60;            // cost share of a quarter, percent of its tile's cost
    uint32_t dp_floor = 64;                // floor of the adaptive split threshold, cost units
    int dilate = -1;                       // radius (8x8 items) of the max-filter over the cost map before dealing; -1: 1 while the view moves, else 0
    bool super_fill = true;
    bool only_quarters = false;            // dev
    uint32_t dev_drop_tenths = 0;          // dev
    uint32_t trim_rounds = 0;              // re-balancing rounds from measured workgroup times after a standing view's list is dealt (VOLYM_OPT_REBALANCE_ROUNDS; off: see trim_list)
    uint32_t prio_tenths[3] = {3, 6, 10};  // issue-priority thresholds, tenths of the fair share ([0] == 0: no priorities)
};

// What the scheduler needs to know of the launch whose costs it is given.
struct CapturedLaunch {
    uint64_t view_serial = 0;
    bool captured_has_dp = false;            // the list it ran held depth-parallel entries
    bool continuous = false;
    bool plain = false;                      // table mode, no importance mode (the common instantiation)
    uint32_t max_grid = 0, waves = 16;
    uint32_t grid = 0;                       // workgroups of the captured launch
};

// geometric list: the 8x8-pixel wave tiles of the shard's 16x16 tiles, centre first
std::vector<uint32_t> build_geometric(const ShardGrid& g);
// Deal `measured_cost` (by item) into a list.  `moving`: the camera has moved since the captured frame.
void deal_list(const ShardGrid& g, const ListSettings& set, const CapturedLaunch& job, bool moving, const std::vector<uint16_t>& measured_cost,
               std::vector<uint8_t>& item_is_dp, const std::vector<uint32_t>& geometric, WorkList& out);
// Re-balance a standing view's list from the times its workgroups took; false: `out` is not a list (no more than `capacity` entries fit)
bool trim_list(const ListSettings& set, const CapturedLaunch& job, size_t capacity, const WorkList& in, const uint32_t* times, WorkList& out);
// device form of a list: {entry, x | y << 16 of the entry's 16x16 tile} (the kernel does no integer division)
void list_to_device_form(const ShardGrid& g, const std::vector<uint32_t>& entries, uint32_t* out);
// costs by list position -> costs by item
void costs_to_items(const WorkList& list, const uint16_t* cost, uint32_t n_entries, std::vector<uint16_t>& item_cost);

}  // namespace volym

// The same five over flat arrays, for tests/test_worklist.py ALONE (it binds them with ctypes): not part of the library's interface, not
// in include/.  0, or VOLYM_E_INVALID for a NULL or a result above the caller's capacity.
extern "C" {
struct volym_wl_list {             // a WorkList over the caller's arrays: `capacity` entries and shares each
    uint32_t* entries;
    uint16_t* shares;
    uint32_t capacity, n, grid, trim_round;
    uint64_t view_serial;
    uint8_t has_dp, trimmable, final_for_view;
};
int volym_wl_build_geometric(const volym::ShardGrid* g, uint32_t* out, uint32_t capacity, uint32_t* n_out);
int volym_wl_deal_list(const volym::ShardGrid* g, const volym::ListSettings* set, const volym::CapturedLaunch* job, int moving, const uint16_t* cost, uint8_t* item_is_dp,
                       uint32_t n_items, const uint32_t* geometric, uint32_t n_geometric, volym_wl_list* out);
int volym_wl_trim_list(const volym::ListSettings* set, const volym::CapturedLaunch* job, uint32_t capacity, const volym_wl_list* in, const uint32_t* times, volym_wl_list* out);
int volym_wl_list_to_device_form(const volym::ShardGrid* g, const uint32_t* entries, uint32_t n, uint32_t* out);
int volym_wl_costs_to_items(const volym_wl_list* list, const uint16_t* cost, uint32_t n_entries, uint16_t* item_cost, uint32_t n_items);
}
