// The code of one work-list entry (variant 2), defined ONCE for the host that deals the lists (worklist.cpp) and the kernel
// that reads them (raymarch_pq.h).  Plain C++ and device code.
//
// An entry is one u32:
//   * item = local_tile*4 + sub: an 8x8 wave tile, one lane per ray;
//   * bit 31 | (item << 2) | quarter: for tiles the cost feedback found expensive, a 4x4 quarter tile marched
//     DEPTH-PARALLEL, four lanes per ray, lane k of a quad taking the k-th speculative sample (raymarch_pq.h "dp");
//   * bit 30 (bit 31 clear) | local_tile: a whole 16x16 tile that was constant in the frame the costs were measured on
//     ("super fill").  One classification of the 16x16 rectangle and, if it still says "constant", 16-byte stores;
//     otherwise its four sub-tiles are processed one after the other;
//   * bits 28-29 of any of them: issue priority the host derived from the measured cost.  The frame ends with its longest
//     chains of dependent samples; a wave that carries one gets the SIMD's issue slots first, the cheap items fill the gaps.
//     (Only while every code of the shard stays below bit 28: worklist.cpp deal_list.);
//   * PQ_NO_ITEM: padding, tested before anything else.
#pragma once

#include <cstdint>

#include "wgsl_math.h"   // VOLYM_HD

namespace volym {

constexpr uint32_t PQ_NO_ITEM = 0xffffffffu;   // padding of the work list
constexpr uint32_t WL_QUARTER = 0x80000000u;   // bit 31
constexpr uint32_t WL_SUPER = 0x40000000u;     // bit 30
constexpr uint32_t WL_PRIO_SHIFT = 28u, WL_PRIO_MASK = 0x30000000u;   // bits 28-29

// ---- encode ----
VOLYM_HD constexpr uint32_t wl_item(uint32_t item) { return item; }
VOLYM_HD constexpr uint32_t wl_quarter(uint32_t item, uint32_t quarter) { return WL_QUARTER | (item << 2) | quarter; }
VOLYM_HD constexpr uint32_t wl_super(uint32_t local_tile) { return WL_SUPER | local_tile; }
VOLYM_HD constexpr uint32_t wl_with_prio(uint32_t code, uint32_t prio) { return code | (prio << WL_PRIO_SHIFT); }

// ---- decode (of an entry that is not PQ_NO_ITEM): the priority and the code without it, then the code's kind and fields ----
VOLYM_HD constexpr uint32_t wl_prio(uint32_t entry) { return (entry >> WL_PRIO_SHIFT) & 3u; }
VOLYM_HD constexpr uint32_t wl_code(uint32_t entry) { return entry & ~WL_PRIO_MASK; }
VOLYM_HD constexpr bool wl_is_quarter(uint32_t code) { return (code >> 31) != 0u; }
VOLYM_HD constexpr bool wl_is_super(uint32_t code) { return (code >> 30) == 1u; }
VOLYM_HD constexpr uint32_t wl_super_tile(uint32_t code) { return code & (WL_SUPER - 1u); }            // of a super fill
VOLYM_HD constexpr uint32_t wl_quarter_item(uint32_t code) { return (code & (WL_QUARTER - 1u)) >> 2; }   // of a quarter
VOLYM_HD constexpr uint32_t wl_quarter_index(uint32_t code) { return code & 3u; }                        // of a quarter
// the local 16x16 tile of any kind of code
VOLYM_HD constexpr uint32_t wl_local_tile(uint32_t code)
{
    return wl_is_quarter(code) ? ((code & (WL_QUARTER - 1u)) >> 4) : (wl_is_super(code) ? wl_super_tile(code) : (code >> 2));
}

}  // namespace volym
