// VARIANT 2 of the ray-march: persistent workgroups + per-wave shading queue (gfx950).
//
// Why this shape (profiles/ and DESIGN.md "Kernel v2"): with one pixel per lane and a monolithic
// loop, the kernel time was the latency of its longest rays -- ~80 dependent iterations of
// {byte gather -> classify -> 6 gradient gathers -> Blinn-Phong -> composite}, executed by waves in
// which a handful of lanes were still alive.  Three observations remove that chain:
//
//  1. CONTROL needs one byte per sample.  Positions, the step state machine, rho >= threshold, the
//     opacity alpha_step (a table of the byte), the alpha < 0.95 exit: none of it needs the gradient
//     or the shading.  So a lane runs only the control path, and every dense sample it accepts is
//     pushed into a per-wave LDS queue as {pos, weight w = (1-alpha)*alpha_step, class byte, owner}.
//  2. COLOUR is a sum of independent terms w_k * shade(pos_k).  Whenever 64 samples are queued the
//     whole wave shades them, one sample per lane, whoever owns them, and adds the result to the
//     owner's accumulator in LDS.  The accumulators are 4.28 fixed point and are updated with integer
//     atomics, so the sum is independent of the order of arrival: deterministic and identical on
//     every GPU/sharding.  (|error| <= 4e-9 per term; the budget is 1e-4.)
//  3. The control path itself is speculated K samples at a time: predict that the next K samples
//     have the class (dense / not dense) of the last one, which fixes their positions through the
//     step state machine; issue the K byte gathers together; then accept samples in order with the
//     REAL classes and stop at the first misprediction.  Accepted samples are bit-identical to the
//     sequential march (same f32 operations in the same order).
//
// Work distribution: persistent workgroups of PQ_WAVES waves, one per CU (it owns the CU's LDS).  Every workgroup reads a
// list of items -- workgroup b the entries b, b+G, b+2G, ... of `order` -- and its waves draw them through a ticket counter
// in LDS: dynamic balance inside the workgroup, no global atomics, nothing to reset between launches.  The first frame of
// a context runs the host's centre-first list (the orbit camera targets the volume centre, src/camera.rs:23); a launch can be
// asked to record a counted cost per list entry, from which a feedback thread on the host deals the next list (raymarch.hip,
// "cost feedback"; the policy is worklist.hpp): most expensive entries first, the most expensive tiles as depth-parallel quarter
// items, constant 16x16 tiles as super fill items.  Entries are {item code (worklist_entry.h), x | y << 16 of the entry's 16x16 tile}.
//
// Item kinds and their loops (all bit-identical to the sequential march):
//   * 8x8 tile, one lane per ray, K speculative samples per iteration ("classic");
//   * 4x4 quarter tile, four lanes per ray ("depth-parallel"): for the long chains of dependent samples a frame ends on;
//   * fill items: tiles the hulls prove constant.
// Template parameters: TABLE (nearest filter without smoothing: density is a table of the byte), COUNT (instrumented),
// TRACE (development), IMP (general flag handling) / IR (importance rendering on the specialised paths), BRICK (layout).
//
// Exact culling (results unchanged, DESIGN.md "Culling"):
//   * no sample outside the AABB of the occupied macro cells can reach the threshold, so a ray is
//     replayed (t += cur in f32, no fetches) up to the AABB entry and abandoned at its exit; a ray that
//     misses the AABB is final at (0,0,0,0).  With the tile mask, the entry and exit are also clipped to
//     the depth range of the occupied cells that project onto the ray's 8x8 tile (CULL_TILE_DEPTH);
//   * a wave tile whose 8x8 pixel rectangle lies outside the projected cube stores (0,0,0,1) and one
//     inside the cube but outside the projected AABB stores (0,0,0,0) without any per-ray work.  Both
//     tests use hulls projected on the host and a 1.5 pixel safety margin; tiles that straddle an
//     edge take the exact per-ray path.
// The instrumented (COUNT) launch disables culling: it counts what the reference would fetch.
#pragma once

#include <cstddef>
#include <type_traits>

#include "raymarch_device.h"
#include "worklist_entry.h"

namespace volym {

constexpr int PQ_WAVES = 16;             // waves per workgroup of the common instantiation (see WAVES below)
constexpr int PQ_WAVES_WIDE = 12;        // ... of the instantiations that need more than 128 VGPRs
constexpr uint32_t PQ_MIN_LEAP_D = 2;    // smallest distance-field value worth a leap
constexpr int PQ_DP_DEPTH = 2;           // depth-parallel items: samples per lane and iteration (4 lanes per ray)
constexpr int PQ_ITEMS_LDS = 512;       // work-list entries staged in LDS per workgroup (the rest stay in global memory)
// ring entries per wave: < 64 left over from the last iteration + 64 per speculative sample of this one.  One workgroup
// per CU owns the whole 160 KB of LDS, so the queue is sized for the shading to run at ONE point of the loop.
constexpr int pq_qcap(int k) { return 64 + 64 * k; }
constexpr float PQ_FIX_SCALE = 268435456.0f;        // 2^28
constexpr float PQ_FIX_INV = 1.0f / 268435456.0f;

__device__ __forceinline__ uint32_t lane_rank_in_mask(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum : uint32_t { TILE_MARCH = 0, TILE_HIT_TEST = 1, TILE_FILL_EMPTY = 2, TILE_FILL_MISS = 3 };

// Classify the pixel rectangle [x0, x0+extent] x [y0, y0+extent] against the two projected hulls (wave-uniform
// result; lane l evaluates hull l>>5, edge (l>>2)&7, corner l&3).
// The lane's edge (a, b, c, valid) is fetched once per kernel (HullEdge): indexing the kernel arguments by lane is a
// memory gather, and a fill tile is little else.
struct HullEdge { float a, b, c; bool valid; };
__device__ __forceinline__ HullEdge load_hull_edge(const FrameParams& fp, uint32_t lane)
{
    // one gather from the kernel-argument segment per kernel
    const uint32_t h = lane >> 5, e = (lane >> 2) & 7u;
    HullEdge r;
    r.a = fp.hull[h][e][0]; r.b = fp.hull[h][e][1]; r.c = fp.hull[h][e][2]; r.valid = fp.hull[h][e][3] > 0.5f;
    return r;
}
__device__ __forceinline__ uint32_t classify_tile(const FrameParams& fp, const HullEdge& edge, uint32_t lane, float x0, float y0, float extent = 7.0f,
                                                   bool masked_out = false)
{
    const uint32_t k = lane & 3u;
    const float cx = (k & 1u) ? x0 + extent : x0, cy = (k & 2u) ? y0 + extent : y0;
    const float a = edge.a, b = edge.b, c = edge.c;
    const bool valid = edge.valid;
    const float v = __builtin_fmaf(a, cx, __builtin_fmaf(b, cy, c));
    const float margin = 1.5f;
    const unsigned long long mo = __ballot(valid && v < -margin);     // corner strictly outside edge
    const unsigned long long mi = __ballot(!valid || v > margin);     // corner strictly inside edge
    auto outside = [&](uint32_t bits) { return ((bits & (bits >> 1) & (bits >> 2) & (bits >> 3)) & 0x11111111u) != 0u; };
    const bool cube_ok = (fp.cull & CULL_CUBE_HULL) != 0u, obj_ok = (fp.cull & CULL_OBJ_HULL) != 0u;
    const bool out_cube = cube_ok && outside(static_cast<uint32_t>(mo));
    const bool in_cube = cube_ok && static_cast<uint32_t>(mi) == 0xffffffffu;
    const bool out_obj = masked_out || (fp.cull & CULL_NOTHING_DENSE) != 0u || (obj_ok && outside(static_cast<uint32_t>(mo >> 32)));
    if (out_cube) return TILE_FILL_MISS;
    if (out_obj) return in_cube ? TILE_FILL_EMPTY : TILE_HIT_TEST;
    return TILE_MARCH;
}
// tile_mask bit of the 8x8 tile (t8x, t8y) (wave-uniform).  The buffer fp.tile_mask names is written by the slot's mask kernel alone,
// earlier on the slot's own stream (raymarch.hip, ensure_frame_resources: every frame slot has its pair of buffers); a march writes
// only the other buffer of the pair (tile_mask_spare).  So it is read as tile_depth is: a scalar load
__device__ __forceinline__ bool tile_mask_bit(const FrameParams& fp, uint32_t t8x, uint32_t t8y)
{
    const uint32_t bit = t8y * fp.mask_t8x + t8x;
    return ((launch_constant(fp.tile_mask)[bit >> 5] >> (bit & 31u)) & 1u) != 0u;
}
// whether any of the four 8x8 tiles of the 16x16 tile (tx16, ty16) has its bit set.  A row of the mask is an even number of bits
// (mask_t8x is twice the frame's 16x16 tiles per row), so each row's pair starts at an even bit and lies in one word: two scalar
// loads, both issued before either is waited for
__device__ __forceinline__ bool tile_mask_any16(const FrameParams& fp, uint32_t tx16, uint32_t ty16)
{
    const auto* mask = launch_constant(fp.tile_mask);
    const uint32_t bit0 = ty16 * 2u * fp.mask_t8x + tx16 * 2u, bit1 = bit0 + fp.mask_t8x;
    const uint32_t w0 = mask[bit0 >> 5], w1 = mask[bit1 >> 5];
    return (((w0 >> (bit0 & 31u)) | (w1 >> (bit1 & 31u))) & 3u) != 0u;
}
// The arguments of volym_raymarch_pq_kernel as the kernel-argument segment lays them out (every argument at its natural alignment, in
// order: the layout of this struct), for the one thing the kernel needs to know about its own segment: where `fp` sits.
// tests/test_kernel_resources.py compares the figure with the .offset the compiler writes into the code object's metadata.
struct PqKernelArgs {
    const uint8_t* vol; const uint8_t* imp; const FrameTables* tables; const uint8_t* df4; const uint2* order; uint32_t n_items; uint16_t* cost;
    uint32_t* out_shard; uint32_t* out_raster; float4* out_f32; Counters* counters; uint4* trace; FrameParams fp;
};
constexpr size_t PQ_FP_KERNARG_OFFSET = offsetof(PqKernelArgs, fp);
static_assert(PQ_FP_KERNARG_OFFSET % 8 == 0 && alignof(FrameParams) == 8, "FrameParams holds pointers: 8-byte aligned in the segment");

// WAVES: waves per workgroup.  16 (four per SIMD, a budget of 128 VGPRs) for the common instantiation, which fits; the
// importance / continuous-rho instantiations need ~150 registers and run 12 waves (three per SIMD, 168 VGPRs) instead of
// spilling 64-100 bytes per lane to scratch (profiles/r02_kernel_resources.txt).
// CJ (with IR): the look-ahead's walks as jobs shared by the waves of the workgroup ("cone jobs" below): 1 the cone look-ahead (a
// record on 8 lanes, one per direction), 2 the straight look-ahead (a record on one lane)
// LB (development build only, north_star "LDS-staged voxel bricks"): the K speculative voxel fetches of an iteration go through a
// per-wave cache of 4x4x4 bricks in LDS, filled with one coalesced 64-byte read per brick (16 lanes x 4 bytes) -- the A/B of
// profiles/r03_lds_bricks_ab.txt.  Bricked layout, common instantiation only.
// RELOAD: every list entry reads the frame parameters of its set-up afresh from the kernel-argument segment (below, at the top of the
// ticket loop) instead of holding them in scalar registers for the whole launch
// The kernel's body is raymarch_pq_body.h, included by this kernel (CUBE256 = false) and by its twin for volumes of 256 texels on every
// axis, volym_raymarch_cube256_kernel below (CUBE256 = true): one text, so that the two cannot drift apart.  An inlined
// __device__ function template would be the plainer way to share it and was built first; it changes the machine code of every
// instantiation of this kernel (DESIGN.md 5, 2026-10-21, and profiles/cube256_asm_equal.txt say why), which the listing tests and the
// measured history of these kernels rest on.
template <bool TABLE, bool COUNT, bool TRACE = false, int KSPEC = 1, bool IMP = true, bool BRICK = false, bool IR = false, int WAVES = PQ_WAVES, int CJ = 0, bool LB = false,
          bool RELOAD = true>
__global__ __launch_bounds__(WAVES * 64) void volym_raymarch_pq_kernel(
    const uint8_t* __restrict__ vol, const uint8_t* __restrict__ imp, const FrameTables* __restrict__ tables,
    const uint8_t* __restrict__ df4, const uint2* __restrict__ order, uint32_t n_items, uint16_t* __restrict__ cost,
    uint32_t* __restrict__ out_shard, uint32_t* __restrict__ out_raster, float4* __restrict__ out_f32,
    Counters* __restrict__ counters, uint4* __restrict__ trace, const FrameParams fp)
{
    constexpr bool CUBE256 = false;
#include "raymarch_pq_body.h"
}

// The twin of the headline instantiation for a volume of 256 x 256 x 256 texels in the linear layout: its texel addresses are the three
// clamped coordinates as bytes side by side (raymarch_device.h, texel256_*).  The same template parameters and the same argument list
// as volym_raymarch_pq_kernel, so PqKernelArgs and PQ_FP_KERNARG_OFFSET hold for it (tests/test_cube256_listing.py compares the offset
// with the code object's metadata).  Instantiated once, for the headline flags, in raymarch_common.hip.
template <bool TABLE, bool COUNT, bool TRACE = false, int KSPEC = 1, bool IMP = true, bool BRICK = false, bool IR = false, int WAVES = PQ_WAVES, int CJ = 0, bool LB = false,
          bool RELOAD = true>
__global__ __launch_bounds__(WAVES * 64) void volym_raymarch_cube256_kernel(
    const uint8_t* __restrict__ vol, const uint8_t* __restrict__ imp, const FrameTables* __restrict__ tables,
    const uint8_t* __restrict__ df4, const uint2* __restrict__ order, uint32_t n_items, uint16_t* __restrict__ cost,
    uint32_t* __restrict__ out_shard, uint32_t* __restrict__ out_raster, float4* __restrict__ out_f32,
    Counters* __restrict__ counters, uint4* __restrict__ trace, const FrameParams fp)
{
    constexpr bool CUBE256 = true;
    static_assert(TABLE && !COUNT && !TRACE && KSPEC == 4 && !IMP && !BRICK && !IR && WAVES == PQ_WAVES && CJ == 0 && !LB && RELOAD,
                  "the 256-cubed twin exists for the headline flags only");
#include "raymarch_pq_body.h"
}

}  // namespace volym
