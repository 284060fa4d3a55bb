// The kernels of the cost pass (volym_cost_pass).  Included by cost.hip alone.  The pieces it shares with the geodesic pass (the
// tile state, the marking, the counting helper) are copies, for the reason of DESIGN.md 4.20 and 4.21: no existing unit includes
// anything new, so every kernel of theirs stays as it is.
//
// The pass: for every texel t of a request's box the key cost(t) << 8 | cost_label(t) (include/volym_hip.h has the rule),
// box-linear.  The keys are the one fixed point of key(t) = min(key(t), min over the six neighbours u of key(u) + (step(u, t) << 8))
// on the medium, the seeds held at their label; every kernel below only ever lowers a word towards it, so whatever order anything
// runs in the bytes agree.
//   zero     the summary, the state's header and the tiles' round flags.
//   init     one wave per row (box_walk.h's walk, layout_offset, either layout): the only kernel that reads scene bytes.  It stores
//            the label on a seed, OPEN on a medium texel, NONE elsewhere, and the density byte of EVERY texel of the box, box-linear,
//            into the pass's byte map: the relax kernel's loads are then coalesced and the same in either layout, and the snapshot
//            does not depend on later edits.  It counts n_seed and n_medium and marks round 0's tiles as the geodesic pass does.
//   relax    one workgroup per ACTIVE tile of COST_TX x COST_TY x COST_TZ texels, round after round.  It loads the tile and a halo of
//            one texel from the key map and from the byte map into LDS, works out each lane's step costs once, iterates in LDS until
//            an iteration lowers nothing (a flag in LDS and one barrier; __syncthreads_or would do, but the library's reduction behind
//            it reserves 260 bytes of LDS of its own, and the kernel is to hold no more than its arrays), stores the words that changed,
//            and for every face on which one changed marks the tile beyond it active FOR THE NEXT ROUND.
//   finish   one wave per row of the key map: OPEN becomes NONE, and the summary through LDS.
//   pack     one thread: the (cost, ~index) key of the maximum becomes max_cost and max_at.
//
// Why no workgroup waits for another, and why no freshness is needed -- for weights.  A relax workgroup reads words of other tiles
// (its halo) that their owners may be storing in the same launch.  Such a load returns the word as it was at some time since the
// launch before, and ANY of those values is an upper bound of the final key: words only decrease, and a word is only ever set to a
// key(u) + step of a word that was itself an upper bound.  That a word can now be lowered many times changes nothing in this.  A
// stale halo only delays a lowering: the owner that lowered a face word has marked this tile, by an atomic on the NEXT round's
// flags and list, which are read only after the kernel boundary.  When a round marks nothing, every tile was last relaxed against
// halo words that have not changed since: a fixed point, and there is one (every step costs at least 1).
//   The rounds.  After round r every texel is final to which some cheapest chain crosses at most r tile faces.  r = 0: the seeds
// are final from the init kernel, round 0 relaxes every tile that holds a seed or has one in its halo, and a tile's iteration runs
// to the fixed point of the tile against its halo, which is at most the cost along any chain that stays inside the tile from a
// final word of the tile or halo.  r -> r + 1: let the chain's last crossing go from u (tile A) to v (tile B).  u is final after
// round r by induction; the round q <= r whose relaxation stored u's final value lowered a word on A's face towards B -- or u is a
// seed on that face -- so B is marked for a round q + 1 <= r + 1 (or round 0), which loads u after a kernel boundary and relaxes
// the rest of the chain inside B.  A cheapest chain visits no texel twice, so it crosses fewer faces than the box has texels: the
// host's guard of (texels + 2) rounds bounds ROUNDS, and holds however often a single word is lowered.
//
// The state (uint32 words) is the geodesic pass's: [0..2] the counts of three consecutive rounds, [4..5] the 64-bit key of the
// maximum, [6..7] the tiles relaxed so far, then flag[2][n_tiles] and list[2][n_tiles], by round parity.  Every load and store of
// the maps is of a texel inside the box (index below the box's texel count <= 2^31 - 2); every tile index is checked against
// n_tiles before it is used.
#pragma once

#include "box_walk.h"

namespace volym {

constexpr uint32_t COST_TX = 32u, COST_TY = 8u, COST_TZ = 8u;   // the tile: 2048 texels, 8 per lane of a 256-lane workgroup
constexpr uint32_t COST_LX = COST_TX + 2u, COST_LY = COST_TY + 2u, COST_LZ = COST_TZ + 2u;   // ... with its halo in LDS: 3400 texels
static_assert(COST_TX * COST_TY == 256u && COST_TX == 32u, "a lane owns one (x, y) of the tile and walks its z; the init kernel marks tiles per half wave");

constexpr uint32_t COST_NONE = VOLYM_COST_NONE;
constexpr uint32_t COST_OPEN = 0xfffffffeu;                     // medium, not reached yet (internal: finish turns it into NONE)
// the state's header
enum { CT_COUNT = 0, CT_MAX_KEY = 4, CT_RELAXED = 6, CT_HEADER = 8 };
// struct volym_cost_summary as 64-bit words
enum { CS_N_SEED = 0, CS_N_MEDIUM = 1, CS_N_REACHED = 2, CS_MAX = 3, CS_CELL = 5, CS_CELL_MEDIUM = 5 + 256, CS_HIST = 5 + 512, COST_SUMMARY_WORDS = 5 + 768 };

// The overflow trap.  key(u) + (step << 8) can pass 2^32 (a key is up to 0xfffffdff, a step << 8 up to 0xff0000), where the geodesic
// pass's key + 256 could not.  The sum is therefore formed SATURATING in 32 bits: it is the exact 64-bit sum clamped to 2^32 - 1,
// which is NONE and above every key the limit admits, so a sum that would wrap is refused by the same comparison that refuses a
// chain past the limit, and an OPEN or NONE neighbour (>= 2^32 - 2, plus at least 256) saturates too.
static_assert((static_cast<uint64_t>(VOLYM_COST_MAX) << 8 | 0xffu) < COST_OPEN && static_cast<uint64_t>(COST_OPEN) + (1u << 8) > 0xffffffffull && VOLYM_COST_STEP_MAX == 255u + 255u * 255u &&
              (static_cast<uint64_t>(VOLYM_COST_STEP_MAX) << 8) < (1ull << 32),
              "candidates are compared as the 64-bit sum clamped to 2^32 - 1: every admitted key lies below OPEN, OPEN plus the least step saturates");

// the box as tiles, and the weights
struct CostTiles {
    uint32_t w, h, d;                   // the box's extents, none 0
    uint32_t ntx, nty, ntz, n_tiles;    // ceil(extent / tile extent), and their product
    uint32_t max_key;                   // max_cost << 8 | 0xff: the largest key the limit admits
    uint32_t step_cost, contrast_cost;  // 1..255, 0..255
};

// what the init kernel reads of the request beside the walk's arguments
struct CostRequest {
    uint8_t seed[256], through[256];
    uint32_t max_byte, n_points;
    uint32_t points[VOLYM_COST_POINTS_MAX][3];
};

__device__ __forceinline__ uint32_t* cost_flags(uint32_t* state, const CostTiles& g, uint32_t parity) { return state + CT_HEADER + parity * g.n_tiles; }
__device__ __forceinline__ uint32_t* cost_list(uint32_t* state, const CostTiles& g, uint32_t parity) { return state + CT_HEADER + (2u + parity) * g.n_tiles; }

// tile t is active in the round of `parity`, whose count is *count: the first to set its flag appends it
__device__ __forceinline__ void cost_mark(uint32_t* flags, uint32_t* list, uint32_t* count, uint32_t n_tiles, uint32_t t)
{
    if (t >= n_tiles) return;
    if (atomicExch(&flags[t], 1u) == 0u) {
        const uint32_t at = atomicAdd(count, 1u);
        if (at < n_tiles) list[at] = t;
    }
}

// the 64-bit sum key + step8, clamped to 2^32 - 1 (one v_add_u32 with clamp)
__device__ __forceinline__ uint32_t cost_add(uint32_t key, uint32_t step8) { return __builtin_elementwise_add_sat(key, step8); }

// step(u, t) << 8 from the two density bytes
__device__ __forceinline__ uint32_t cost_step8(const CostTiles& g, uint32_t bu, uint32_t bt)
{
    const uint32_t diff = bu > bt ? bu - bt : bt - bu;
    return (g.step_cost + g.contrast_cost * diff) << 8;
}

// the summary at rest, the header and the flags of both parities.  Any grid.
__global__ __launch_bounds__(256) void volym_cost_zero_kernel(unsigned long long* __restrict__ summary, uint32_t* __restrict__ state, uint32_t n_state)
{
    const uint32_t i0 = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x == 0u) {
        for (uint32_t i = threadIdx.x; i < COST_SUMMARY_WORDS; i += 256u) summary[i] = i == CS_MAX ? static_cast<unsigned long long>(COST_NONE) : 0ull;
    }
    for (uint32_t i = i0; i < n_state; i += gridDim.x * 256u) state[i] = 0u;
}

// ---- 1. init ----------------------------------------------------------------------------------------------------------------------------
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_cost_init_kernel(BoxWalkArgs a, CostRequest q, CostTiles g, uint32_t* __restrict__ keys, uint8_t* __restrict__ bytes,
                                                              uint32_t* __restrict__ state, unsigned long long* __restrict__ summary)
{
    __shared__ uint8_t s_seed[256], s_through[256];
    __shared__ uint32_t s_points[VOLYM_COST_POINTS_MAX][3];
    s_seed[threadIdx.x] = q.seed[threadIdx.x];
    s_through[threadIdx.x] = q.through[threadIdx.x];
    if (threadIdx.x < 3u * VOLYM_COST_POINTS_MAX) s_points[threadIdx.x / 3u][threadIdx.x % 3u] = q.points[threadIdx.x / 3u][threadIdx.x % 3u];
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* const flags = cost_flags(state, g, 0u);
    uint32_t* const list = cost_list(state, g, 0u);
    uint32_t* const count = state + CT_COUNT;
    unsigned long long wave_seed = 0ull, wave_medium = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        const uint32_t ry = row % a.h, rz = row / a.h;
        const uint32_t y = a.lo[1] + ry, z = a.lo[2] + rz;
        const uint32_t base = row * a.w;
        const uint32_t ty = ry / COST_TY, tz = rz / COST_TZ;
        // the points of this row, one per lane (at most 64 of them): uniform, and 0 in all but a few rows
        const uint64_t row_points = __ballot(lane < q.n_points && s_points[lane][1] == y && s_points[lane][2] == z);
        for (uint32_t x0 = 0u; x0 < a.w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < a.w;
            bool seed = false, medium = false;
            uint32_t label = 0u;
            if (in) {
                const uint32_t o = layout_offset(a.bricked != 0u, bx, bxy, a.lo[0] + xi, y, z);
                const uint32_t b = a.vol[o];
                const bool window = b >= a.min_byte && b <= q.max_byte;
                bool point = false;
                for (uint64_t m = row_points; m != 0ull; m &= m - 1ull)
                    if (s_points[__builtin_ctzll(m)][0] == a.lo[0] + xi) point = true;
                if (LABELS && (window || point)) label = a.labels[o];
                seed = point || (window && s_seed[label] != 0u);
                medium = window && s_through[label] != 0u;
                keys[base + xi] = seed ? label : (medium ? COST_OPEN : COST_NONE);
                bytes[base + xi] = static_cast<uint8_t>(b);                // every texel of the box: a step's cost reads both its ends
            }
            const uint64_t s = __ballot(seed);
            wave_seed += static_cast<uint32_t>(__popcll(s));
            wave_medium += static_cast<uint32_t>(__popcll(__ballot(medium && !seed)));
            if (s == 0ull) continue;                                        // (uniform)
            // Round 0's tiles, per half wave (x0 is a multiple of 64, a tile is 32 wide): the tile of a seed, and the tile beyond
            // each face a seed of the half lies on -- a seed on a face lowers that neighbour's texels though its own tile stores nothing.
            const uint32_t half = lane >> 5, l5 = lane & 31u;
            const uint32_t hs = static_cast<uint32_t>(s >> (32u * half));   // the seeds of this lane's half
            if (l5 == 0u && hs != 0u) {
                const uint32_t tx = x0 / COST_TX + half;
                const uint32_t t = tx + g.ntx * (ty + g.nty * tz);
                cost_mark(flags, list, count, g.n_tiles, t);
                if ((hs & 1u) && tx > 0u) cost_mark(flags, list, count, g.n_tiles, t - 1u);
                if ((hs >> 31) && tx + 1u < g.ntx) cost_mark(flags, list, count, g.n_tiles, t + 1u);
                if (ry % COST_TY == 0u && ty > 0u) cost_mark(flags, list, count, g.n_tiles, t - g.ntx);
                if (ry % COST_TY == COST_TY - 1u && ty + 1u < g.nty) cost_mark(flags, list, count, g.n_tiles, t + g.ntx);
                if (rz % COST_TZ == 0u && tz > 0u) cost_mark(flags, list, count, g.n_tiles, t - g.ntx * g.nty);
                if (rz % COST_TZ == COST_TZ - 1u && tz + 1u < g.ntz) cost_mark(flags, list, count, g.n_tiles, t + g.ntx * g.nty);
            }
        }
    }
    if (lane == 0u && wave_seed) atomicAdd(&summary[CS_N_SEED], wave_seed);
    if (lane == 0u && wave_medium) atomicAdd(&summary[CS_N_MEDIUM], wave_medium);
}

// What a relax workgroup holds in LDS, as one object so that nothing is padded between its parts: 17 016 bytes.
struct CostTileLds {
    uint32_t key[COST_LZ][COST_LY][COST_LX];    // the keys of the tile and its halo
    uint32_t word[4];                           // [0..2] the iteration flags, in rotation; [3] the bits of the faces that changed
    uint8_t byte[COST_LZ][COST_LY][COST_LX];    // the density bytes of the same texels
};
static_assert(sizeof(CostTileLds) == 5u * COST_LX * COST_LY * COST_LZ + 16u, "the arrays and nothing else");

// ---- 2. relax: one round ----------------------------------------------------------------------------------------------------------------
// A fixed grid strides over the round's list, whose count sits in device memory.  Lane (x, y) of the workgroup owns the 8 texels
// (x, y, 0..7) of the tile and walks them in ascending z on even iterations, descending on odd ones, in place in LDS: a word another
// lane is lowering reads as either value, and either is an upper bound.  The lane's step costs -- four lateral ones per texel and
// the nine along its column, each already << 8 -- are worked out once per tile visit from the bytes in LDS and stay in registers;
// an iteration reads keys only.  NONE words (neither seed nor medium, or outside the box) are never written; a seed's word is its
// label, below every key(u) + (step << 8), so min() never moves it.  A byte outside the box reads as 0: the key beside it is NONE.
__global__ __launch_bounds__(256) void volym_cost_relax_kernel(CostTiles g, uint32_t* __restrict__ keys, const uint8_t* __restrict__ bytes, uint32_t* __restrict__ state,
                                                               uint32_t round)
{
    __shared__ CostTileLds lds;
    auto& s_key = lds.key;
    auto& s_byte = lds.byte;
    uint32_t* const s_lowered = lds.word;
    uint32_t& s_faces = lds.word[3];
    const uint32_t parity = round & 1u;
    uint32_t* const flags = cost_flags(state, g, parity);
    const uint32_t* const list = cost_list(state, g, parity);
    uint32_t* const next_flags = cost_flags(state, g, parity ^ 1u);
    uint32_t* const next_list = cost_list(state, g, parity ^ 1u);
    uint32_t* const next_count = state + CT_COUNT + (round + 1u) % 3u;
    const uint32_t n = min(state[CT_COUNT + round % 3u], g.n_tiles);
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        state[CT_COUNT + (round + 2u) % 3u] = 0u;
        *reinterpret_cast<unsigned long long*>(state + CT_RELAXED) += n;       // (one thread of one launch at a time)
    }
    const uint32_t lx = threadIdx.x % COST_TX, ly = threadIdx.x / COST_TX;
    const uint32_t x = lx + 1u, y = ly + 1u;

    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t t = list[i];
        if (t >= g.n_tiles) continue;                                       // (uniform; never taken: the list holds what cost_mark stored)
        const uint32_t tx = t % g.ntx, ty = (t / g.ntx) % g.nty, tz = t / (g.ntx * g.nty);
        const uint32_t ox = tx * COST_TX, oy = ty * COST_TY, oz = tz * COST_TZ;    // the tile's first texel in the box
        if (threadIdx.x == 0u) { flags[t] = 0u; s_faces = 0u; s_lowered[0] = s_lowered[1] = s_lowered[2] = 0u; }
        // the tile and its halo; NONE and byte 0 outside the box (a word with index -1 wraps to >= the extent)
        for (uint32_t j = threadIdx.x; j < COST_LX * COST_LY * COST_LZ; j += 256u) {
            const uint32_t jx = j % COST_LX, jy = (j / COST_LX) % COST_LY, jz = j / (COST_LX * COST_LY);
            const uint32_t vx = ox + jx - 1u, vy = oy + jy - 1u, vz = oz + jz - 1u;
            const bool in = vx < g.w && vy < g.h && vz < g.d;
            const uint32_t at = vx + g.w * (vy + g.h * vz);
            s_key[jz][jy][jx] = in ? keys[at] : COST_NONE;
            s_byte[jz][jy][jx] = in ? bytes[at] : static_cast<uint8_t>(0u);
        }
        __syncthreads();
        uint32_t was[COST_TZ], sx0[COST_TZ], sx1[COST_TZ], sy0[COST_TZ], sy1[COST_TZ], sz[COST_TZ + 1u];
        {
            uint32_t below = s_byte[0u][y][x];
#pragma unroll
            for (uint32_t k = 0u; k < COST_TZ; ++k) {
                const uint32_t z = k + 1u, b = s_byte[z][y][x];
                was[k] = s_key[z][y][x];
                sx0[k] = cost_step8(g, s_byte[z][y][x - 1u], b);
                sx1[k] = cost_step8(g, s_byte[z][y][x + 1u], b);
                sy0[k] = cost_step8(g, s_byte[z][y - 1u][x], b);
                sy1[k] = cost_step8(g, s_byte[z][y + 1u][x], b);
                sz[k] = cost_step8(g, below, b);                            // the step between z - 1 and z
                below = b;
            }
            sz[COST_TZ] = cost_step8(g, below, s_byte[COST_TZ + 1u][y][x]);
        }

        for (uint32_t it = 0u;; ++it) {
            int lowered = 0;
            // (k is a constant wherever this is called, so that the step arrays stay in registers)
            const auto relax = [&](uint32_t k) {
                const uint32_t z = k + 1u;
                const uint32_t own = s_key[z][y][x];
                if (own == COST_NONE) return;
                const uint32_t m = min(min(min(cost_add(s_key[z][y][x - 1u], sx0[k]), cost_add(s_key[z][y][x + 1u], sx1[k])),
                                           min(cost_add(s_key[z][y - 1u][x], sy0[k]), cost_add(s_key[z][y + 1u][x], sy1[k]))),
                                       min(cost_add(s_key[z - 1u][y][x], sz[k]), cost_add(s_key[z + 1u][y][x], sz[k + 1u])));
                if (m <= g.max_key && m < own) { s_key[z][y][x] = m; lowered = 1; }
            };
            if (it & 1u) {
#pragma unroll
                for (uint32_t k = 0u; k < COST_TZ; ++k) relax(COST_TZ - 1u - k);
            } else {
#pragma unroll
                for (uint32_t k = 0u; k < COST_TZ; ++k) relax(k);
            }
            // Did any lane lower a word?  One flag per iteration, three in rotation: lanes set flag[it % 3] before the barrier and read
            // it after; lane 0 then clears flag[(it + 2) % 3], which every lane read before this barrier and none sets before the next.
            if (lowered) s_lowered[it % 3u] = 1u;
            __syncthreads();
            const uint32_t any = s_lowered[it % 3u];
            if (threadIdx.x == 0u) s_lowered[(it + 2u) % 3u] = 0u;
            if (!any) break;                                                // (uniform)
        }

        // the words that changed go to the map; the faces they lie on
        uint32_t faces = 0u;
#pragma unroll
        for (uint32_t k = 0u; k < COST_TZ; ++k) {
            const uint32_t v = s_key[k + 1u][y][x];
            if (v != was[k]) {                                              // (a word that is NONE outside the box never changes)
                keys[(ox + lx) + g.w * ((oy + ly) + g.h * (oz + k))] = v;
                faces |= (lx == 0u ? 1u : 0u) | (lx == COST_TX - 1u ? 2u : 0u) | (ly == 0u ? 4u : 0u) | (ly == COST_TY - 1u ? 8u : 0u) | (k == 0u ? 16u : 0u) |
                         (k == COST_TZ - 1u ? 32u : 0u);
            }
        }
        if (faces) atomicOr(&s_faces, faces);
        __syncthreads();
        const uint32_t f = s_faces;
        if (threadIdx.x == 0u && (f & 1u) && tx > 0u) cost_mark(next_flags, next_list, next_count, g.n_tiles, t - 1u);
        if (threadIdx.x == 1u && (f & 2u) && tx + 1u < g.ntx) cost_mark(next_flags, next_list, next_count, g.n_tiles, t + 1u);
        if (threadIdx.x == 2u && (f & 4u) && ty > 0u) cost_mark(next_flags, next_list, next_count, g.n_tiles, t - g.ntx);
        if (threadIdx.x == 3u && (f & 8u) && ty + 1u < g.nty) cost_mark(next_flags, next_list, next_count, g.n_tiles, t + g.ntx);
        if (threadIdx.x == 4u && (f & 16u) && tz > 0u) cost_mark(next_flags, next_list, next_count, g.n_tiles, t - g.ntx * g.nty);
        if (threadIdx.x == 5u && (f & 32u) && tz + 1u < g.ntz) cost_mark(next_flags, next_list, next_count, g.n_tiles, t + g.ntx * g.nty);
        __syncthreads();                                                    // s_key, s_byte, s_faces and s_lowered are the next tile's from here
    }
}

// ---- 3. finish: OPEN -> NONE, and the summary -------------------------------------------------------------------------------------------
// counts[v] += the lanes of `who`, each of which carries the value v: where they all carry the same one, one lane adds them (the
// geodesic pass's finish kernel counts so)
__device__ __forceinline__ void cost_count(uint32_t* counts, uint64_t who, bool mine, uint32_t v, uint32_t lane)
{
    if (!who) return;                                               // (wave-uniform)
    const uint32_t lead = __shfl(v, static_cast<int>(__ffsll(static_cast<unsigned long long>(who))) - 1);
    if (__ballot(mine && v != lead) == 0ull) {
        if (lane == 0u) atomicAdd(&counts[lead], static_cast<uint32_t>(__popcll(who)));
    } else if (mine) {
        atomicAdd(&counts[v], 1u);
    }
}

// One wave per row of the map (n_rows rows of w words).  The maximum as one 64-bit key (1 + cost) << 32 | ~index: the largest cost,
// and among equals the smallest box-linear index, the first in (z, y, x).  A workgroup walks fewer than 2^32 texels: u32 in LDS.
__global__ __launch_bounds__(256) void volym_cost_finish_kernel(uint32_t w, uint32_t n_rows, uint32_t hist_shift, uint32_t* __restrict__ keys, uint32_t* __restrict__ state,
                                                                unsigned long long* __restrict__ summary)
{
    __shared__ uint32_t s_cell[256], s_cell_medium[256], s_hist[256];
    __shared__ unsigned long long s_reached, s_max;
    s_cell[threadIdx.x] = s_cell_medium[threadIdx.x] = s_hist[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) { s_reached = 0ull; s_max = 0ull; }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long wave_reached = 0ull, best = 0ull;
    for (uint32_t row = box_wave_index(); row < n_rows; row += gridDim.x * 4u) {
        const uint32_t base = row * w;
        for (uint32_t x0 = 0u; x0 < w; x0 += 64u) {
            const uint32_t xi = x0 + lane;
            const bool in = xi < w;
            const uint32_t key = in ? keys[base + xi] : COST_NONE;
            if (key == COST_OPEN) keys[base + xi] = COST_NONE;
            const bool reached = key < COST_OPEN;
            const uint32_t cost = key >> 8, label = key & 0xffu;
            const bool grown = reached && cost != 0u;                   // reached and no seed: every step costs at least 1
            const uint64_t r = __ballot(reached);
            cost_count(s_cell, r, reached, label, lane);
            cost_count(s_cell_medium, __ballot(grown), grown, label, lane);
            cost_count(s_hist, r, reached, min(cost >> hist_shift, 255u), lane);
            wave_reached += static_cast<uint32_t>(__popcll(r));
            if (reached) {
                // (1 + cost, so that a reached seed's key is not 0, the key of "none")
                const unsigned long long k = (static_cast<unsigned long long>(cost + 1u) << 32) | (~(base + xi));
                best = k > best ? k : best;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0u && wave_reached) { atomicAdd(&s_reached, wave_reached); atomicMax(&s_max, best); }
    __syncthreads();
    // only the entries this workgroup touched go to memory
    if (s_cell[threadIdx.x]) atomicAdd(&summary[CS_CELL + threadIdx.x], static_cast<unsigned long long>(s_cell[threadIdx.x]));
    if (s_cell_medium[threadIdx.x]) atomicAdd(&summary[CS_CELL_MEDIUM + threadIdx.x], static_cast<unsigned long long>(s_cell_medium[threadIdx.x]));
    if (s_hist[threadIdx.x]) atomicAdd(&summary[CS_HIST + threadIdx.x], static_cast<unsigned long long>(s_hist[threadIdx.x]));
    if (threadIdx.x == 0u && s_reached) {
        atomicAdd(&summary[CS_N_REACHED], s_reached);
        atomicMax(reinterpret_cast<unsigned long long*>(state + CT_MAX_KEY), s_max);
    }
}

// the key of the maximum into the summary's max_cost and max_at (volume coordinates).  One thread.
__global__ __launch_bounds__(64) void volym_cost_pack_kernel(BoxWalkArgs a, const uint32_t* __restrict__ state, unsigned long long* __restrict__ summary)
{
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const unsigned long long k = *reinterpret_cast<const unsigned long long*>(state + CT_MAX_KEY);
    if (k == 0ull) return;                                              // nothing reached: NONE and {0, 0, 0}, as the zero kernel left them
    const uint32_t cost = static_cast<uint32_t>(k >> 32) - 1u, index = ~static_cast<uint32_t>(k);
    const uint32_t x = a.lo[0] + index % a.w, y = a.lo[1] + (index / a.w) % a.h, z = a.lo[2] + index / (a.w * a.h);
    summary[CS_MAX] = static_cast<unsigned long long>(cost) | (static_cast<unsigned long long>(x) << 32);
    summary[CS_MAX + 1] = static_cast<unsigned long long>(y) | (static_cast<unsigned long long>(z) << 32);
}

}  // namespace volym
