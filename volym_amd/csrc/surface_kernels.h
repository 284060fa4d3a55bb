// The kernels of the surface pass (volym_surface_pass, volym_surface_faces_pass): the boundary faces of the solid texels of a
// request, counted per label and direction with their divergence moments, and written out as one list in canonical order.
// Included by surface.hip alone.
//
// The walk both passes share is the row walk of box_walk.h: lane i of chunk c stands on x = lo_x + 64 * c + i, a run of one texel
// per step, so that the wave's loads are 64 consecutive bytes of a linear row (16 whole x-runs of a bricked one).  The solidity of
// the chunk is one 64-bit ballot S.  The x neighbours need no load: they are S shifted by one lane, with bit 63 of the chunk
// before and bit 0 of the chunk after, which the wave loads one step ahead and which becomes its own S in the next step (every texel of the row is loaded once as "self").
// The y and z neighbours are loaded only by lanes whose own texel is solid -- air asks nothing -- and only where they lie inside
// the request's box: a neighbour outside the box is not solid by the rule, whatever its bytes, and is never read.  So every load
// is of a texel inside the request's box, which volym_surface_check puts inside the volume.
//   The six face ballots F[d] = S & ~neighbour[d] hold everything: popcounts give the row's count, popcounts under the mask of
// the lanes below give a lane's place in the row.  No atomic and no shuffle decides a position, and the order is (x, dir) within
// the row whatever the layout: rows are numbered y first, then z, so the list is ascending in (z, y, x, dir).
//   Rows are addressed through layout_offset: no 16-byte loads, so a row that starts or ends inside a 16-byte chunk (37-texel rows;
// a box from x = 5) needs no keep mask -- the trap of measure_own_run does not exist in this form.
#pragma once

#include "box_walk.h"

namespace volym {

using SurfaceArgs = BoxWalkArgs;

// the summary in device memory: struct volym_surface_summary, as the arrays the kernels index
struct SurfaceOut {
    unsigned long long* faces;          // [256][6]
    unsigned long long* total;
    unsigned long long* pos;            // [256][3]
    unsigned long long* neg;            // [256][3]
};

// Widths.  The host launches at least ceil(n_rows / (4 * WALK_ROWS_PER_WAVE)) workgroups of four waves (walk_grid), so a wave
// walks at most 4096 rows of at most 4096 texels, a lane at most 64 texels of each: 2^18 texels.
//   lane, u32:       faces of one direction <= 2^18; a moment <= 2^18 * 4096 = 2^30.
//   workgroup, LDS:  256 lanes: faces of one (label, direction) <= 2^26, u32; a moment <= 2^38: 64-bit.
//   wave, u64:       the wave's faces (6 * 2^24 at most) are summed in a 64-bit scalar.
//   row, u32:        at most 6 * 4096 faces.
//   global:          everything 64-bit; the row offsets are 32-bit, and volym_surface_faces_pass refuses a total beyond them.
static_assert(WALK_ROWS_PER_WAVE == 4096u, "the widths above");

__global__ __launch_bounds__(256) void volym_surface_init_kernel(unsigned long long* summary, uint32_t n_words)
{
    for (uint32_t i = threadIdx.x; i < n_words; i += 256u) summary[i] = 0ull;
}

// One row, chunk by chunk: step(x, label, S, F) is called once per chunk by all 64 lanes with the lane's own x and label (label
// valid where the lane's bit of S is set) and the wave-uniform ballots.
template <bool LABELS, class Step>
__device__ __forceinline__ void surface_walk_row(const SurfaceArgs& a, const uint8_t* s_select, uint32_t bx, uint32_t bxy, uint32_t row, uint32_t lane,
                                                 Step&& step)
{
    const uint32_t ry = a.hi[1] - a.lo[1];
    const uint32_t y = a.lo[1] + row % ry, z = a.lo[2] + row / ry;
    const bool ym = y > a.lo[1], yp = y + 1u < a.hi[1], zm = z > a.lo[2], zp = z + 1u < a.hi[2];
    uint32_t label_next = 0u;
    uint32_t x = a.lo[0] + lane;
    uint64_t s_next = __ballot(x < a.hi[0] && box_solid<LABELS>(a, s_select, layout_offset(a.bricked != 0u, bx, bxy, x, y, z), label_next));
    uint64_t before = 0ull;                                        // bit 0: the last texel of the chunk before is solid
    for (uint32_t x0 = a.lo[0]; x0 < a.hi[0]; x0 += 64u, x += 64u) {
        const uint64_t s = s_next;
        const uint32_t label = label_next;
        s_next = __ballot(x + 64u < a.hi[0] && box_solid<LABELS>(a, s_select, layout_offset(a.bricked != 0u, bx, bxy, x + 64u, y, z), label_next));
        const bool self = (s >> lane) & 1ull;                      // (a lane beyond the row's end is not solid)
        // the four y and z neighbours together: their density bytes in one round of loads, then their label bytes in one, not eight
        // dependent loads one after the other (the walk waits for memory, not for arithmetic)
        const uint32_t ny_[4] = {y - 1u, y + 1u, y, y}, nz_[4] = {z, z, z - 1u, z + 1u};
        const bool in[4] = {self && ym, self && yp, self && zm, self && zp};
        uint32_t off[4], dense[4], lab[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) off[k] = in[k] ? layout_offset(a.bricked != 0u, bx, bxy, x, ny_[k], nz_[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) dense[k] = in[k] && a.vol[off[k]] >= a.min_byte;
#pragma unroll
        for (int k = 0; k < 4; ++k) lab[k] = (LABELS && dense[k]) ? a.labels[off[k]] : 0u;
        uint64_t f[6];
        f[0] = s & ~((s << 1) | before);
        f[1] = s & ~((s >> 1) | (s_next << 63));
#pragma unroll
        for (int k = 0; k < 4; ++k) f[2 + k] = s & ~__ballot(dense[k] && s_select[lab[k]] != 0u);
        before = s >> 63;
        step(x, y, z, label, s, f);
    }
}

// The count pass: rows[row] = faces of the row; the per-label face counts and moments through LDS into the summary, as
// volym_measure_kernel accumulates: a lane carries one run of equal labels and flushes it when the label changes and at the end.
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_surface_count_kernel(SurfaceArgs a, BoxSelect select, SurfaceOut out, uint32_t* __restrict__ rows)
{
    __shared__ uint32_t s_faces[256 * 6];                          // (widths: see above)
    __shared__ unsigned long long s_pos[256 * 3], s_neg[256 * 3], s_total;
    __shared__ uint8_t s_select[256];
    {
        const uint32_t l = threadIdx.x;
        for (int d = 0; d < 6; ++d) s_faces[l * 6 + d] = 0u;
        for (int i = 0; i < 3; ++i) s_pos[l * 3 + i] = s_neg[l * 3 + i] = 0ull;
        s_select[l] = select.v[l];
        if (l == 0u) s_total = 0ull;
    }
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;

    uint32_t cur = 256u, cf[6] = {0, 0, 0, 0, 0, 0}, cp[3] = {0, 0, 0}, cn[3] = {0, 0, 0};      // the run of equal labels (256: none yet)
    auto flush = [&]() {
        if (cur > 255u) return;
#pragma unroll
        for (int d = 0; d < 6; ++d) if (cf[d]) atomicAdd(&s_faces[cur * 6 + d], cf[d]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (cp[i]) atomicAdd(&s_pos[cur * 3 + i], static_cast<unsigned long long>(cp[i]));
            if (cn[i]) atomicAdd(&s_neg[cur * 3 + i], static_cast<unsigned long long>(cn[i]));
        }
    };
    unsigned long long wave_total = 0ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        uint32_t row_total = 0u;
        surface_walk_row<LABELS>(a, s_select, bx, bxy, row, lane, [&](uint32_t x, uint32_t y, uint32_t z, uint32_t label, uint64_t s, const uint64_t (&f)[6]) {
#pragma unroll
            for (int d = 0; d < 6; ++d) row_total += static_cast<uint32_t>(__popcll(f[d]));
            if (!((s >> lane) & 1ull)) return;
            if (label != cur) {
                flush();
                cur = label;
#pragma unroll
                for (int d = 0; d < 6; ++d) cf[d] = 0u;
#pragma unroll
                for (int i = 0; i < 3; ++i) cp[i] = cn[i] = 0u;
            }
            const uint32_t t[3] = {x, y, z};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t minus = static_cast<uint32_t>((f[2 * i] >> lane) & 1ull), plus = static_cast<uint32_t>((f[2 * i + 1] >> lane) & 1ull);
                cf[2 * i] += minus; cf[2 * i + 1] += plus;
                cn[i] += minus * t[i]; cp[i] += plus * (t[i] + 1u);
            }
        });
        if (lane == 0u) rows[row] = row_total;
        wave_total += row_total;
    }
    flush();
    if (lane == 0u && wave_total) atomicAdd(&s_total, wave_total);
    __syncthreads();
    const uint32_t l = threadIdx.x;
    for (int d = 0; d < 6; ++d) {
        const uint32_t v = s_faces[l * 6 + d];
        if (v) atomicAdd(&out.faces[l * 6 + d], static_cast<unsigned long long>(v));
    }
    for (int i = 0; i < 3; ++i) {
        if (s_pos[l * 3 + i]) atomicAdd(&out.pos[l * 3 + i], s_pos[l * 3 + i]);
        if (s_neg[l * 3 + i]) atomicAdd(&out.neg[l * 3 + i], s_neg[l * 3 + i]);
    }
    if (l == 0u && s_total) atomicAdd(out.total, s_total);
}

// The emit pass: the same walk; rows[row] is now the offset of the row's first face.  A face record is 8 bytes, stored whole:
// x | y << 16, z | dir << 16 | label << 24.
template <bool LABELS>
__global__ __launch_bounds__(256) void volym_surface_emit_kernel(SurfaceArgs a, BoxSelect select, const uint32_t* __restrict__ rows, uint2* __restrict__ faces)
{
    __shared__ uint8_t s_select[256];
    s_select[threadIdx.x] = select.v[threadIdx.x];
    __syncthreads();
    const uint32_t bx = layout_bx(a.bricked != 0u, a.nx), bxy = layout_bxy(a.bricked != 0u, a.nx, a.ny);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t row = box_wave_index(); row < a.n_rows; row += gridDim.x * 4u) {
        uint32_t at = rows[row];                                   // wave-uniform: where the chunk's first face goes
        surface_walk_row<LABELS>(a, s_select, bx, bxy, row, lane, [&](uint32_t x, uint32_t y, uint32_t z, uint32_t label, uint64_t s, const uint64_t (&f)[6]) {
            uint32_t mine = at;
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                mine += static_cast<uint32_t>(__popcll(f[d] & below));
                at += static_cast<uint32_t>(__popcll(f[d]));
            }
            if (!((s >> lane) & 1ull)) return;
            const uint32_t w0 = x | (y << 16), w1 = z | (label << 24);
#pragma unroll
            for (uint32_t d = 0; d < 6u; ++d)
                if ((f[d] >> lane) & 1ull) faces[mine++] = make_uint2(w0, w1 | (d << 16));
        });
    }
}

}  // namespace volym
