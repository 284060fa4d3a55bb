// The walk the box passes share (surface_kernels.h, components_kernels.h, distance_kernels.h): a ROW of a request's box (fixed y, z;
// x ascending) belongs to one wave, which walks it in chunks of 64 consecutive x through layout_offset with byte loads, so odd row
// lengths and box offsets need no keep mask.  A texel is PRESENT when its density byte is at least min_byte, and SOLID when it is
// present and its label is selected in the request's 256-byte table.  Here: the arguments of such a walk and how the host fills them,
// the table as a kernel takes it, the row a wave starts on, and the texel predicate.  What a pass does along its rows is its own.
#pragma once

#include "context.hpp"

namespace volym {

// the request's select table, passed by value; a kernel copies it into LDS before it walks
struct BoxSelect { uint8_t v[256]; };

struct BoxWalkArgs {
    const uint8_t* vol;
    const uint8_t* labels;              // LABELS only (NULL: every label is 0)
    uint32_t lo[3], hi[3];              // the request's box, not empty
    uint32_t nx, ny, nz, bricked, min_byte;
    uint32_t n_rows;                    // h * (hi[2] - lo[2]) <= 4096^2
    uint32_t w, h;                      // hi[0] - lo[0], hi[1] - lo[1]; behind n_rows, so that a kernel that reads neither fetches its
                                        // arguments as it would without them
};

// the arguments of the walk over `box` (checked, not empty) of the context's volume, density read from `vol`
inline BoxWalkArgs box_walk_args(const volym_ctx* c, const uint32_t box[6], uint32_t min_byte, const uint8_t* vol, bool labels)
{
    BoxWalkArgs a = {};
    a.vol = vol;
    a.labels = labels ? c->d_labels : nullptr;
    for (int i = 0; i < 3; ++i) { a.lo[i] = box[i]; a.hi[i] = box[3 + i]; }
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    a.bricked = c->bricked ? 1u : 0u;
    a.min_byte = min_byte;
    a.w = a.hi[0] - a.lo[0]; a.h = a.hi[1] - a.lo[1];
    a.n_rows = a.h * (a.hi[2] - a.lo[2]);                          // (at most 4096^2 = 2^24)
    return a;
}

// the first row of the wave (walk_grid: four waves per workgroup), in a scalar register; the next is gridDim.x * 4 further
__device__ __forceinline__ uint32_t box_wave_index()
{
    return __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
}

// The texel predicate, in two steps so that a caller pays for what it uses and no more.  The texel at layout offset o is present;
// `label` is its label, loaded only where it is present and only under LABELS (else the constant 0: no labels held).
template <bool LABELS>
__device__ __forceinline__ bool box_present(const BoxWalkArgs& a, uint32_t o, uint32_t& label)
{
    label = 0u;
    if (a.vol[o] < a.min_byte) return false;
    if (LABELS) label = a.labels[o];
    return true;
}

// ... and solid: present, and its label selected in the table (s_select: the kernel's copy in LDS)
__device__ __forceinline__ bool box_selected(const uint8_t* s_select, uint32_t label) { return s_select[label] != 0u; }

template <bool LABELS>
__device__ __forceinline__ bool box_solid(const BoxWalkArgs& a, const uint8_t* s_select, uint32_t o, uint32_t& label)
{
    return box_present<LABELS>(a, o, label) && box_selected(s_select, label);
}

}  // namespace volym
