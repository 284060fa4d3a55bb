// The outline pass (gfx950): ring and tint of the selected segments, from pick records, in screen space.  A unit of its own, as
// pick.hip and scene_bytes.hip are: nothing here is instantiated in, or changes, the units of the frame, pick or scene kernels.
// It holds the pass's kernels (outline_kernels.h), its C ABI (volym_outline_pass, volym_read_outline, volym_outline_device_ptr)
// and what the context keeps for it: the bit plane, its own target and two events.
#include <hip/hip_runtime.h>

#include <cstring>

#include "context.hpp"
#include "outline_kernels.h"

static_assert(sizeof(volym_outline) == 268, "volym_outline is 268 bytes");
static_assert(sizeof(volym_pick_record) == 2 * sizeof(uint2), "the pack kernel reads the second 8-byte half of a 16-byte record");
static_assert(offsetof(volym_pick_record, label) == 10 && offsetof(volym_pick_record, status) == 12, "label and status sit in bytes 8..15");

namespace volym {

// first use (a set-up step, blocking): the bit plane with its guards zeroed, and the events that order the pass between frame slots
static int ensure_outline_resources(volym_ctx* c)
{
    if (c->outline_plane.ptr) return VOLYM_OK;
    const uint32_t stride = (c->W + 63u) / 64u + 2u;
    const size_t words = static_cast<size_t>(stride) * (c->H + 2u * OUTLINE_GUARD_ROWS);
    for (hipEvent_t& ev : c->outline_ev)
        if (!ev) VOLYM_HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const int rc = c->outline_plane.reserve(c, c->slot0().stream, words, "outline plane");
    if (rc != VOLYM_OK) return rc;
    // on the stream the passes go on: a hipMemset on the null stream is not ordered with a non-blocking stream, and may return
    // before the device has zeroed the plane
    const hipError_t e = hipMemsetAsync(c->outline_plane.ptr, 0, words * sizeof(uint64_t), c->slot0().stream);
    if (e != hipSuccess) { c->outline_plane.release(); return ctx_fail(c, VOLYM_E_HIP, std::string("hipMemsetAsync(outline plane): ") + hipGetErrorString(e)); }
    c->outline_stride = stride;
    return VOLYM_OK;
}

void free_outline(volym_ctx* c)
{
    c->outline_plane.release();
    c->outline.release();
    for (hipEvent_t& ev : c->outline_ev) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
}

}  // namespace volym

using namespace volym;

extern "C" {

int volym_outline_pass(volym_ctx* c, const volym_outline* o, const void* records_device, const uint32_t rect[4], void* target_rgba8)
{
    if (!c) return VOLYM_E_INVALID;
    if (!o) return ctx_fail(c, VOLYM_E_INVALID, "volym_outline_pass: NULL volym_outline");
    if (o->radius < 1u || o->radius > OUTLINE_GUARD_ROWS) return ctx_fail(c, VOLYM_E_INVALID, "volym_outline_pass: radius must be 1..8");
    if ((records_device == nullptr) != (rect == nullptr))
        return ctx_fail(c, VOLYM_E_INVALID, "volym_outline_pass: records and rect go together (both NULL: those of the latest volym_pick_pass)");
    uint32_t r[4] = {c->pick_x0, c->pick_y0, c->pick_w, c->pick_h};      // (those of the latest pick pass, checked by it)
    if (rect) { const int rc = frame_rect(c, rect, "volym_outline_pass", r); if (rc != VOLYM_OK) return rc; }
    if (c->world != 1u) return ctx_fail(c, VOLYM_E_STATE, "volym_outline_pass: not on a sharded context (its frame buffer holds a picture only on the root, after assembly)");
    if (!c->frame_rendered) return ctx_fail(c, VOLYM_E_STATE, "volym_outline_pass: no volym_compute_pass yet");
    if (!records_device && c->picks.count == 0u) return ctx_fail(c, VOLYM_E_STATE, "volym_outline_pass: no volym_pick_pass yet");
    VOLYM_HIPCHK(c, hipSetDevice(c->device));
    FrameSlot& s0 = c->slot0();                    // the pass runs where the pick passes run: ordered with them and with itself
    FrameSlot& sf = *c->slots[c->last];            // the slot of the frame it reads
    int rc = ensure_outline_resources(c);
    if (rc != VOLYM_OK) return rc;
    uint32_t* dst = static_cast<uint32_t*>(target_rgba8);
    if (!dst) {
        // our own target, allocated on first use (a set-up step: the one blocking path of the call)
        rc = c->outline.reserve(c, s0.stream, static_cast<size_t>(c->W) * c->H, "outline target");
        if (rc != VOLYM_OK) return rc;
        dst = c->outline.ptr;
    }

    OutlineArgs a;
    a.tails = static_cast<const uint2*>(records_device ? records_device : static_cast<const void*>(c->picks.ptr));
    a.plane = c->outline_plane.ptr;
    a.src = c->frame_buf(sf);
    a.dst = dst;
    std::memset(a.sel, 0, sizeof a.sel);
    for (uint32_t l = 0; l < 256u; ++l)
        if (o->selected[l]) a.sel[l >> 6] |= 1ull << (l & 63u);
    a.W = c->W; a.H = c->H; a.stride = c->outline_stride;
    a.x0 = r[0]; a.y0 = r[1]; a.w = r[2]; a.h = r[3];
    a.ring = pack_rgba(o->ring_rgba);
    a.fill = pack_rgba(o->fill_rgba);

    // Two frames in flight: the frame may have been marched on the other slot's stream.  The pass starts behind it, and that stream
    // goes on only when the pass has ended (its next march rewrites the frame the pass reads; with a bound frame buffer either
    // slot's does).  Events, no host wait.
    const bool cross = c->slots[1] && (c->last == 1 || c->bound_frame);
    FrameSlot& other = *c->slots[c->slots[1] ? 1 : 0];
    if (cross) {
        VOLYM_HIPCHK(c, hipEventRecord(c->outline_ev[0], other.stream));
        VOLYM_HIPCHK(c, hipStreamWaitEvent(s0.stream, c->outline_ev[0], 0));
    }
    const uint32_t words = (c->W + 63u) / 64u;
    hipLaunchKernelGGL(volym_outline_pack_kernel, dim3(words, (c->H + 4u * OUTLINE_PACK_ROWS - 1u) / (4u * OUTLINE_PACK_ROWS)), dim3(64, 4), 0, s0.stream, a);
    VOLYM_HIPCHK(c, hipGetLastError());
    const dim3 grid(words, (c->H + 4u * OUTLINE_STRIP_ROWS - 1u) / (4u * OUTLINE_STRIP_ROWS));
    hipLaunchKernelGGL(volym_outline_blend_kernel, grid, dim3(64, 4), 0, s0.stream, a, o->radius);
    VOLYM_HIPCHK(c, hipGetLastError());
    if (cross) {
        VOLYM_HIPCHK(c, hipEventRecord(c->outline_ev[1], s0.stream));
        VOLYM_HIPCHK(c, hipStreamWaitEvent(other.stream, c->outline_ev[1], 0));
    }
    if (!target_rgba8) c->outline.count = static_cast<size_t>(c->W) * c->H;
    return VOLYM_OK;
}

int volym_read_outline(volym_ctx* c, uint8_t* out)
{
    if (!c) return VOLYM_E_INVALID;
    if (!out) return ctx_fail(c, VOLYM_E_INVALID, "volym_read_outline: NULL output");
    if (c->outline.count == 0u) return ctx_fail(c, VOLYM_E_STATE, "volym_read_outline: no volym_outline_pass into the context's own target yet");
    return c->outline.read(c, c->slot0().stream, out, c->outline.count);
}

void* volym_outline_device_ptr(volym_ctx* c) { return (c && c->outline.count != 0u) ? c->outline.ptr : nullptr; }

}  // extern "C"
