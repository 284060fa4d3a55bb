// Internal: what the label edits share on the host -- relabel.hip (volym_edit_labels, the history, undo and redo), brush.hip, lasso.hip,
// smooth.hip, nearest.hip (the fill) and geodesic.hip (the flood).  The edit's transition as named pieces (begin_edit, edit_slab, DeviceResult, launch_label_swap, finish_edit), the
// transition of an edit in one kernel built from them (edit_labels, with the kernel as a parameter), and the three things every launch
// site needs: edit_density, launch_edit and CallArray.  The pieces that are plain functions are defined once, in relabel.hip.  All of it
// is blocking set-up path, like the other edits of the scene's bytes (scene_bytes.hip), whose seam (scene_bytes.hpp) it is built on.
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "scene_bytes.hpp"
#include "edit_chunks.h"

namespace volym {

constexpr uint64_t JOURNAL_RECORD_BYTES = 20u;          // a chunk index and 16 bytes

// What the edit's transition needs to know of a request, whichever kernel carries it out: the box its kernel walks and keeps to, the
// table, DRY_RUN, the name errors carry, and the labels that may receive texels (begin_edit's receives[256]; NULL: those the table
// moves texels to -- an edit whose new label does not come from the table, the fill or the flood, names its own).
struct LabelEdit { const uint32_t* box; const uint8_t* to; bool dry; const char* who; const uint8_t* receives = nullptr; };

// the working result of an edit, an undo or a redo in device memory: the result, then the journal's counter
struct DeviceRelabelResult { volym_relabel_result result; uint32_t records, pad; };

// ---- the transition's pieces (relabel.hip) -----------------------------------------------------------------------------------------
// what volym_edit_labels refuses of the context's state, in the name of `who`
int editable_state(volym_ctx* c, const char* who);
// Begin: the slots at rest, and the uncut copies where receives[l] != 0 for a hidden label l or the mask is active.  A hidden label
// with voxels has made the copies already; one without has not (retarget takes the idle path for it), and texels may be about to
// move into it.  The bytes are still uncut then (the precondition of ensure_uncropped_copies), and the copies go in stream order in
// front of the edit's kernel and the rewrites.
int begin_edit(volym_ctx* c, const uint8_t receives[256]);
// the edit's slab: the walk over the request's box with keep = inside that box, whatever the crop box and the plane are (the cuts
// are in the bytes the window reads); returns its items
uint64_t edit_slab(const volym_ctx* c, const uint32_t box[6], CropSlab& s);
// room for `capacity` records in the journal's staging area
int reserve_journal(volym_ctx* c, hipStream_t stream, uint64_t capacity);
// volym_label_swap_kernel over the records (index, old) into `out`, on `stream`; the launch's error
hipError_t launch_label_swap(const volym_ctx* c, hipStream_t stream, const uint32_t* index, uint4* old, uint64_t records, const RelabelOut& out);
// the journal of the edit that has just stored becomes the newest step of the history (relabel.hip says when it is given up instead)
void record_step(volym_ctx* c, const volym_relabel_result& res, uint64_t records, uint64_t capacity);
// Finish: `res` as the device left it (hi INCLUSIVE) becomes the call's result -- a zero box with nothing changed, else hi exclusive --
// and, unless `dry`, the step is recorded (journalled) and follow_labels runs.  A failure from here on leaves bytes that belong to
// neither state: the context then asks for volym_set_volume again, as after a failed retarget.
int finish_edit(volym_ctx* c, volym_relabel_result& res, bool dry, bool journalled, uint64_t records, uint64_t capacity, const char* who);

// The device result for the length of one call, in the shape of CallArray: allocated, seeded in stream order in front of each kernel
// that tallies into it, read back behind that kernel, and freed when the scope ends, on every path.
struct DeviceResult {
    DeviceRelabelResult* ptr = nullptr;
    hipStream_t stream = nullptr;

    int alloc(volym_ctx* c, hipStream_t on)               // VOLYM_E_NOMEM "hipMalloc(relabel result): <hip error>"
    {
        stream = on;
        const hipError_t e = hipMalloc(&ptr, sizeof *ptr);
        if (e != hipSuccess) { ptr = nullptr; return ctx_fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(relabel result): ") + hipGetErrorString(e)); }
        return VOLYM_OK;
    }
    // counts 0, lo = max, hi = 0: the kernels keep INCLUSIVE maxima.  Back is DeviceRelabelResult, or volym_relabel_result where no
    // journal is written (undo and redo): the copies are of what the caller reads back
    template <class Back>
    hipError_t seed()
    {
        DeviceRelabelResult init = {};
        for (int a = 0; a < 3; ++a) init.result.box[a] = 0xffffffffu;
        return hipMemcpyAsync(ptr, &init, sizeof(Back), hipMemcpyHostToDevice, stream);
    }
    template <class Back>
    hipError_t fetch(Back& back)                          // to the host behind the work of the stream; waits for it
    {
        const hipError_t e = hipMemcpyAsync(&back, ptr, sizeof back, hipMemcpyDeviceToHost, stream);
        return e == hipSuccess ? hipStreamSynchronize(stream) : e;
    }
    RelabelOut out() const
    {
        volym_relabel_result* const r = &ptr->result;
        return {reinterpret_cast<unsigned long long*>(&r->changed), reinterpret_cast<unsigned long long*>(r->left), reinterpret_cast<unsigned long long*>(r->arrived), r->box};
    }
    // the staging area, counted in `records`
    LabelJournal journal(const volym_ctx* c, uint64_t capacity) const { return {c->journal_index.ptr, c->journal_old.ptr, &ptr->records, static_cast<uint32_t>(capacity)}; }
    DeviceResult() = default;
    DeviceResult(const DeviceResult&) = delete;
    ~DeviceResult() { (void)hipFree(ptr); }
};

// ---- the transition of an edit in one kernel ---------------------------------------------------------------------------------------
// The counterpart of retarget for a change of labels under a (box, plane, mask) that stays.  launch(stream, grid, out, to, slab, items,
// journal) enqueues the request's kernel over the slab of r.box; journal is NULL unless the history is on and the request is no
// DRY_RUN.  With no texel changed (or DRY_RUN) nothing but the result is written.
template <class Launch>
int edit_labels(volym_ctx* c, const LabelEdit& r, volym_relabel_result& res, Launch launch)
{
    const bool journalled = c->history_budget != 0u && !r.dry;
    std::memset(&res, 0, sizeof res);
    for (int a = 0; a < 3; ++a) if (r.box[a] == r.box[3 + a]) return VOLYM_OK;        // an empty box: nothing to walk

    uint8_t receives[256] = {};
    for (int l = 0; l < 256; ++l) if (r.to[l] != l) receives[r.to[l]] = 1u;
    int rc = begin_edit(c, r.receives ? r.receives : receives);
    if (rc != VOLYM_OK) return rc;

    const hipStream_t stream = c->slot0().stream;
    CropSlab s;
    const uint64_t items = edit_slab(c, r.box, s);
    // the staging area holds the slab's worst case, one record per item, or what the budget holds: past that the kernel only counts
    const uint64_t capacity = journalled ? std::min<uint64_t>(items, c->history_budget / JOURNAL_RECORD_BYTES) : 0u;
    if (journalled) rc = reserve_journal(c, stream, capacity);
    if (rc != VOLYM_OK) return rc;
    DeviceRelabelResult back = {};
    {
        DeviceResult d;
        rc = d.alloc(c, stream);
        if (rc != VOLYM_OK) return rc;
        hipError_t e = d.seed<DeviceRelabelResult>();
        if (e == hipSuccess) {
            LabelTable to;
            std::memcpy(to.v, r.to, 256);
            const LabelJournal journal = d.journal(c, capacity);
            launch(stream, dim3(stream_grid(c, items)), d.out(), to, s, static_cast<uint32_t>(items), journalled ? &journal : nullptr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = d.fetch(back);
        if (e != hipSuccess) {
            if (!r.dry) c->have_vol = c->have_frame = false;                  // (the kernel may have stored)
            return ctx_fail(c, VOLYM_E_HIP, std::string(r.who) + ": " + hipGetErrorString(e));
        }
    }
    res = back.result;
    return finish_edit(c, res, r.dry, journalled, back.records, capacity, r.who);
}

// the density an edit's window reads: the uncut copy with UNCUT, where there is one (call it after begin_edit: inside launch)
inline const uint4* edit_density(const volym_ctx* c, bool uncut) { return reinterpret_cast<const uint4*>(uncut && c->d_vol0 ? c->d_vol0 : c->d_vol); }

// What edit_labels' launch does with what it is handed, for a pair of kernels (plain, journalling) that differ in the journal argument
// alone: the labels first, then `front` (what the kernel reads beside them), the result, the table, the slab and the rule, the journal
// where there is one, and the volume's shape.
template <class Plain, class Journalling, class Rule, class... Front>
void launch_edit(const volym_ctx* c, Plain plain, Journalling journalling, hipStream_t stream, dim3 grid, const RelabelOut& out, const LabelTable& to,
                 const CropSlab& s, const Rule& rule, uint32_t items, const LabelJournal* journal, Front... front)
{
    uint4* const labels = reinterpret_cast<uint4*>(c->d_labels);
    const uint32_t bricked = c->bricked ? 1u : 0u;
    if (journal) hipLaunchKernelGGL(journalling, grid, dim3(256), 0, stream, labels, front..., out, to, s, rule, *journal, c->nx, c->ny, c->nz, bricked, items);
    else hipLaunchKernelGGL(plain, grid, dim3(256), 0, stream, labels, front..., out, to, s, rule, c->nx, c->ny, c->nz, bricked, items);
}

// A small host array on the device for the length of one call (the brush's segments, the lasso's edges): copied on `stream`, in
// stream order in front of the call's kernels, and freed when the call returns, once the stream is idle (after a refusal the copy or a
// kernel may still run).
template <class T>
struct CallArray {
    T* ptr = nullptr;
    hipStream_t stream = nullptr;

    // VOLYM_E_NOMEM "hipMalloc(<what>): <hip error>", or VOLYM_E_HIP "<who>: <hip error>" for the copy
    int upload(volym_ctx* c, hipStream_t on, const std::vector<T>& host, const char* what, const char* who)
    {
        stream = on;
        hipError_t e = hipMalloc(&ptr, host.size() * sizeof(T));
        if (e != hipSuccess) { ptr = nullptr; return ctx_fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e)); }
        e = hipMemcpyAsync(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? VOLYM_OK : ctx_fail(c, VOLYM_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    CallArray() = default;
    CallArray(const CallArray&) = delete;
    ~CallArray() { if (ptr) { (void)hipStreamSynchronize(stream); (void)hipFree(ptr); } }
};

}  // namespace volym
