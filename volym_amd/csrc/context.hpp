// Internal: the context behind include/volym_hip.h (one device, one W x H output, one or two frame slots) and the pieces of host
// logic that more than one translation unit needs.  The units, each with the C ABI of what it holds:
//   raymarch.hip      the frame loop, the cost-feedback thread and the capture that feeds it; mgpu.inc, the native multi-GPU loop,
//                     is included in it
//   scene_bytes.hip   the bytes of the scene; the seam in front of it for the two groups below is scene_bytes.hpp
//   pick.hip, outline.hip, slice.hip, project.hip, measure.hip, surface.hip, components.hip, distance.hip
//                     the pass of that name
//   nearest.hip       the nearest pass and the fill by it, an edit like those below
//   geodesic.hip      the geodesic pass and the flood by it, an edit like those below
//   cost.hip          the cost pass; the spread by it is the flood's kernel, launched by geodesic.hip's flood_by_map
//   interpolate.hip   the interpolate pass (fill between slices) and the edit by it, an edit like those below
//   relabel.hip, brush.hip, lasso.hip, smooth.hip
//                     the label edit of that name (relabel.hip: and the history); what they share on the host is label_edit.hpp
//   box_pass.hip      no ABI: what the passes over a request's box share -- the scan of row counts into offsets and the read-back
//                     of a box-linear volume
// The work-list scheduler that the feedback thread runs is worklist.hpp / worklist.cpp: host only, it knows nothing of this header.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/volym_hip.h"
#include "raymarch_device.h"
#include "worklist.hpp"

namespace volym {

int ctx_fail(volym_ctx* c, int code, const std::string& msg);

// A device buffer of the context's own: what a pass writes when the caller passes no target.  It grows to the largest size asked
// for and never shrinks; growing is the one blocking step of a pass.  Freed by hand (release), with the device set and the streams
// idle: volym_destroy's order says when.  The members are defined below volym_ctx.
template <class T>
struct OwnedBuffer {
    T* ptr = nullptr;
    size_t capacity = 0;                     // elements ptr holds
    size_t count = 0;                        // elements the latest pass into it wrote (0: none yet); the pass sets it, growth clears it

    // room for `need` elements.  Nothing when there is; else `stream` (where the earlier passes into it ran) is synchronised and the
    // buffer replaced.  On failure it is left empty: VOLYM_E_NOMEM, "hipMalloc(<what>): <hip error>"
    int reserve(volym_ctx* c, hipStream_t stream, size_t need, const char* what);
    // the first n elements to host memory, blocking (read_back)
    int read(volym_ctx* c, hipStream_t stream, void* out, size_t n) const;
    void release() { (void)hipFree(ptr); ptr = nullptr; capacity = count = 0; }
};

// One count per row of a request's box, which scan_row_offsets turns in place into the offset of the row's first item, and the block
// sums of that scan: one per VOLYM_SURFACE_SCAN_ROWS rows.  The two are replaced together.
struct RowOffsets {
    OwnedBuffer<uint32_t> rows, sums;

    // room for n_rows rows.  Nothing when there is; else both are replaced as OwnedBuffer::reserve replaces one, and should either
    // allocation fail neither is kept
    int reserve(volym_ctx* c, hipStream_t stream, size_t n_rows, const char* what);
    void release() { rows.release(); sums.release(); }
};

// What a capture hands the feedback thread: written by the caller before FB_CAPTURED, by the worker before FB_READY.
struct FbJob {
    int list = 0;                            // which of lists[] the captured launch ran
    uint32_t n_entries = 0;
    CapturedLaunch launch;                   // the facts of that launch the scheduler reads
    ListSettings set;                        // the context's settings at the capture
    double t_us[6] = {};                     // dev: wall-clock stamps of the job's stages
    std::string error;                       // worker -> caller
};

// One frame in flight: everything a launch writes or rewrites in stream order, and the work lists and cost feedback that
// schedule its launches.  A context has one (slot 0) or, with VOLYM_OPT_FRAMES_IN_FLIGHT = 2, two; the scene they march is
// the context's (raymarch.hip "frames in flight").
struct FrameSlot {
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    hipStream_t copy_stream = nullptr;      // cost read-backs and work-list uploads of the feedback thread

    // per-(transfer function, step) tables: one device copy, refreshed in stream order from a ring of pinned stagings
    static constexpr int TABLE_RING = 8;
    FrameTables* d_tables = nullptr;
    FrameTables* h_tables[TABLE_RING] = {};
    hipEvent_t tables_ev[TABLE_RING] = {};
    int tables_slot = 0;
    FrameTables tables_now;                  // what d_tables holds (or will, in stream order)
    bool tables_dirty = true;
    float tables_alpha_y = -1.0f;

    uint8_t* d_df = nullptr;                 // packed 4-bit distance field for (d_mc, thr_byte)
    uint32_t df_thr_byte = 0xffffffffu;
    uint32_t thr_byte_cull = 256;
    bool hull_dirty = true;
    uint32_t* d_tile_mask = nullptr;         // one bit per 8x8 pixel tile: some occupied macro cell projects onto it (per view); two
                                             // buffers of tile_mask_words: the one in use and the one being kept zeroed for the next view
    int mask_cur = 0;
    bool mask_wanted = false;                // compute_culling: this view gets a mask
    bool mask_pending = false;               // ... and has not got it yet
    uint32_t view_launches = 0;              // launches since the view last changed
    float mask_clip[16] = {};                // world -> clip of the view (f32 copy for the mask kernel)
    float mask_margin = 0.0f;
    uint32_t* d_tile_depth = nullptr;        // per 8x8 tile: the depth range of its occupied cells (FrameParams::tile_depth), 64 words per
                                             // mask word; zeroed and rebuilt in stream order with each view's mask
    int* d_aabb = nullptr;                   // written by the distance-field kernel (kept for the dev tools)

    uint32_t* d_shard_own = nullptr;
    uint32_t* d_frame_own = nullptr;
    float4* d_f32 = nullptr;
    OwnedBuffer<uint32_t> blit;              // volym_blit target when the caller passes none
    uint32_t blit_w = 0, blit_h = 0;         // size of the latest blit into it
    OwnedBuffer<uint8_t> gather_tmp;         // volym_assemble_host's device copy of the gathered shards (count unused)
    uint32_t* d_pack_counters = nullptr;
    uint32_t pack_parity = 0;
    Counters* d_counters = nullptr;
    uint4* d_trace = nullptr;

    // ---- work lists + cost feedback (variant 2) ----
    uint32_t* d_list[2] = {nullptr, nullptr};   // device lists: `cur` is launched from, the other is the feedback thread's
    uint32_t* h_list_pinned = nullptr;          // staging of the list the feedback thread uploads
    uint16_t* d_cost = nullptr;                 // position-indexed costs of ONE captured launch, then (u32) the end time of every
    uint16_t* h_cost_pinned = nullptr;          // wave and the start time of every workgroup of that launch (raymarch_pq.h)
    size_t list_capacity = 0;                   // entries each of the above can hold
    int cur = 0;
    WorkList lists[2];
    std::vector<uint16_t> item_cost;            // last measured / estimated cost per 8x8 item (4 * n_local), carried across views
    std::vector<uint8_t> item_is_dp;            // hysteresis of the depth-parallel split
    std::atomic<uint64_t> view_serial{1};       // bumped by every volym_update that changes the uniforms (read by the feedback thread)
    // ---- variant 3 (ray pool): {-, -, error bits of the frames so far}
    uint32_t* d_pool_sync = nullptr;
    bool pool_launched = false;
    uint32_t* d_pool_dbg = nullptr;             // development timeline of variant 3 (volym_dev_pool_timeline)
    bool pool_dbg = false;

    enum : int { FB_IDLE = 0, FB_CAPTURED = 1, FB_READY = 2, FB_QUIT = 3 };
    std::thread fb_thread;
    std::mutex fb_mu;
    std::condition_variable fb_cv;
    std::atomic<int> fb_state{FB_IDLE};
    hipEvent_t ev_march = nullptr, ev_cost = nullptr, ev_list = nullptr;
    FbJob fb_job;

    FrameParams fp;
};

}  // namespace volym

// The scene and the settings: what the set-up calls write and every frame slot only reads.
struct volym_ctx {
    int device = 0;
    uint32_t W = 0, H = 0, tiles_x = 0, tiles_y = 0, n_tiles = 0;
    uint32_t rank = 0, world = 1, n_local = 0, shard_tiles = 0;
    std::vector<uint32_t> geometric;            // centre-first list of this shard (rebuilt by the setup calls)

    uint8_t* d_vol = nullptr;
    uint8_t* d_imp = nullptr;
    uint32_t nx = 0, ny = 0, nz = 0;
    uint32_t inx = 0, iny = 0, inz = 0;
    int imp_box_lo[3] = {1, 1, 1}, imp_box_hi[3] = {0, 0, 0};   // texel AABB of the importances >= 128 (lo > hi: none)
    uint64_t imp_bytes = 0;                  // size of the d_imp allocation
    // label volume (volym_set_labels): kept in the layout d_imp gets; volym_set_segment_importances maps it into d_imp
    uint8_t* d_labels = nullptr;
    uint32_t lnx = 0, lny = 0, lnz = 0;
    bool labels_bricked = false;
    uint64_t label_count[256] = {};
    int label_box[256][6] = {};              // texel AABB {x0, y0, z0, x1, y1, z1} of every label value (count 0: none)
    // crop box (volym_set_crop_box), texels of the volume; [0, n) after volym_set_volume.  From the first crop on d_vol0 holds the
    // uncropped density and d_vol is "d_vol0 inside the box, 0 elsewhere".  The importances likewise: their uncropped source is
    // the labels through seg_table when a table has been set since the labels, else d_imp0 (NULL: d_imp is uncropped).  They are
    // cropped only while their dimensions are the volume's (volym_update refuses any other).
    uint32_t crop_lo[3] = {0, 0, 0}, crop_hi[3] = {0, 0, 0};
    // clip plane (volym_set_clip_plane): texel (x, y, z) is kept iff clip_n . (x, y, z) <= clip_d; (0, 0, 0), 0 = no plane, the
    // state after volym_set_volume.  A third term of the invariant below, cut from the same uncut sources as the box.
    int32_t clip_n[3] = {0, 0, 0}, clip_d = 0;
    uint8_t* d_vol0 = nullptr;
    uint8_t* d_imp0 = nullptr;
    bool imp_bricked = false;                // layout of d_imp (and d_imp0)
    uint8_t seg_table[256] = {};
    bool have_seg_table = false;
    int imp_box0_lo[3] = {1, 1, 1}, imp_box0_hi[3] = {0, 0, 0};   // imp_box_* of the uncropped importances (of the visible segments)
    // segment visibility (volym_set_segment_visibility): seg_hidden[l] != 0 hides label l; all 0 after volym_set_labels,
    // volym_set_importances and volym_set_volume.  The invariant every edit of box or mask keeps, and relies on to rewrite only
    // the texels whose state changes:  d_vol[t] = (t inside the crop box && t kept by the clip plane && !seg_hidden[label(t)]) ?
    // d_vol0[t] : 0  for every texel t, and the same for d_imp with its uncropped source (above).  An edit that fails after its first launch breaks it,
    // and the context then asks for volym_set_volume again (have_vol false).  While a segment is hidden the labels have the
    // volume's dimensions and layout (the call refuses anything else).  One function keeps it: retarget (scene_bytes.hip), which
    // every set-up call that changes box, plane, mask or bytes goes through.
    uint8_t seg_hidden[256] = {};
    int filter = VOLYM_FILTER_NEAREST;
    uint8_t lut[256 * 4] = {};
    uint32_t tf_n = 0;
    bool have_vol = false, have_imp = false, have_tf = false, have_frame = false;

    uint8_t* d_mc = nullptr;                 // per-macro-cell density maxima
    std::vector<uint8_t> h_mc;               // host copy of d_mc
    int aabb_tab[257][6];                    // occupied-cell AABB per threshold byte {x0,y0,z0,x1,y1,z1}; x1 < x0: none
    uint32_t mc_n = 32;
    // The grid the per-view tile mask and depth bounds are built from (raymarch.hip ensure_frame_resources): maxima of fine_n^3 cells
    // defined as the macro cells are (scene_kernels.h volym_fine_cell_kernel), shared by the frame slots as d_mc is, device only.
    // NULL with fine_n == mc_n: the macro cells themselves.  bounds_cells is VOLYM_OPT_BOUNDS_CELLS: -1 the rule
    // (volym_bounds_cells_for), 0 the macro-cell grid, else an explicit power of two.
    uint8_t* d_mc_fine = nullptr;
    uint32_t fine_n = 32;
    int bounds_cells = -1;
    uint32_t tile_mask_words = 0;            // 0: the frame has more tiles than the mask kernel holds in LDS -- no mask
    bool tile_mask = true;                   // dev switch
    bool tile_depth = true;                  // dev switch: per-tile depth bounds with the mask
    bool mask_eager = false;                 // dev

    // bound by volym_bind_output (NULL: each slot renders into its own)
    uint32_t* bound_shard = nullptr;
    uint32_t* bound_frame = nullptr;

    static constexpr uint32_t THROTTLE_RING = 9;          // one more than the deepest wait volym_throttle accepts (8)
    hipEvent_t throttle_ev[THROTTLE_RING] = {};
    uint32_t throttle_head = 0;

    // ---- the read-only passes: each writes a buffer of the context's own when the caller passes no target, always on slot 0's stream
    // pick passes (volym_pick_pass, pick.hip): the records of the latest pass
    volym::OwnedBuffer<volym_pick_record> picks;
    uint32_t pick_w = 0, pick_h = 0;         // rect size of the latest pass
    uint32_t pick_x0 = 0, pick_y0 = 0;       // ... and its origin in the frame (the outline pass places the records by it)

    // outline passes (volym_outline_pass, outline.hip)
    volym::OwnedBuffer<uint64_t> outline_plane;   // one bit per frame pixel plus zeroed guards (outline_kernels.h), reserved once
    uint32_t outline_stride = 0;             // words per plane row
    volym::OwnedBuffer<uint32_t> outline;    // W x H target, reserved once
    hipEvent_t outline_ev[2] = {};           // frame of the other slot -> pass, pass -> the other slot's next work
    bool frame_rendered = false;             // some volym_compute_pass has been enqueued

    // slice passes (volym_slice_pass, slice.hip)
    volym::OwnedBuffer<uint32_t> slice;
    uint32_t slice_w = 0, slice_h = 0;       // size of the latest pass into it

    // projection passes (volym_project_pass, project.hip): records and image
    volym::OwnedBuffer<volym_projection> projection;
    volym::OwnedBuffer<uint32_t> projection_image;
    uint32_t projection_w = 0, projection_h = 0;                        // rect size of the latest pass into projection
    uint32_t projection_image_w = 0, projection_image_h = 0;            // ... and into projection_image
    volym::OwnedBuffer<volym_projection> projection_at;                 // the one record of volym_project_at, reserved once

    // measure passes (volym_measure_pass, measure.hip): one result, reserved once; count 1: a pass has written it since the latest
    // volym_set_volume
    volym::OwnedBuffer<volym_measurement> measure;

    // surface passes (volym_surface_pass / volym_surface_faces_pass, surface.hip)
    uint64_t scene_serial = 0;               // bumped by every set-up call that changes a byte the surface pass reads (density, labels)
    volym::OwnedBuffer<volym_surface_summary> surface;   // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::RowOffsets surface_offsets;          // per row of the request's box: its face count, scanned in place into the offset of its first face
    uint64_t surface_serial = 0;             // scene_serial at that pass: the offsets describe the scene while it is the current one
    volym_surface surface_request = {};      // what that pass was asked (the emit pass walks it again)
    const uint8_t* surface_vol = nullptr;    // ... and the density it read (d_vol, or d_vol0 under UNCUT)
    bool surface_labels = false;             // ... and whether it read labels
    bool surface_total_known = false;        // surface_total is the pass's total (read back once)
    uint64_t surface_total = 0;
    volym::OwnedBuffer<volym_surface_face> surface_faces;   // the context's own face list; count: the faces of the latest faces pass
    bool surface_faces_valid = false;        // a faces pass has written it since the latest surface pass (a surface may have 0 faces)

    // components passes (volym_components_pass, components.hip): a snapshot, valid until the next volym_set_volume
    volym::OwnedBuffer<volym_components_summary> components;   // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::OwnedBuffer<uint32_t> component_ids;      // the id volume of the request's box, box-linear; the union-find forest while the pass runs
    volym::OwnedBuffer<volym_component> component_table;   // the records: min(max_components, texels of the box) of them at most
    volym::OwnedBuffer<uint32_t> component_work;     // the working table the records accumulate in (components_kernels.h), sized with the table
    volym::RowOffsets component_offsets;        // per row of the request's box: its roots, scanned in place into the number of its first root
    uint32_t component_box[6] = {};          // the box of the latest pass (the reads address the id volume by it)

    // distance passes (volym_distance_pass, distance.hip): a snapshot, valid until the next volym_set_volume
    volym::OwnedBuffer<volym_distance_summary> distance;   // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::OwnedBuffer<uint32_t> distance_map;       // D of every texel of the request's box, box-linear
    volym::OwnedBuffer<uint32_t> distance_work;      // the column sweeps' stacks: two words per texel of the box (distance_kernels.h)
    volym::OwnedBuffer<unsigned long long> distance_keys;   // the working summary: counters and 64-bit (D, index) keys, packed into `distance`
    uint32_t distance_box[6] = {};           // the box of the latest pass (the reads address the map by it)

    // nearest passes (volym_nearest_pass, nearest.hip): a snapshot, valid until the next volym_set_volume
    volym::OwnedBuffer<volym_nearest_summary> nearest;   // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::OwnedBuffer<uint32_t> nearest_sites;      // site of every texel of the request's box, box-linear; the sweeps' g while the pass runs
    volym::OwnedBuffer<uint8_t> nearest_labels;      // ... and the label byte of that site
    volym::OwnedBuffer<uint16_t> nearest_winners;    // wx, wy, wz: the winning entry per texel and axis (nearest_kernels.h), three per texel
    volym::OwnedBuffer<uint32_t> nearest_work;       // the column sweeps' stacks, where the distance pass's work arrays are too small
    uint32_t nearest_box[6] = {};            // the box of the latest pass (the reads and the fill address the maps by it)
    uint32_t nearest_weight[3] = {};         // ... and its weights (the fill's band is in its metric)

    // geodesic passes (volym_geodesic_pass, geodesic.hip): a snapshot, valid until the next volym_set_volume
    volym::OwnedBuffer<volym_geodesic_summary> geodesic;   // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::OwnedBuffer<uint32_t> geodesic_map;       // the key of every texel of the request's box, box-linear; aliases no other pass's result
    volym::OwnedBuffer<uint32_t> geodesic_tiles;     // the relaxation's state: a header, then per tile two round flags and two list entries (geodesic_kernels.h)
    uint32_t geodesic_box[6] = {};           // the box of the latest pass (the reads and the flood address the map by it)
    uint64_t geodesic_rounds = 0;            // the rounds the latest pass enqueued, those past the last active one included

    // cost passes (volym_cost_pass, cost.hip): a snapshot of its own, valid until the next volym_set_volume
    volym::OwnedBuffer<volym_cost_summary> cost;     // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::OwnedBuffer<uint32_t> cost_map;           // the key of every texel of the request's box, box-linear; aliases no other pass's result
    volym::OwnedBuffer<uint8_t> cost_bytes;          // the density byte of every texel of that box as the pass read it, box-linear
    volym::OwnedBuffer<uint32_t> cost_tiles;         // the relaxation's state, laid out as geodesic_tiles is (cost_kernels.h)
    uint32_t cost_box[6] = {};               // the box of the latest pass (the reads and the spread address the map by it)
    uint64_t cost_rounds = 0;                // the rounds the latest pass enqueued, those past the last active one included

    // interpolate passes (volym_interpolate_pass, interpolate.hip): a snapshot of its own, valid until the next volym_set_volume
    volym::OwnedBuffer<volym_interpolate_summary> interpolate;   // one summary, reserved once; count 1: a pass has written it since the latest volym_set_volume
    volym::OwnedBuffer<uint32_t> interpolate_work;   // four words per texel of the request's box: Dout, Din and the two stacks of the column sweeps; the signed
                                                     // map is stored over the first stack (interpolate_kernels.h)
    volym::OwnedBuffer<uint8_t> interpolate_state;   // the state byte of every texel of that box, box-linear
    volym::OwnedBuffer<uint32_t> interpolate_counts; // the SHAPE texels per slice, VOLYM_INTERPOLATE_SLICES words
    uint32_t interpolate_box[6] = {};        // the box of the latest pass (the reads and the edit address the maps by it)
    uint32_t interpolate_texels = 0;         // ... and its texels: the signed map starts at word 2 * interpolate_texels of the work array

    // the history of label edits (volym_label_history, relabel.hip): off (budget 0) in a new context
    struct LabelStep {
        uint32_t* index = nullptr;           // the chunks the edit stored ...
        uint4* old = nullptr;                // ... and the 16 bytes each held on the other side of the step
        uint64_t records = 0;
        volym_relabel_result result = {};    // the edit's result: names the labels an undo (left) and a redo (arrived) send texels to
    };
    uint64_t history_budget = 0;
    std::vector<LabelStep> history_steps;    // oldest first: [0, history_cursor) can be undone, the rest redone (the nearest first)
    size_t history_cursor = 0;
    uint64_t history_used = 0;               // 20 * records over history_steps
    uint64_t history_dropped = 0, history_lost = 0;
    volym::OwnedBuffer<uint32_t> journal_index;   // where an edit journals: room for the worst case of its slab within the budget
                                                  // (and where the smoothing's vote leaves its records, history on or off: smooth.hip)
    volym::OwnedBuffer<uint4> journal_old;

    // the lasso (volym_lasso_labels, lasso.hip): the polygon's bit plane of the latest call over lasso_rect; count: its words
    volym::OwnedBuffer<uint32_t> lasso_plane;
    uint32_t lasso_rect[4] = {};
    bool lasso_have = false;                 // a call has passed its checks: volym_read_lasso_mask has something to read

    bool feedback = true;
    bool feedback_frozen = false;               // dev
    int wide_waves = 0;                         // dev: 0 default choice, 12 or 16 (raymarch.hip launch_march)
    volym::ListSettings list_settings;          // how the work lists are dealt (worklist.hpp)
    bool bricked = false;
    uint64_t brick_from_bytes = 64ull << 20;
    int layout_choice = -1;
    int n_cus = 256;
    uint32_t wgs_per_cu = 1;
    bool culling = true;
    bool setup_ieee = false;                    // VOLYM_OPT_SETUP_IEEE: make_ray with plain divisions (FrameParams::setup_lo = +inf)
    bool texel_bytes = true;                    // VOLYM_OPT_TEXEL_BYTES: 256-cubed linear volumes march in volym_raymarch_cube256_kernel
    bool last_march_cube256 = false;            // ... and whether the latest plain launch of kernel 2 was that kernel (volym_texel_bytes_in_use)
    bool straight_jobs = false;                 // dev switch (option 121): CJ = 2 instantiation for the straight look-ahead
    bool lds_bricks = false;        // dev option 122: LDS-staged bricks in the common instantiation (bricked layout)
    volym_camera_uniforms cam_copy;
    volym_parameter_uniforms par_copy;
    int kernel_variant = 2;
    bool write_f32 = false;
    uint32_t xcd_bands = 0;

    // slot 0 always exists; slot 1 while VOLYM_OPT_FRAMES_IN_FLIGHT = 2, and then volym_compute_pass alternates between them
    std::unique_ptr<volym::FrameSlot> slots[2];
    int last = 0;                               // the slot the latest volym_compute_pass went to
    int last_blit = 0;                          // ... and the latest volym_blit
    uint32_t flight_parity = 0;
    std::string err;

    int n_slots() const { return slots[1] ? 2 : 1; }
    volym::FrameSlot& slot0() { return *slots[0]; }
    uint32_t* frame_buf(const volym::FrameSlot& s) const { return bound_frame ? bound_frame : s.d_frame_own; }
    uint32_t* shard_buf(const volym::FrameSlot& s) const { return bound_shard ? bound_shard : s.d_shard_own; }
};

namespace volym {

// one plain ray-march launch of slot 0 on its stream (what volym_compute_pass enqueues); used by the multi-GPU loop
int ctx_launch_march(volym_ctx* c);

// the seam between the frame loop (raymarch.hip) and the scene's bytes (scene_bytes.hip); all blocking set-up path
// raymarch.hip: every slot's feedback at rest and stream idle, before what the slots share is rewritten or freed
int quiesce_slots(volym_ctx* c);
// raymarch.hip: the work lists of every slot in geometric order, no costs (the costs no longer describe the scene)
int rebuild_lists(volym_ctx* c);
// raymarch.hip: the look-ahead's reject box of a frame from imp_box_*
void set_reject_box(const volym_ctx* c, FrameParams& fp);
// pick.hip: what the context keeps for the pick pass (every stream idle)
void free_pick(volym_ctx* c);
// outline.hip: what the context keeps for the outline pass (every stream idle)
void free_outline(volym_ctx* c);
// slice.hip: what the context keeps for the slice pass (every stream idle)
void free_slice(volym_ctx* c);
// project.hip: what the context keeps for the projection pass (every stream idle)
void free_projection(volym_ctx* c);
// measure.hip: what the context keeps for the measure pass (every stream idle)
void free_measure(volym_ctx* c);
// surface.hip: what the context keeps for the surface passes (every stream idle)
void free_surface(volym_ctx* c);
// components.hip: what the context keeps for the components pass (every stream idle)
void free_components(volym_ctx* c);
// distance.hip: what the context keeps for the distance pass (every stream idle)
void free_distance(volym_ctx* c);
// nearest.hip: what the context keeps for the nearest pass (every stream idle)
void free_nearest(volym_ctx* c);
// geodesic.hip: what the context keeps for the geodesic pass (every stream idle)
void free_geodesic(volym_ctx* c);
// geodesic.hip: the flood's edit by any key map of the flood's format (key >> 8 in the band, key & 0xff the label that takes), box-linear
// over pass_box, which holds f->box: volym_flood_labels by the geodesic map, volym_spread_labels (cost.hip) by the cost map.  `who` names
// the call in errors.  The request and the context's state are checked by the caller.
int flood_by_map(volym_ctx* c, const volym_flood* f, const uint32_t* keys, const uint32_t pass_box[6], const char* who, volym_relabel_result& res);
// cost.hip: what the context keeps for the cost pass (every stream idle)
void free_cost(volym_ctx* c);
// interpolate.hip: what the context keeps for the interpolate pass (every stream idle)
void free_interpolate(volym_ctx* c);
// relabel.hip: the steps of the label history, when the labels they belong to are replaced or dropped (the budget stays)
void clear_label_history(volym_ctx* c);
// relabel.hip: the steps and the staging area of the label history (every stream idle)
void free_label_history(volym_ctx* c);
// lasso.hip: what the context keeps of the latest lasso (every stream idle)
void free_lasso(volym_ctx* c);
// scene_bytes.hip: macro-cell maxima of d_vol for mc_n, their host copy and the occupied-cell boxes, and the fine maxima (sets have_vol)
int build_macro_cells(volym_ctx* c);
// scene_bytes.hip: the fine maxima alone, after VOLYM_OPT_BOUNDS_CELLS changed under a volume
int build_fine_cells(volym_ctx* c);

}  // namespace volym

#define VOLYM_HIPCHK(ctx, expr)                                                                          \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return volym::ctx_fail(ctx, VOLYM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- what the read-only passes (pick, outline, slice, projection, measure, surface, components, distance) and the blit share on the host ----
namespace volym {

// `bytes` of device memory to host memory behind the work of `stream`, blocking: what every volym_read_* ends in
inline int read_back(volym_ctx* c, hipStream_t stream, void* out, const void* src, size_t bytes)
{
    VOLYM_HIPCHK(c, hipSetDevice(c->device));
    VOLYM_HIPCHK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, stream));
    VOLYM_HIPCHK(c, hipStreamSynchronize(stream));
    return VOLYM_OK;
}

template <class T>
int OwnedBuffer<T>::reserve(volym_ctx* c, hipStream_t stream, size_t need, const char* what)
{
    if (need <= capacity) return VOLYM_OK;
    VOLYM_HIPCHK(c, hipStreamSynchronize(stream));
    release();                               // (a failing hipFree follows a sticky error that the next call reports anyway)
    const hipError_t e = hipMalloc(&ptr, need * sizeof(T));
    if (e != hipSuccess) { ptr = nullptr; return ctx_fail(c, VOLYM_E_NOMEM, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e)); }
    capacity = need;
    return VOLYM_OK;
}

template <class T>
int OwnedBuffer<T>::read(volym_ctx* c, hipStream_t stream, void* out, size_t n) const
{
    return read_back(c, stream, out, ptr, n * sizeof(T));
}

inline int RowOffsets::reserve(volym_ctx* c, hipStream_t stream, size_t n_rows, const char* what)
{
    if (n_rows <= rows.capacity) return VOLYM_OK;
    int rc = rows.reserve(c, stream, n_rows, what);
    if (rc == VOLYM_OK) { sums.release(); rc = sums.reserve(c, stream, (n_rows + VOLYM_SURFACE_SCAN_ROWS - 1u) / VOLYM_SURFACE_SCAN_ROWS, what); }
    if (rc != VOLYM_OK) release();
    return rc;
}

inline uint32_t pack_rgba(const uint8_t c[4])
{
    return static_cast<uint32_t>(c[0]) | static_cast<uint32_t>(c[1]) << 8 | static_cast<uint32_t>(c[2]) << 16 | static_cast<uint32_t>(c[3]) << 24;
}

// labels of the volume's dimensions are on the device (labels of any other dimensions count as absent)
inline bool labels_fit(const volym_ctx* c) { return c->d_labels && c->lnx == c->nx && c->lny == c->ny && c->lnz == c->nz; }

// r = rect, or the whole frame for NULL; a rect that is empty or reaches outside the frame is refused in the name of `who`
inline int frame_rect(volym_ctx* c, const uint32_t rect[4], const char* who, uint32_t r[4])
{
    const uint32_t whole[4] = {0u, 0u, c->W, c->H};
    for (int k = 0; k < 4; ++k) r[k] = rect ? rect[k] : whole[k];
    if (r[2] == 0u || r[3] == 0u || r[0] >= c->W || r[1] >= c->H || r[2] > c->W - r[0] || r[3] > c->H - r[1])
        return ctx_fail(c, VOLYM_E_INVALID, std::string(who) + ": the rect must be non-empty and inside the frame");
    return VOLYM_OK;
}

// the 256 + 256 dwords that travel with a slice or projection launch: the request's palette and the context's transfer function
inline void pack_palette_and_lut(const volym_ctx* c, const uint8_t palette[256][4], uint32_t out_palette[256], uint32_t out_lut[256])
{
    for (uint32_t l = 0; l < 256u; ++l) out_palette[l] = pack_rgba(palette[l]);
    for (uint32_t l = 0; l < 256u; ++l) out_lut[l] = l < c->tf_n ? pack_rgba(c->lut + 4u * l) : 0u;
}

// The box of a request over the scene's bytes (measure, surface, components, distance), {lo[3], hi[3]} in texels: the whole volume, and the check
// lo <= hi <= dims on every axis.  No context: the volym_*_check calls run without a device.
inline void whole_volume_box(const uint32_t dims[3], uint32_t box[6])
{
    for (int a = 0; a < 3; ++a) { box[a] = 0u; box[3 + a] = dims[a]; }
}
inline bool box_in_volume(const uint32_t box[6], const uint32_t dims[3])
{
    for (int a = 0; a < 3; ++a) if (box[a] > box[3 + a] || box[3 + a] > dims[a]) return false;
    return true;
}
inline bool box_empty(const uint32_t box[6]) { return box[0] >= box[3] || box[1] >= box[4] || box[2] >= box[5]; }
// texels of a box that lies in a volume of at most 4096^3: below 2^36
inline uint64_t box_texels(const uint32_t box[6])
{
    return static_cast<uint64_t>(box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]);
}
// a box with lo <= hi has at most `max` < 2^32 texels: the product of three 32-bit extents in two steps -- once the first is bounded
// the second cannot wrap 64 bits; an empty box has 0 texels
inline bool box_at_most(const uint32_t box[6], uint64_t max)
{
    const uint64_t w = box[3] - box[0], h = box[4] - box[1], d = box[5] - box[2];
    return w == 0u || h == 0u || d == 0u || (w * h <= max && w * h * d <= max);
}
// ... and what such a pass refuses before it reads labels beside the density: the two uploaded under different layouts
inline int check_labels_layout(volym_ctx* c, const char* who)
{
    if (labels_fit(c) && c->labels_bricked != c->bricked)
        return ctx_fail(c, VOLYM_E_STATE, std::string(who) + ": volume and labels were uploaded under different VOLYM_OPT_VOLUME_LAYOUT settings");
    return VOLYM_OK;
}

// ---- the passes that walk a box row by row (box_walk.h: surface, components, distance) ----
// The workgroups of a walk: one wave per row and step, four waves per workgroup; at most eight workgroups per CU, but at least so
// many that no wave walks more than WALK_ROWS_PER_WAVE rows (the widths of surface_kernels.h rest on it).  A permitted box has at most
// 4096^2 = 2^24 rows, so that floor is at most 2^24 / 16384 = 1024 workgroups; on a device of 256 CUs the cap is 2048, and wherever
// 8 * n_cus >= ceil(n_rows / 16384) the floor changes nothing: the grid is max(min(ceil(n_rows / 4), 8 * n_cus), 1).
constexpr uint32_t WALK_ROWS_PER_WAVE = 4096u;
inline uint32_t walk_grid(const volym_ctx* c, uint32_t n_rows)
{
    const uint32_t wanted = (n_rows + 3u) / 4u, floor_grid = (n_rows + 4u * WALK_ROWS_PER_WAVE - 1u) / (4u * WALK_ROWS_PER_WAVE);
    return std::max(std::max(std::min(wanted, static_cast<uint32_t>(c->n_cus) * 8u), floor_grid), 1u);
}
// box_pass.hip: rows[0 .. n_rows) from counts into their exclusive prefix sums, in place, on `stream`; sums holds the block sums
// (RowOffsets).  Sums wrap at 2^32.  Enqueue-only.
int scan_row_offsets(volym_ctx* c, hipStream_t stream, const RowOffsets& offsets, uint32_t n_rows);
// box_pass.hip: what volym_read_component_ids and volym_read_distance_map are.  `src` is a uint32 volume over `box`, box-linear; its
// part over `sub` (NULL: all of it) goes to `out` behind the work of slot 0's stream, blocking.  `have`: the pass `pass` has written
// it; the messages are in the name of `who`.
int read_box_volume(volym_ctx* c, const char* who, const char* pass, bool have, const uint32_t box[6], const uint32_t* src, const uint32_t sub[6],
                    uint32_t* out);
// box_pass.hip: ... and volym_component_of and volym_distance_at: the one word of texel (x, y, z)
int read_box_texel(volym_ctx* c, const char* who, const char* pass, bool have, const uint32_t box[6], const uint32_t* src, uint32_t x, uint32_t y,
                   uint32_t z, uint32_t* out);

}  // namespace volym
