/*
 * volym_hip.h -- C ABI of the MI355X-native ray-march path (libvolym_hip.so).
 *
 * This is the drop-in boundary for the reference's compute plugin:
 *
 *     trait ComputeDemo { fn init(ctx, state, output_texture) -> Result<Self>;
 *                         fn update_gpu_state(&self, ctx, state) -> Result<()>;
 *                         fn compute_pass(&self, ctx) -> Result<()>; }
 *                                              -- /root/reference/src/demos/mod.rs:9-17
 *
 * and for the wgpu resource wrappers it owns (src/gpu_resources/, src/gpu_context.rs,
 * src/demos/pipeline.rs).  Plain C, no C++/torch types, no exceptions: a Rust
 * `extern "C"` block binds it unchanged (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success or a negative VOLYM_E_* code; the text of
 *     the last failure is volym_last_error(ctx) (volym_last_error(NULL) for create).
 *   - a context is bound to one device and is NOT thread-safe (the reference calls
 *     everything from the winit event-loop thread, src/event_loop.rs:62).
 *   - volym_set_* copy from caller memory; the caller may free immediately (as
 *     queue.write_texture does, src/gpu_resources/volume.rs:81-90).
 *   - volym_update and volym_compute_pass only enqueue (src/demos/pipeline.rs:97 queue.submit): no allocation,
 *     no stream synchronisation on their path.  The one exception is spelled out at volym_update.
 *     Blocking calls: volym_create / volym_destroy, volym_set_* (uploads; they also wait for the frames in flight),
 *     volym_set_option, volym_set_shard, volym_set_stream, volym_sync, volym_settle, volym_read_*, volym_packed_tiles,
 *     volym_assemble_host, volym_stats_pass, volym_time_*; volym_blit blocks only when it has to (re)size its own target, and
 *     volym_surface_faces_pass when it has to learn the face total of its surface pass or grow the context's own face buffer;
 *     volym_components_pass blocks only when it has to allocate or grow its buffers; volym_read_components,
 *     volym_read_component_table, volym_read_component_ids and volym_component_of block (they are volym_read_* in all but name);
 *     volym_distance_pass blocks only when it has to allocate or grow its buffers; volym_read_distance, volym_read_distance_map
 *     and volym_distance_at block; volym_nearest_pass, its reads and volym_nearest_at likewise; volym_geodesic_pass BLOCKS (it
 *     reads 4 bytes after every batch of its rounds), and so do its reads and volym_geodesic_at; volym_cost_pass BLOCKS in the
 *     same way, and so do its reads and volym_cost_at; volym_interpolate_pass blocks only when it has to allocate or grow its
 *     buffers, its reads and volym_interpolate_at block; volym_edit_labels and the other
 *     label edits (brush, lasso, smooth, fill, flood, spread, interpolate) are set-up calls and block like volym_set_*.
 *   - the default kernel schedules its work from lists that a feedback thread inside the library re-deals from the
 *     counted cost of earlier frames (asynchronously: a frame never waits for it, and every list renders the same
 *     pixels); volym_settle runs that loop to its fixed point for the current view.
 */
#ifndef VOLYM_HIP_H
#define VOLYM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOLYM_ABI_VERSION 2

enum {
    VOLYM_OK = 0,
    VOLYM_E_INVALID = -1,   /* bad argument / call order */
    VOLYM_E_HIP = -2,       /* a HIP runtime call failed */
    VOLYM_E_NO_DEVICE = -3, /* no usable gfx950 device */
    VOLYM_E_NOMEM = -4,
    VOLYM_E_STATE = -5      /* volume / importances / transfer function not all set */
};

/* Volume sampler.  NEAREST is what the reference runs (SamplerDescriptor::default(),
 * src/gpu_resources/volume.rs:92-95); LINEAR is the trilinear mode BASELINE.json names. */
enum { VOLYM_FILTER_NEAREST = 0, VOLYM_FILTER_LINEAR = 1 };

/* volym_set_option keys */
enum {
    VOLYM_OPT_KERNEL = 1,     /* 0 = direct march (every reference fetch issued),
                                 1 = macro-cell march: empty-space fetches elided, step
                                     arithmetic replayed exactly,
                                 2 = (default) 1 + persistent workgroups, centre-first tile
                                     order, per-wave shading queue, speculative sample batches,
                                 3 = ray pool (round 3): ray state in LDS, phase lists, pixel-block
                                     lattice dealing, no work list and no cost feedback; the common
                                     flag set only (nearest filter, opacity on, no importance mode --
                                     every other frame runs kernel 2); same pixels as 2, ~3x slower at
                                     1920x1080 */
    VOLYM_OPT_WRITE_F32 = 2,  /* 1 = also store pre-quantisation float RGBA (parity tests) */
    VOLYM_OPT_MACRO_CELLS = 3, /* macro cells per axis (power of two, 4..32; default 32)    */
    VOLYM_OPT_VOLUME_LAYOUT = 4, /* device layout of the NEXT volume / importance upload: -1 = by size (default: 4x4x4
                                    bricks above 64 MiB), 0 = linear, 1 = bricks.  Invisible at this boundary. */
    VOLYM_OPT_CULLING = 5,     /* 0 = no exact culling (projected hulls, AABB clip, per-view tile mask of the occupied cells) in
                                  kernel 2; default 1 */
    VOLYM_OPT_COST_FEEDBACK = 6, /* 0 = kernel 2 keeps its centre-first work list; default 1 (lists re-dealt from counted costs) */
    VOLYM_OPT_DEPTH_PARALLEL = 7, /* tile cost from which kernel 2 marches a tile as four depth-parallel quarter items:
                                    < 0 adaptive (-N = N/10 x a wave's fair share of the frame; -1 = default), 0 never, > 0 explicit */
    VOLYM_OPT_XCD_BANDS = 8,   /* kernels 0/1: block -> tile remap bands per XCD (0 = identity, default) */
    VOLYM_OPT_REBALANCE_ROUNDS = 9, /* kernel 2: after a standing view's list is dealt, re-balance it this many times (0..8) from
                                    the times its workgroups took (measured: the list then depends on the weather).  Default 0. */
    VOLYM_OPT_FRAMES_IN_FLIGHT = 11, /* 1 (default) = one frame after the other on the context's stream.  2 = the context keeps a
                                  second frame slot (stream, frame buffer, tables, distance field, lists, feedback) that marches
                                  the same scene, and volym_compute_pass alternates between the two: a frame of the persistent kernel
                                  ends on its longest chains, and the next frame's workgroups take the CUs it leaves idle
                                  (1920x1080: 31.9 -> 27.6 us per frame; 3840x2160: 74.7 -> 70.7).  Set it before the volume,
                                  the importances and the transfer function, and not with a caller's stream.
                                  volym_update / _settle / _sync / _set_* and volym_bind_output act on both slots; volym_read_rgba8 /
                                  _rgba32f / volym_blit and volym_frame_device_ptr / _shard_device_ptr take the frame of the
                                  latest pass; volym_throttle marks it; volym_stats_pass, volym_time_*
                                  and volym_selftest_ray_setup use the first slot alone (one frame at a time); the shard /
                                  pack / assemble calls and volym_set_stream return VOLYM_E_STATE.  Memory: the volume,
                                  importances and macro cells once; the frame buffers, tables and work lists twice. */
    VOLYM_OPT_BOUNDS_CELLS = 12, /* cells per axis of the grid of density maxima that a standing view's tile mask and per-tile depth
                                  bounds are built from, once per view: -1 (default) = by the volume's size (volym_bounds_cells_for:
                                  cells of two voxels on the longest axis, at most VOLYM_BOUNDS_CELLS_DEFAULT_MAX, never fewer than the
                                  macro cells), 0 = the macro cells themselves, else a power of two from VOLYM_OPT_MACRO_CELLS to
                                  VOLYM_BOUNDS_CELLS_MAX.  Same pixels for every value: a finer grid only trims more constant tiles
                                  and more of the empty ends of the rays.  The march loop does not read the grid.  A view with the
                                  cone look-ahead (use_importance_rendering and use_cone_importance_check) keeps the macro cells.  Blocking; with a
                                  volume on the device it rebuilds the grid, and every view gets a new mask. */
    VOLYM_OPT_TEXEL_BYTES = 13, /* 1 (default) = a volume of 256 x 256 x 256 texels in the linear layout, marched by kernel 2 with opacity
                                  on, the nearest filter and no importance mode, runs volym_raymarch_cube256_kernel: the texel address
                                  is the three clamped coordinates as bytes side by side, one saturating conversion each
                                  (raymarch_device.h texel256_insert; volym_selftest_texel256).  0 = the general kernel.  Same
                                  pixels for either value; every other volume, flag set and the instrumented launch run the general
                                  kernels whatever it is.  Takes effect with the next pass. */
    VOLYM_OPT_SETUP_IEEE = 10  /* 1 = the ray set-up (wgsl:221-241) runs its 14 divisions as 14 plain IEEE divisions; default 0: the
                                  divisions that share a denominator share its refined reciprocal -- the same instructions on the
                                  same values, so the same bits (raymarch_device.h make_ray; volym_selftest_ray_setup).  Takes
                                  effect with the next volym_update. */
};

/* CameraUniforms, byte-for-byte (src/gpu_resources/camera.rs:56-64; WGSL mirror
 * shaders/importance_driven_volume_rendering.wgsl:2-7).  Column-major m[col][row]. */
typedef struct volym_camera_uniforms {
    float view_matrix[4][4];
    float projection_matrix[4][4];
    float inverse_view_proj[4][4];
    float camera_position[3];
    float _padding;
} volym_camera_uniforms;

/* ParameterUniforms, byte-for-byte (src/gpu_resources/parameters.rs:55-66; WGSL mirror
 * shaders/importance_driven_volume_rendering.wgsl:9-18). */
typedef struct volym_parameter_uniforms {
    float density_threshold;
    uint32_t use_cone_importance_check;
    uint32_t use_importance_coloring;
    uint32_t use_opacity;
    uint32_t use_importance_rendering;
    uint32_t use_gaussian_smoothing;
    uint32_t importance_check_ahead_steps;
    float raymarching_step_size;
} volym_parameter_uniforms;

/* Reference texture fetches of the current frame, counted by an instrumented
 * (untimed) launch: B_alg = n_vol*b_vol + n_imp + 4*W*H  (SURVEY.md section 8d). */
typedef struct volym_stats {
    uint64_t n_vol;    /* density fetches the reference shader executes   */
    uint64_t n_imp;    /* importance fetches the reference shader executes */
    uint64_t n_steps;  /* march-loop iterations                             */
    uint64_t n_dense;  /* iterations with rho >= density_threshold          */
    uint64_t n_hit;    /* rays that hit the unit cube                       */
    uint64_t n_rays;   /* pixels owned by this context (all of them count)  */
} volym_stats;

typedef struct volym_ctx volym_ctx;

/* --- lifetime: GpuContext::new + GpuWriteTexture2D::new (src/gpu_context.rs:20-62,
 * src/gpu_resources/texture.rs:40-59).  device_id < 0 = current device. */
int volym_create(volym_ctx** out, uint32_t width, uint32_t height, int device_id);
void volym_destroy(volym_ctx* ctx);
const char* volym_last_error(const volym_ctx* ctx);
int volym_abi_version(void);

/* Use the caller's HIP stream (hipStream_t as void*; NULL = the context's own). */
int volym_set_stream(volym_ctx* ctx, void* hip_stream);
int volym_set_option(volym_ctx* ctx, int key, int value);

/* Screen-tile sharding: this context renders the 16x16 tiles
 * k with k % world == rank into a compact buffer of volym_local_tiles() tiles. */
int volym_set_shard(volym_ctx* ctx, uint32_t rank, uint32_t world);

/* --- resources: Simple::init (src/demos/simple/mod.rs:36-110) --------------------- */
/* GpuVolume::init upload (src/gpu_resources/volume.rs:63-95): nx*ny*nz bytes, x fastest,
 * already padded/flipped by the host shim (volym_host.h volym_prepare_volume).  The caller's
 * layout is always x fastest; on the device, volumes above 64 MiB are re-laid into 4x4x4 bricks
 * (DESIGN.md section 3), which is invisible at this boundary. */
int volym_set_volume(volym_ctx* ctx, const uint8_t* voxels, uint32_t nx, uint32_t ny,
                     uint32_t nz, int filter);
/* GpuImportances::init upload (src/demos/simple/importance.rs:93-131); same dims. */
int volym_set_importances(volym_ctx* ctx, const uint8_t* importances, uint32_t nx,
                          uint32_t ny, uint32_t nz);
/* Segment importances on the device (new; the reference maps labels on the host, importance.rs:148-158, and uploads the result).
 * volym_set_labels: nx*ny*nz label bytes, prepared like the volume (volym_prepare_volume: padded, flipped).  Kept on the device in
 * the layout the importances get (VOLYM_OPT_VOLUME_LAYOUT / the size rule); one pass counts, per label value, its voxels and
 * their texel AABB.  Leaves the importances (and whether there are any) as they were.  Label dims must match the volume's
 * exactly as importances must: volym_update refuses a mismatch.  Blocking set-up call, like volym_set_importances. */
int volym_set_labels(volym_ctx* ctx, const uint8_t* labels, uint32_t nx, uint32_t ny, uint32_t nz);
/* importance(voxel) = table[label(voxel)] for every voxel, computed on the device into the importance volume the march reads:
 * the same state as volym_set_importances with the host-mapped bytes (device bytes, important-texel box, work lists).  The box
 * is the union of the boxes of the labels with table[l] >= 128: no pass over the voxels on the host.  The frames enqueued after
 * the call use the new importances, with or without a volym_update in between; those enqueued before it the old ones (it waits
 * for them, in every frame slot).  VOLYM_E_STATE without labels; volym_set_importances drops the labels, so a table after it is
 * VOLYM_E_STATE as well.  Blocking set-up call, but no upload. */
int volym_set_segment_importances(volym_ctx* ctx, const uint8_t table[256]);
/* Voxel count per label value, from the volym_set_labels pass (the reference logs such a histogram, importance.rs:83-91).
 * Counts the whole label volume, whatever the crop box.  VOLYM_E_STATE without labels. */
int volym_label_counts(volym_ctx* ctx, uint64_t counts[256]);
/* The grids of density maxima (macro cells, and the finer grid of VOLYM_OPT_BOUNDS_CELLS) divide an axis of `dim` voxels into
 * n_cells cells; cell k covers the voxels a nearest-filter sample at a position in [k / n_cells, (k + 1) / n_cells) can select,
 * and one more voxel on either side.  volym_cells_meeting_box: the cells whose voxels meet [lo, hi), as [*c0, *c1); none, and
 * lo >= hi, give *c0 == *c1 == 0.  An edit that rewrites a box of texels refreshes exactly these cells of each grid.  Pure host
 * arithmetic, no context.  VOLYM_E_INVALID for NULL, n_cells outside 1..4096 or dim outside 1..65536. */
int volym_cells_meeting_box(uint32_t n_cells, uint32_t dim, uint32_t lo, uint32_t hi, uint32_t* c0, uint32_t* c1);
/* The default of VOLYM_OPT_BOUNDS_CELLS for a volume of dims[0] x dims[1] x dims[2] voxels and that many macro cells per axis. */
#define VOLYM_BOUNDS_CELLS_MAX 128u         /* the largest grid the option takes */
#define VOLYM_BOUNDS_CELLS_DEFAULT_MAX 64u  /* the largest the default takes: 128 costs a view more to build than it gives back */
uint32_t volym_bounds_cells_for(const uint32_t dims[3], uint32_t macro_cells);
/* Axis-aligned crop box on the device (new; the reference has none).  The frames enqueued after the call are the frames of the
 * same scene in which every density byte AND every importance byte of a texel outside the box is 0 (an important structure
 * that is cut away stops suppressing what lies in front of it).  lo inclusive, hi exclusive, in texels of the volume as
 * volym_set_volume received it (prepared: padded, Y-flipped), x first.  Valid: lo[a] <= hi[a] <= n[a] on every axis; an empty
 * box (lo == hi on some axis) renders the background everywhere; anything else is VOLYM_E_INVALID, a call without a volume
 * VOLYM_E_STATE.  The whole volume [0, n) means "no crop" and is the state after volym_set_volume, which resets the box.
 * The box belongs to the scene: volym_set_importances and volym_set_labels + volym_set_segment_importances made after a crop
 * give cropped importances.  Blocking set-up call with the semantics of volym_set_segment_importances: it waits for the frames
 * in flight in every frame slot (they show the old box), and needs no volym_update before the next volym_compute_pass.  No
 * pass over voxels on the host and no upload: the first crop makes a device copy of the uncropped density (and of uploaded
 * importances; labels on the device serve as their own source), and every edit rewrites only the slabs of texels between the
 * old faces and the new ones, then the macro cells those slabs touch.  Memory: one more volume (two with uploaded
 * importances) from the first crop until the next volym_set_volume; nothing in a context that never crops. */
int volym_set_crop_box(volym_ctx* ctx, const uint32_t lo[3], const uint32_t hi[3]);
int volym_get_crop_box(volym_ctx* ctx, uint32_t lo[3], uint32_t hi[3]);
/* The slabs volym_set_crop_box rewrites when the box goes from [old_lo, old_hi) to [new_lo, new_hi): at most six boxes
 * {x0, y0, z0, x1, y1, z1} whose union holds every texel that is in exactly one of the two boxes; *n_slabs of them are written
 * (0 when the boxes are equal).  Pure host arithmetic, no context.  VOLYM_E_INVALID for NULL or lo > hi. */
int volym_crop_slabs(const uint32_t old_lo[3], const uint32_t old_hi[3], const uint32_t new_lo[3], const uint32_t new_hi[3],
                     uint32_t slabs[6][6], uint32_t* n_slabs);
/* Oblique clip plane on the device (new; the reference has none): the cut the box cannot make.  A plane is an integer normal n
 * and an integer offset d; texel (x, y, z) -- the coordinates volym_set_crop_box and the pick records use -- is KEPT iff
 * n[0]*x + n[1]*y + n[2]*z <= d.  The frames enqueued after the call are the frames of the same scene in which every density
 * byte AND every importance byte of a texel that is not kept is 0.  Valid: |n[a]| <= VOLYM_CLIP_PLANE_MAX on every axis, and
 * n == (0, 0, 0) only with d == 0, which means "no plane" and is the state after volym_set_volume (to keep nothing use e.g.
 * n = (1, 0, 0), d = -1); anything else is VOLYM_E_INVALID, a call without a volume VOLYM_E_STATE.  With these bounds and the
 * 4096 texels per axis volym_set_volume admits, |n . t| <= 3 * 4096 * 4099 < 2^31 (4099: the walk also evaluates a brick's padding texels): the test is exact in 32-bit integers on host
 * and device, for every volume the library holds.
 *   Box, plane and mask commute: any interleaving of volym_set_crop_box, volym_set_clip_plane and
 * volym_set_segment_visibility that ends at the same (box, plane, mask) leaves the same bytes, and a box that grows over clipped
 * texels leaves them 0.  The plane belongs to the scene as the box does: volym_set_volume resets it, and volym_set_importances,
 * volym_set_labels and volym_set_segment_importances made under a plane give clipped importances.  Blocking set-up call with the
 * semantics of volym_set_crop_box: it waits for the frames in flight in every frame slot (they show the old plane), needs no
 * volym_update before the next volym_compute_pass, makes no pass over voxels on the host and no upload.  The first cut of any
 * kind (box, plane, mask) makes the uncut device copies; an edit walks the box of volym_clip_plane_box and stores only the
 * 16-byte chunks in which a texel changes side, then refreshes the macro cells that box touches.  A plane equal to the current
 * one returns at once.  A failure after the first kernel of an edit leaves the context asking for volym_set_volume again. */
#define VOLYM_CLIP_PLANE_MAX 4096
int volym_set_clip_plane(volym_ctx* ctx, const int32_t n[3], int32_t d);
int volym_get_clip_plane(volym_ctx* ctx, int32_t n[3], int32_t* d);
/* The box of texels volym_set_clip_plane walks when the plane goes from (old_n, old_d) to (new_n, new_d) inside [lo, hi): 0 or 1
 * boxes {x0, y0, z0, x1, y1, z1} (hi exclusive) inside [lo, hi) that hold every texel of [lo, hi) the two planes classify
 * differently; *n_boxes is 0 when there is no such texel, in particular when the planes are equal.  The box is tight in this
 * sense: over an outer slice of it, normal to an axis, the two predicates are not both constant and equal (the extremes of n . t
 * over a slice are exact).  Pure host arithmetic, no context.  VOLYM_E_INVALID for NULL, an invalid plane, lo > hi or
 * hi > 65536. */
int volym_clip_plane_box(const int32_t old_n[3], int32_t old_d, const int32_t new_n[3], int32_t new_d, const uint32_t lo[3],
                         const uint32_t hi[3], uint32_t box[6], uint32_t* n_boxes);
/* Segment visibility on the device (new; the reference has none): switch segments off without touching the volume on the host.
 * visible[l] != 0 shows label value l.  The frames enqueued after the call are the frames of the same scene in which every
 * density byte AND every importance byte of a texel whose label is hidden, or that lies outside the crop box, is 0 (a hidden
 * structure stops suppressing what lies in front of it, as a cropped one does).  Crop box and mask commute: any interleaving of
 * volym_set_crop_box and this call that ends at the same (box, mask) leaves the same bytes, and a box that grows over hidden
 * texels leaves them 0.
 *   Call order: needs a volume and labels on the device whose dimensions equal the volume's, else VOLYM_E_STATE; NULL context or
 * table VOLYM_E_INVALID.  Volume, labels (and importances) held in different device layouts -- VOLYM_OPT_VOLUME_LAYOUT changed
 * between their uploads -- are refused with VOLYM_E_STATE as well.
 *   Blocking set-up call with the semantics of volym_set_segment_importances: it waits for the frames in flight in every frame
 * slot (they show the old mask), and needs no volym_update before the next volym_compute_pass.  A mask equal to the current one
 * returns at once.  A label value without voxels is accepted and toggling it changes nothing; label 0 (which covers the padding)
 * can be hidden like any other.
 *   The mask belongs to the labels.  Initially all visible; volym_set_labels resets it to all visible (new labels, new
 * segments), volym_set_importances drops the labels and with them the mask, volym_set_volume resets it as it resets the box:
 * after any of the three the scene is that of the crop box alone, the hidden texels have their bytes back (where a call of the
 * three then fails on its arguments, the mask is reset all the same).  volym_set_segment_importances called while segments are
 * hidden gives importances with those segments hidden, and the look-ahead's reject box is then that of the labels with
 * table[l] >= 128 that are visible, cut to the crop box (with uploaded importances: their box, cut to the crop box).
 * volym_label_counts keeps counting the whole label volume.
 *   No pass over voxels on the host, no upload: an edit rewrites the texels inside the boxes of the labels that flipped, cut to
 * the crop box (volym_visibility_boxes), skipping every 16-byte chunk without a texel of such a label, then the macro cells
 * those boxes touch.  Memory: the uncropped copies of the crop box (volym_set_crop_box), made by the first hide or the first
 * crop, whichever comes first; the copy of the importances only when they were uploaded rather than mapped from the labels;
 * nothing in a context that never hides or crops.  A failure after the first kernel of an edit leaves bytes that belong to
 * neither mask, and the context then asks for volym_set_volume again. */
int volym_set_segment_visibility(volym_ctx* ctx, const uint8_t visible[256]);
/* The current mask as 0 / 1 per label value (all 1 without labels). */
int volym_get_segment_visibility(volym_ctx* ctx, uint8_t visible[256]);
/* The boxes of texels volym_set_segment_visibility rewrites when the labels with flipped[l] != 0 change visibility: at most
 * VOLYM_VISIBILITY_MAX_BOXES boxes {x0, y0, z0, x1, y1, z1} (hi exclusive) inside the crop box [crop_lo, crop_hi) whose union
 * holds every texel of a flipped label inside the crop box; *n_boxes of them are written.  counts[l] and label_boxes[l]
 * ({x0, y0, z0, x1, y1, z1}, hi INCLUSIVE) are the voxel count and texel AABB of label l, as the volym_set_labels pass finds
 * them; a label without voxels is skipped.  The rule: every flipped label's box, cut to the crop box, joins the first box so far
 * whose hull with it holds no more texels than the two apart (overlapping and nested boxes: nothing is read twice); else it
 * becomes a box of its own while there is room; else it joins the box that grows least.  At the end, boxes are joined while a
 * hull holds no more texels than its two boxes.  So one label costs one launch over its own box, and 200 labels at most
 * VOLYM_VISIBILITY_MAX_BOXES launches.  Pure host arithmetic, no context.  VOLYM_E_INVALID for NULL, crop_lo > crop_hi or a
 * counted label with a negative or inverted box. */
#define VOLYM_VISIBILITY_MAX_BOXES 8
int volym_visibility_boxes(const uint8_t flipped[256], const uint64_t counts[256], const int32_t label_boxes[256][6], const uint32_t crop_lo[3],
                           const uint32_t crop_hi[3], uint32_t boxes[VOLYM_VISIBILITY_MAX_BOXES][6], uint32_t* n_boxes);
/* GPUTransferFunction::new_texture_1d_rgbt upload (src/gpu_resources/transfer_function.rs:36-90):
 * n RGBA8 texels (the reference uses n = 256), Linear/ClampToEdge sampler. */
int volym_set_transfer_function(volym_ctx* ctx, const uint8_t* rgba8, uint32_t n);

/* --- per frame ------------------------------------------------------------------ */
/* ComputeDemo::update_gpu_state (src/demos/pipeline.rs:208-212): GpuCamera::update +
 * GpuParameters::update.  Fails with VOLYM_E_INVALID on out-of-range parameters.  Enqueue only; a change of the step size
 * or of the transfer function uploads 10 KiB of tables in stream order from a ring of 8 staging buffers, and only a caller
 * that makes 8 such changes while the device is still 8 frames behind waits for a slot.
 *
 * The camera: inverse_view_proj and camera_position are taken verbatim, and any finite pair is rendered by the shader's rule
 * (wgsl:221-234): the ray of a pixel starts at camera_position and passes through the pixel's point of the plane ndc z = 0,
 * unprojected by inverse_view_proj -- with the eye inside the volume, the volume off screen or behind the eye, any roll, field
 * of view, aspect and near plane.  The culling devices (projected hulls, the ray pool's rectangle, tile mask, tile depth
 * bounds) describe the rays only for a CONSISTENT pair, one whose camera_position is the centre of projection of the matrix, as
 * every pair from volym_camera_uniforms_from is: they are used while no point of a ray beyond the near plane projects further
 * than VOLYM_VIEW_EYE_SLACK_PIXELS from the ray's own pixel (volym_view_eye_displacement), which f32 rounding of a consistent
 * pair stays far below.  Any other pair is rendered without them: the same pixels, more time.  view_matrix and
 * projection_matrix are not read. */
int volym_update(volym_ctx* ctx, const volym_camera_uniforms* camera,
                 const volym_parameter_uniforms* parameters);
/* How far camera_position is from the centre of projection of inverse_view_proj, in pixels of a W x H frame: the largest
 * distance between the pixel of a ray and the projection, under the matrix, of a point of that ray whose clip w is at least
 * w_min (w_min <= 0: any point beyond the near plane).  0 for the exact centre; +inf where the bound fails (camera_position at
 * or beyond the near plane's w, or w_min not above its own).  Pure host arithmetic in double precision, no context (DESIGN.md
 * 4, "a consistent eye").  VOLYM_E_INVALID for NULL, an empty frame, a matrix that is singular or not finite, or one whose near
 * plane is not in front of its centre. */
#define VOLYM_VIEW_EYE_SLACK_PIXELS 0.375     /* a quarter of the 1.5 pixels by which hulls and tile rectangles are grown */
int volym_view_eye_displacement(const volym_camera_uniforms* camera, uint32_t W, uint32_t H, double w_min, double* pixels);
/* ComputeDemo::compute_pass (src/demos/pipeline.rs:62-102, :214-225): enqueue one
 * ray-march of every owned tile on the context's stream; returns immediately. */
int volym_compute_pass(volym_ctx* ctx);
int volym_sync(volym_ctx* ctx);
/* Back-pressure for a frame loop, the role surface.get_current_texture() plays in the reference (src/event_loop.rs:114: it
 * blocks while the swap chain's images are all in flight).  Call once per frame after volym_compute_pass: it marks the work
 * enqueued so far and waits until at most `max_in_flight` (1..8) such marks are outstanding.  A loop that runs hundreds of
 * frames ahead of the device also runs hundreds of frames ahead of the cost feedback of its work lists. */
int volym_throttle(volym_ctx* ctx, uint32_t max_in_flight);
/* Bring the cost feedback (see the conventions above) to rest for the current view: waits for a re-deal in flight, then
 * enqueues frames of the current view itself (exactly what volym_compute_pass enqueues: the output buffers are rewritten
 * with the same pixels) until the list in use is the final one for this view.  A handful of frames at most; blocks.
 * The frames after it run at the steady rate of a standing view.  Never needed for correctness. */
int volym_settle(volym_ctx* ctx);

/* --- output --------------------------------------------------------------------- */
/* Full-frame readback (world == 1, or after volym_assemble on the root):
 * W*H*4 bytes as the rgba8unorm store leaves them / W*H*4 floats before quantisation
 * (the latter needs VOLYM_OPT_WRITE_F32 = 1). */
int volym_read_rgba8(volym_ctx* ctx, uint8_t* out);
int volym_read_rgba32f(volym_ctx* ctx, float* out);
/* The tile mask and the per-tile depth bounds of the view of the latest pass, as the march reads them (for tests and tools).
 * volym_tile_bounds_size: the frame's 8x8 tiles per row and per column and the 32-bit words of its mask.  volym_read_tile_bounds
 * blocks and addresses the frame slot of the latest pass: mask_bits receives mask_words words, bit (i & 31) of word (i >> 5)
 * for tile i = ty * tiles_x8 + tx; near and far receive 32 * mask_words floats each, indexed by i: the range of the ray
 * parameter outside which no sample of the tile's pixels can be dense.  A tile no occupied cell projects onto has near = +inf
 * and far = 0; a view without depth bounds has near = 0 and far = +inf everywhere.  VOLYM_E_STATE while the view has no mask:
 * a standing view gets it with its second frame, a view whose scene or options changed since loses it. */
int volym_tile_bounds_size(volym_ctx* ctx, uint32_t* tiles_x8, uint32_t* tiles_y8, uint32_t* mask_words);
int volym_read_tile_bounds(volym_ctx* ctx, uint32_t* mask_bits, float* near, float* far);

/* The step after the path: RenderPipeline::render_pass (src/render_pipeline.rs:88-130) with shaders/render.wgsl:39-43 --
 * every pixel (x, y) of an out_w x out_h rgba8 target samples the frame at uv = (x + 0.5, y + 0.5) / (W, H) through a
 * Linear / ClampToEdge sampler (src/gpu_resources/texture.rs:84-101), BlendState::REPLACE.  Note the divisor: the INPUT
 * size, as in the shader, so the pass maps pixels 1:1 (a larger target repeats the edge texels, a smaller one crops).
 * target_rgba8 = device memory of out_w*out_h*4 bytes, or NULL for a target the context owns (volym_read_blit reads it
 * back).  Enqueued on the context's stream behind the frame. */
int volym_blit(volym_ctx* ctx, void* target_rgba8, uint32_t out_w, uint32_t out_h);
int volym_read_blit(volym_ctx* ctx, uint8_t* out);

/* Sharded output.  Local buffer = volym_local_tiles() tiles of 16x16 RGBA8 pixels
 * (1024 bytes each, padded to volym_shard_bytes()); device pointer for the collective. */
uint32_t volym_local_tiles(const volym_ctx* ctx);
size_t volym_shard_bytes(const volym_ctx* ctx);
/* The buffers the latest volym_compute_pass renders into (bound or the context's own); with two frames in flight, those of
 * the frame slot that ran it, so that volym_frame_device_ptr holds what volym_read_rgba8 reads. */
void* volym_shard_device_ptr(volym_ctx* ctx);
void* volym_frame_device_ptr(volym_ctx* ctx);
/* Let the caller own the device buffers (e.g. torch tensors handed to RCCL):
 * shard_rgba8 = volym_shard_bytes() bytes, frame_rgba8 = W*H*4 bytes; NULL gives the context its own back.  Takes effect for
 * passes enqueued after the call; a pass already enqueued keeps the buffers it was launched with.
 * With VOLYM_OPT_FRAMES_IN_FLIGHT = 2 both frame slots render into the bound buffers (NULL: each into its own again), so
 * consecutive passes may write one buffer at the same time.  Frames of the same view write the same pixels, and a buffer that
 * receives them is well defined.  A caller that moves the camera with two frames in flight binds a different buffer before
 * each volym_compute_pass, as a swap chain does: a ring of two or more buffers, rebound before each pass, gives every frame
 * its own.  Back to VOLYM_OPT_FRAMES_IN_FLIGHT = 1, the bound buffers stay bound (a buffer of the second slot itself excepted:
 * the context takes its own back). */
int volym_bind_output(volym_ctx* ctx, void* shard_rgba8, void* frame_rgba8);
/* Root side of the image gather: `gathered` = world shards back to back in rank order
 * (device memory, world * volym_shard_bytes() bytes) -> raster W*H*4 in the frame buffer. */
int volym_assemble(volym_ctx* ctx, const void* gathered);
/* Packed shards (new; the reference has no multi-GPU path): most 16x16 tiles of a frame are constant -- outside the
 * volume's silhouette -- and the gather only has to move the others.  volym_pack_shard enqueues, after a
 * volym_compute_pass, the compaction of the bound shard into `packed`: a header (one {slot | constant flag, value} pair per
 * local tile) followed by the 1 KiB tiles that are not constant; a tile that finds no room sets the overflow flag.
 * volym_packed_shard_bytes(ctx, tiles): bytes of a packed shard with room for `tiles` tiles (tiles >= local tiles: always
 * enough).  volym_packed_tiles: synchronises and reports how many tiles the last pack stored (size the steady-state buffers
 * with the maximum over the ranks).  volym_assemble_packed: root side, `gathered` = world packed shards `stride_bytes`
 * apart in rank order -> the raster in the frame buffer. */
size_t volym_packed_shard_bytes(const volym_ctx* ctx, uint32_t tiles);
int volym_pack_shard(volym_ctx* ctx, void* packed_device, size_t capacity_bytes);
int volym_packed_tiles(volym_ctx* ctx, uint32_t* tiles_used, uint32_t* overflowed);
int volym_assemble_packed(volym_ctx* ctx, const void* gathered_device, size_t stride_bytes);
/* Host-memory conveniences for callers without a device-side collective (tests, the CLI):
 * copy this context's shard out (volym_shard_bytes() bytes, padding zeroed) / assemble from
 * world shards held in host memory. */
int volym_read_shard(volym_ctx* ctx, uint8_t* out);
int volym_assemble_host(volym_ctx* ctx, const uint8_t* gathered_host);

/* --- pick (new; the reference has none: its GUI has sliders only) --------------------------------------------------- */
/* Segment, texel and depth under a pixel, by the rule the picture was made by.  For pixel (gx, gy) of the W x H frame take the
 * ray of the last volym_update (camera and parameters) and march it exactly as wgsl:243-326 does through the scene as it
 * stands, crop box and hidden segments included: the same positions, step state machine, threshold test, look-ahead suppression
 * and alpha chain (w = (1 - alpha) * a; alpha += w, f32, in that order).  A composited sample is an iteration that reaches
 * wgsl:313.  The pick is the first composited sample after whose compositing alpha >= alpha_min; the march ends there.  So
 * alpha_min == 0 picks the first composited sample whatever its opacity; in first-hit mode (use_opacity == 0 without importance
 * colouring) alpha becomes 1 at the first composited sample, which is then the pick for every valid alpha_min; importance
 * colouring follows the same rule with its own alpha source.  A ray that leaves the loop without a pick has none.
 * Valid: 0 <= alpha_min <= 0.95 (the loop's own exit); NaN or anything else is VOLYM_E_INVALID. */
struct volym_pick {
    float    t;          /* ray parameter of the picked sample (pos = eye + d*t); -1 unless status == 2 */
    uint16_t x, y, z;    /* its nearest texel, clamp(floor(pos*n), 0, n-1), in the volume as volym_set_volume received it
                            (the coordinates volym_set_crop_box takes) */
    uint8_t  label;      /* label byte of that texel; 0 when has_labels == 0 */
    uint8_t  density;    /* density byte of that texel as the march sees it */
    uint8_t  status;     /* 0 = the ray misses the cube, 1 = hits it, nothing picked, 2 = picked */
    uint8_t  alpha8;     /* unorm8 of alpha after the picked sample; status 1: the ray's final alpha; status 0: 255 */
    uint8_t  has_labels; /* 1 = labels with the volume's dimensions are on the device */
    uint8_t  reserved;   /* 0 */
};                       /* 16 bytes; records of status 0 or 1 have x = y = z = label = density = 0 */
/* The call volym_pick below shares the record's name, and C keeps typedef names and functions in one name space: the record is
 * `struct volym_pick` (a tag, which may share it), or volym_pick_record for short. */
typedef struct volym_pick volym_pick_record;
#if defined(__cplusplus)
static_assert(sizeof(struct volym_pick) == 16, "volym_pick is 16 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(struct volym_pick) == 16, "volym_pick is 16 bytes");
#endif
/* Enqueue only: one pick march of the rect {x0, y0, w, h} (NULL = the whole frame) goes behind what is already enqueued, into a
 * device buffer the context owns: w*h records, row-major within the rect.  The buffer grows to the largest rect asked for so far;
 * the call blocks only when it has to grow, as volym_blit does for its target.  An empty rect, or one not inside the frame, is
 * VOLYM_E_INVALID; a call without volume, importances, transfer function or a volym_update is VOLYM_E_STATE.
 *   A pick pass only reads the scene and writes no frame buffer: a frame enqueued before or after it is byte for byte the frame
 * without it.  With VOLYM_OPT_FRAMES_IN_FLIGHT = 2 it runs on the first slot alone, like volym_stats_pass; with a caller's stream
 * (volym_set_stream) it goes on that stream.  On a sharded context it ignores the shard: any pixel of the W x H frame may be
 * picked, since every rank holds the whole volume (the native multi-GPU loop has no forward for it).
 *   It works with uploaded importances, with labels + table, or with no labels at all (has_labels = 0); labels whose dimensions
 * differ from the volume's count as absent.  The labels may sit in a different device layout than the volume: there is one label
 * fetch per ray, and it takes the labels' own layout.  Cost: a subset of a frame's work per ray -- no gradient taps, no shading,
 * and the march stops at the pick. */
int volym_pick_pass(volym_ctx* ctx, const uint32_t rect[4], float alpha_min);
/* Blocks; copies the w*h records of the latest pick pass.  VOLYM_E_STATE before any pass. */
int volym_read_picks(volym_ctx* ctx, struct volym_pick* out);
/* The device buffer of the latest pick pass (for a highlight or outline pass on the same stream), or NULL before any.  A later
 * pass with a larger rect may move it. */
void* volym_pick_device_ptr(volym_ctx* ctx);
/* A pick pass over the one pixel (x, y) plus the read.  Blocks. */
int volym_pick(volym_ctx* ctx, uint32_t x, uint32_t y, float alpha_min, struct volym_pick* out);

/* --- outline (new; the reference has none) ---------------------------------------------------------------------------- */
/* Ring and tint of the selected segments, in screen space, from pick records that are already there: no march.  It reads the
 * frame of the latest volym_compute_pass, a set of pick records and a selection, and writes an annotated W x H rgba8 image; it
 * never changes the scene or the records, nor the frame unless the frame is the target.  While the view stands the records of
 * one whole-frame pick pass stay valid, and hovering over another segment changes only `selected`.
 *   The rule (integers only; scene.outline_frame of the Python package is its host twin, equal in every byte).  rect =
 * {x0, y0, w, h} is the part of the frame the records cover, row-major within it.  A pixel of the frame is SELECTED when it lies
 * inside rect, its record has status == 2 and selected[record.label] != 0; nothing else is (not a pixel outside rect, not a
 * record of status 0 or 1 whose label byte happens to be selected).  has_labels == 0 records carry label 0, so selected[0] then
 * selects every picked pixel.  A pixel is on the RING when it is not selected and some selected pixel q of the frame has
 * max(|px - qx|, |py - qy|) <= radius; pixels beyond the frame do not exist, and a ring pixel may lie outside rect.  With src
 * the frame's texel, ring pixels take col = ring_rgba, selected pixels col = fill_rgba, every other pixel copies src; with
 * A = col[3]:  out[c] = (src[c] * (255 - A) + col[c] * A + 127) / 255 for r, g, b and out[3] = (src[3] * (255 - A) + 255 * A +
 * 127) / 255, integer division.  A = 0 is the identity; A = 255 replaces rgb and makes alpha 255. */
typedef struct volym_outline {
    uint8_t  selected[256];     /* per label value: != 0 selects it */
    uint8_t  ring_rgba[4];
    uint8_t  fill_rgba[4];
    uint32_t radius;            /* 1..8 */
} volym_outline;                /* 268 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_outline) == 268, "volym_outline is 268 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_outline) == 268, "volym_outline is 268 bytes");
#endif
/* Enqueue only: two kernels (records -> a bit plane of the selected pixels; ring and blend) behind the frame and the pick pass.
 *   records_device == NULL and rect == NULL: the records and the rect of the latest volym_pick_pass (VOLYM_E_STATE before any).
 * Otherwise records_device is device memory holding rect[2] * rect[3] records and rect is required; one without the other is
 * VOLYM_E_INVALID.  The records are not checked for staleness: records of an older view or scene outline that older view.
 *   target_rgba8 == NULL: a W x H target the context owns (volym_read_outline, volym_outline_device_ptr).  Otherwise caller
 * device memory of W * H * 4 bytes; it may be the frame buffer itself (a pixel reads only its own frame texel), and the frame
 * then holds the annotated image.
 *   VOLYM_E_INVALID: NULL ctx, NULL o, radius outside 1..8, a rect that is empty or not inside the frame.  VOLYM_E_STATE: before
 * any volym_compute_pass, and on a sharded context (world > 1): its frame buffer holds a picture only on the root after
 * assembly, and the native multi-GPU loop has no forward for this call.
 *   No allocation and no synchronisation, except on first use: the first pass of a context allocates the bit plane (about 1 MB
 * at 3840 x 2160), the first pass into the context's own target that target; that is the one blocking path, as with volym_blit.
 *   Streams: the pass goes on the first slot's stream, where the pick passes go (a caller's stream when one is set).  With
 * VOLYM_OPT_FRAMES_IN_FLIGHT = 2 events order it, without a host wait: it starts behind the frame it reads and behind the pick
 * pass, and neither a later compute pass into that frame buffer nor a later pick pass into those records starts before it ends. */
int   volym_outline_pass(volym_ctx* ctx, const volym_outline* o, const void* records_device, const uint32_t rect[4], void* target_rgba8);
/* Blocks; W * H * 4 bytes of the context's own target.  VOLYM_E_STATE before any pass into it. */
int   volym_read_outline(volym_ctx* ctx, uint8_t* out);
/* The context's own target after the latest pass into it, NULL before any. */
void* volym_outline_device_ptr(volym_ctx* ctx);

/* --- slice (new; the reference has none) ------------------------------------------------------------------------------ */
/* A plane through the volume that shows the bytes of the scene themselves, with the segments as a colour overlay and the texels
 * the cuts remove marked: the view beside the 3-D picture.  It reads only the bytes of the scene and writes only its target.
 *   The rule (integers only; scene.slice_frame of the Python package is its host twin, equal in every byte).  A slice is an affine
 * map from output pixels to 16.16 fixed-point texel coordinates, the texel coordinates volym_set_crop_box, volym_set_clip_plane
 * and the pick records use; texel x covers [x, x + 1), so its centre is (x << 16) + 0x8000.  For output pixel (i, j):
 * p[a] = origin[a] + i * du[a] + j * dv[a] over the integers, t[a] = floor(p[a] / 65536) (an arithmetic shift).  The pixel is INSIDE
 * iff 0 <= t[a] < n[a] on every axis; nothing is clamped, and an outside pixel is `background`, unchanged.  A slice is VALID only
 * if its four corner positions (i = 0 | width - 1, j = 0 | height - 1), over the integers, have every component in [-2^30, 2^30);
 * p is affine, so every pixel of a valid slice is in that range as well.
 *   An inside pixel is composed in this order.  (1) base, from byte b of texel t: DENSITY (b, b, b, 255) with b the density; TF the
 * r, g, b of texel (b * tf_n) >> 8 of the table volym_set_transfer_function received (its RGBA8 bytes, no filtering) with alpha
 * 255, b the density; IMPORTANCE (m, m, m, 255) with m the importance byte as the march reads it.  The density is the scene's as
 * it stands (box, plane and mask applied); with UNCUT it is the uncut copy when the context holds one (from the first cut on),
 * else the same bytes.  IMPORTANCE with UNCUT is invalid: the importances' uncut source is not one buffer.  (2) LABELS: with
 * l = label(t) and col = palette[l], col is blended over the base with A = col[3] by the outline's formula (at volym_outline);
 * A = 0 leaves the base.  (3) MARK_CUT: cut_rgba is blended, by the same formula, over every texel the context's current cut
 * state removes: a texel outside the crop box, or with clip_n . t > clip_d under a plane, or with a hidden label while labels of
 * the volume's dimensions are on the device.  The predicate decides, not the bytes: a removed texel needs no non-zero byte. */
enum { VOLYM_SLICE_DENSITY = 0, VOLYM_SLICE_TF = 1, VOLYM_SLICE_IMPORTANCE = 2 };          /* mode */
enum { VOLYM_SLICE_UNCUT = 1, VOLYM_SLICE_LABELS = 2, VOLYM_SLICE_MARK_CUT = 4 };          /* flags */
typedef struct volym_slice {
    int32_t  origin[3];         /* 16.16: position of output pixel (0, 0) */
    int32_t  du[3], dv[3];      /* 16.16: step per pixel to the right / per row down */
    uint32_t width, height;     /* 1..8192 each */
    uint32_t mode, flags;
    uint8_t  background[4];     /* pixels whose texel lies outside the volume */
    uint8_t  cut_rgba[4];       /* MARK_CUT */
    uint8_t  palette[256][4];   /* LABELS: colour per label value, alpha = strength */
} volym_slice;                  /* 1084 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_slice) == 1084, "volym_slice is 1084 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_slice) == 1084, "volym_slice is 1084 bytes");
#endif
/* Enqueue only: one kernel on the first slot's stream, where the pick passes go (a caller's stream when one is set).  The output
 * is width * height * 4 bytes, row-major.  target_rgba8 == NULL: a target the context owns (volym_read_slice,
 * volym_slice_device_ptr); it grows to the largest slice asked for so far, and the call blocks only when it has to grow, as
 * volym_pick_pass does for its records.  Apart from that growth there is no allocation, no synchronisation and no copy: palette
 * and transfer function travel with the launch as kernel arguments.
 *   It needs no volym_update and no frame: it reads only the bytes of the scene, which only blocking set-up calls change, and
 * those idle every slot's stream first.  So with VOLYM_OPT_FRAMES_IN_FLIGHT = 2 it needs no events, and a frame enqueued before
 * or after it is byte for byte the frame without it.  It works on a sharded context, since every rank holds the whole volume; the
 * native multi-GPU loop has no forward for it.  The labels may sit in a different device layout than the volume.
 *   VOLYM_E_INVALID: NULL ctx or slice, an unknown mode or flag bit, IMPORTANCE with UNCUT, a size outside 1..8192, an invalid
 * corner (volym_slice_check).  VOLYM_E_STATE: no volume; LABELS without labels of the volume's dimensions on the device;
 * IMPORTANCE without importances of the volume's dimensions; TF without a transfer function. */
int   volym_slice_pass(volym_ctx* ctx, const volym_slice* slice, void* target_rgba8);
/* Blocks; width * height * 4 bytes of the latest pass into the context's own target.  VOLYM_E_STATE before any such pass. */
int   volym_read_slice(volym_ctx* ctx, uint8_t* out);
/* The context's own target after the latest pass into it, NULL before any.  A later, larger slice may move it. */
void* volym_slice_device_ptr(volym_ctx* ctx);
/* The validity rules above, without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, an unknown mode or flag bit, IMPORTANCE
 * with UNCUT, a size outside 1..8192 or a corner outside [-2^30, 2^30).  Pure host arithmetic. */
int volym_slice_check(const volym_slice* slice);
/* Geometry and size of the slice normal to `axis` (0 = x, 1 = y, 2 = z) through texel `index` of a dims[0] x dims[1] x dims[2]
 * volume: one texel per pixel, through texel centres.  z: u = +x, v = +y.  y: u = +x, v = +z.  x: u = +y, v = +z.  It writes
 * origin, du, dv, width and height and leaves mode, flags and colours alone.  VOLYM_E_INVALID for NULL, an axis outside 0..2,
 * index >= dims[axis], an in-plane dimension outside 1..8192 or an index of 16384 or more (its centre lies beyond 2^30).  Pure
 * host arithmetic. */
int volym_slice_axis(int axis, uint32_t index, const uint32_t dims[3], volym_slice* out);
/* The map itself, for click-on-slice: the texel t of output pixel (i, j), inside the volume or not.  VOLYM_E_INVALID for NULL
 * or a pixel outside width x height.  Pure host arithmetic. */
int volym_slice_texel(const volym_slice* slice, uint32_t i, uint32_t j, int32_t t[3]);

/* --- projection (new; the reference has none) ------------------------------------------------------------------------- */
/* Maximum and mean intensity along the view rays: the brightest sample of every ray (where it is, what segment it lies in) and
 * the mean of all its samples ("X-ray").  It reads the bytes of the scene as they stand -- box, plane and mask are in them -- and
 * writes only its records and its image.
 *   The rule (integers wherever something is decided; scene.project_frame of the Python package is its host twin, equal in every
 * byte).  Pixel (gx, gy) of the W x H frame has the ray of the last volym_update: o, d, t_entry, t_exit, hit (wgsl:221-241).  With
 * `step` from the call, sample k = 0, 1, 2, ... lies at t_k = t_entry + (float)k * step -- f32, one multiply, one add, not fused --
 * and exists while t_k < t_exit; t_k does not decrease with k, so the samples are a prefix and n_samples is their count (at least
 * 1 on a hit ray, at most 65535: the path through the cube is at most sqrt(3)).  Positions are not accumulated: a sample depends on
 * k alone.  Sample k reads the density byte b_k of texel clamp(floor(pos * n), 0, n - 1), pos = o + d * t_k: the march's nearest
 * fetch, whatever filter the volume was given.  max is the largest b_k and k* the SMALLEST k that attains it: the running maximum
 * starts at 0 and only a strictly greater byte replaces it, so a ray of zeros has max 0 and no position.  mean =
 * (2 * sum + n_samples) / (2 * n_samples) over the integers, sum the sum of all b_k.  A record holds both, whatever the mode.
 *   The image: a miss is `background`; otherwise v = max (MAX) or mean (MEAN) and the base is (v, v, v, 255), or with TF the r, g,
 * b of texel (v * tf_n) >> 8 of the table volym_set_transfer_function received with alpha 255 (the slice pass's rule); with LABELS
 * (MAX only) and status 2, palette[label] is blended over the base by the outline's formula (at volym_outline). */
enum { VOLYM_PROJECT_MAX = 0, VOLYM_PROJECT_MEAN = 1 };                                    /* mode */
enum { VOLYM_PROJECT_TF = 1, VOLYM_PROJECT_LABELS = 2, VOLYM_PROJECT_NO_SKIP = 4 };        /* flags */
typedef struct volym_project {
    float    step;              /* distance between samples along the ray, [1e-4, 1]: volym_update's range for the march step */
    uint32_t mode, flags;
    uint8_t  background[4];     /* image: pixels whose ray misses the cube */
    uint8_t  palette[256][4];   /* LABELS: colour per label value, alpha = strength */
} volym_project;                /* 1040 bytes */
struct volym_projection {
    float    t;          /* t_{k*}: ray parameter of the first sample that attains the maximum; -1 when status < 2 */
    uint16_t x, y, z;    /* texel of that sample, the coordinates volym_set_crop_box takes; 0 when status < 2 */
    uint8_t  max;        /* the largest density byte among the ray's samples */
    uint8_t  mean;       /* (2 * sum + n_samples) / (2 * n_samples); 0 on a miss */
    uint8_t  label;      /* label byte of that texel; 0 when status < 2 or without labels of the volume's dimensions on the device */
    uint8_t  status;     /* 0 = the ray misses the cube, 1 = hit with max == 0, 2 = hit with max > 0 */
    uint16_t n_samples;  /* 0 on a miss */
};
#if defined(__cplusplus)
static_assert(sizeof(volym_project) == 1040, "volym_project is 1040 bytes");
static_assert(sizeof(struct volym_projection) == 16, "volym_projection is 16 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_project) == 1040, "volym_project is 1040 bytes");
_Static_assert(sizeof(struct volym_projection) == 16, "volym_projection is 16 bytes");
#endif
/* Enqueue only: one kernel over the rect {x0, y0, w, h} (NULL = the whole frame) on the first slot's stream, where the pick passes
 * go (a caller's stream when one is set); with VOLYM_OPT_FRAMES_IN_FLIGHT = 2 it uses the first slot alone.  It ignores the shard:
 * every rank holds the whole volume.  It only reads the scene and writes no frame buffer: a frame enqueued before or after it is
 * byte for byte the frame without it.
 *   records_device: caller device memory of w * h records, row-major within the rect, or NULL for records the context owns
 * (volym_read_projection, volym_projection_device_ptr); those grow to the largest rect asked for so far, and the call blocks only
 * when they have to grow.  image_rgba8: caller device memory of w * h * 4 bytes, row-major within the rect, or NULL for no image.
 * volym_project_image_pass is the same pass with records and image both in buffers the context owns (volym_read_projection_image,
 * volym_projection_image_device_ptr): two plain calls instead of a sentinel pointer.  Records and image leave the same launch.
 *   By default the march skips samples that cannot change the record: those inside a macro cell (VOLYM_OPT_MACRO_CELLS) whose
 * maximum is 0, which add nothing to the sum and never exceed the running maximum.  A record holds max and mean of the same
 * ray, so a cell whose maximum is merely not above the running maximum still has to be read for the sum.  NO_SKIP reads every
 * sample; both paths give the same records for every ray.
 *   VOLYM_E_INVALID: NULL ctx or volym_project, what volym_project_check refuses, an empty rect or one outside the frame.
 * VOLYM_E_STATE: no volume, no volym_update yet or the volume changed since; LABELS without labels of the volume's dimensions on
 * the device; TF without a transfer function. */
int   volym_project_pass(volym_ctx* ctx, const volym_project* p, const uint32_t rect[4], void* records_device, void* image_rgba8);
int   volym_project_image_pass(volym_ctx* ctx, const volym_project* p, const uint32_t rect[4]);
/* Blocks; the w * h records of the latest pass into the context's own records.  VOLYM_E_STATE before any such pass. */
int   volym_read_projection(volym_ctx* ctx, struct volym_projection* out);
/* Blocks; w * h * 4 bytes of the latest volym_project_image_pass.  VOLYM_E_STATE before any. */
int   volym_read_projection_image(volym_ctx* ctx, uint8_t* out);
/* The context's own buffers after the latest pass into them, NULL before any.  A later, larger rect may move them. */
void* volym_projection_device_ptr(volym_ctx* ctx);
void* volym_projection_image_device_ptr(volym_ctx* ctx);
/* Rect size {w, h} of the latest pass into the context's own records / own image, {0, 0} before any: what the two reads copy,
 * so that a caller sizes its buffer from the context and not from a note of its own. */
int   volym_projection_size(volym_ctx* ctx, uint32_t size[2]);
int   volym_projection_image_size(volym_ctx* ctx, uint32_t size[2]);
/* A MAX pass without flags over the one pixel (x, y) plus the read.  Blocks.  The record goes through a 16-byte buffer of the
 * call's own: the context's own records, their size and volym_projection_device_ptr stay what the latest pass made them. */
int   volym_project_at(volym_ctx* ctx, uint32_t x, uint32_t y, float step, struct volym_projection* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a step that is not finite or outside [1e-4, 1], an unknown
 * mode or flag bit, LABELS with MEAN.  Pure host arithmetic. */
int   volym_project_check(const volym_project* p);
/* The count rule: *n = the number of k >= 0 with t_entry + (float)k * step < t_exit in f32 (0 when t_exit <= t_entry).
 * VOLYM_E_INVALID for NULL, a step outside [1e-4, 1] or a t that is not finite or outside [0, 128] (up to there t_k grows with
 * every k).  Pure host arithmetic; the kernel's count agrees with it on every ray. */
int   volym_project_samples(float t_entry, float t_exit, float step, uint32_t* n);

/* --- measuring segments (new; the reference has none) ----------------------------------------------------------------- */
/* How large a segment is, where it lies and how its density is distributed, and the density histogram of the visible scene: one
 * pass over the bytes of the scene that writes one 36 KB result.  It reads the bytes as they stand and writes nothing else.
 *   The rule (integers only; scene.measure_volume of the Python package is its host twin, equal in every byte).  A request is a box
 * [lo, hi) of texels (box = {x0, y0, z0, x1, y1, z1}, the coordinates volym_set_crop_box takes), flags, and a table group[256] that
 * maps a label value to one of VOLYM_MEASURE_GROUPS histogram groups or to VOLYM_MEASURE_NO_GROUP.  Texel t of the box is IN iff it
 * lies inside the crop box, is kept by the clip plane (n . t <= d) and its label is not hidden; with UNCUT every texel of the box is
 * in.  Its density byte is that of the scene as it stands; with UNCUT that of the uncut copy when the context holds one (from the
 * first cut on), else the same bytes.  Its label is the byte of the label volume, or 0 for every texel while the context holds no
 * labels of the volume's dimensions (the mask term then removes nothing).
 *   seg[l] sums over the in-texels with label l: their number, the density byte, its square and the three texel coordinates, with
 * the smallest and largest byte and the texel box {x0, y0, z0, x1, y1, z1}, hi inclusive (the convention of the label boxes).  A
 * label without an in-texel has the empty record: zeros, min = 255, max = 0, box = {INT32_MAX x 3, -1 x 3}.  hist[g][b] is the number
 * of in-texels with density byte b whose label maps to group g.  Mean, deviation, centroid and physical volume are floats the host
 * derives from the record (scene.segment_summary); the device computes none of them. */
enum { VOLYM_MEASURE_UNCUT = 1 };                                                            /* flags */
#define VOLYM_MEASURE_GROUPS 8
#define VOLYM_MEASURE_NO_GROUP 255
typedef struct volym_measure {
    uint32_t box[6];            /* {x0, y0, z0, x1, y1, z1}: lo inclusive, hi exclusive, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint8_t  group[256];        /* label value -> histogram group 0..7, or VOLYM_MEASURE_NO_GROUP */
} volym_measure;                /* 284 bytes */
struct volym_segment_stats {
    uint64_t count, sum, sum_sq;        /* in-texels, their density bytes, the squares of those */
    uint64_t sum_x, sum_y, sum_z;       /* their texel coordinates */
    int32_t  box[6];                    /* {x0, y0, z0, x1, y1, z1}, hi inclusive */
    uint32_t min, max;                  /* smallest and largest density byte */
};                                      /* 80 bytes */
struct volym_measurement {
    struct volym_segment_stats seg[256];
    uint64_t hist[VOLYM_MEASURE_GROUPS][256];
};                                      /* 36864 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_measure) == 284, "volym_measure is 284 bytes");
static_assert(sizeof(struct volym_segment_stats) == 80, "volym_segment_stats is 80 bytes");
static_assert(sizeof(struct volym_measurement) == 36864, "volym_measurement is 36864 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_measure) == 284, "volym_measure is 284 bytes");
_Static_assert(sizeof(struct volym_segment_stats) == 80, "volym_segment_stats is 80 bytes");
_Static_assert(sizeof(struct volym_measurement) == 36864, "volym_measurement is 36864 bytes");
#endif
/* Enqueue only, on the first slot's stream, where pick, slice and projection passes go (a caller's stream when one is set): one small
 * kernel that puts the context's own result back to 256 empty records and zeroed histograms, then the pass.  m == NULL: the whole
 * volume, every label in group 0, no flags.  The one blocking path is the first allocation of the result.  It needs a volume, but no
 * volym_update, no frame and no transfer function; it ignores the shard (every rank holds the whole volume) and writes no frame
 * buffer.  The bytes of the scene change only in blocking set-up calls that idle every stream, so with
 * VOLYM_OPT_FRAMES_IN_FLIGHT = 2 it needs no events, and a frame enqueued before or after it is byte for byte the frame without it.
 * The sums are integers, so the result does not depend on the order in which workgroups arrive.
 *   VOLYM_E_INVALID: NULL ctx, what volym_measure_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions held
 * in the other device layout than the volume (the walk reads label chunk k beside density chunk k; volym_set_segment_visibility
 * refuses the same). */
int   volym_measure_pass(volym_ctx* ctx, const volym_measure* m);
/* Blocks; the result of the latest pass.  VOLYM_E_STATE before any pass, and after volym_set_volume until the next one. */
int   volym_read_measure(volym_ctx* ctx, struct volym_measurement* out);
/* The context's own result (a struct volym_measurement in device memory) after a pass, NULL before any. */
void* volym_measure_device_ptr(volym_ctx* ctx);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, a group entry that is neither below VOLYM_MEASURE_GROUPS nor VOLYM_MEASURE_NO_GROUP.  An empty box is valid: it yields 256
 * empty records.  Pure host arithmetic. */
int   volym_measure_check(const volym_measure* m, const uint32_t dims[3]);

/* --- segment surfaces (new; the reference has none) -------------------------------------------------------------------- */
/* The boundary faces of a segment, or of the isosurface density >= threshold: how many there are per label and direction (the
 * surface area), the divergence sums that give the enclosed texel count back, and the faces themselves as one list a mesh is
 * written from.  Two read-only passes over the bytes of the scene as they stand; nothing else is written.
 *   The rule (integers only; scene.surface_volume of the Python package is its host twin, equal in every byte).  A request is a box
 * [lo, hi) of texels (volym_measure's conventions), flags, min_byte in 1..255 and a table select[256].  Texel t is SOLID iff it
 * lies in the request's box, its density byte is >= min_byte and select[label(t)] != 0.  The byte is that of the scene as it
 * stands; with UNCUT that of the uncut copy when the context holds one (from the first cut on), else the same bytes.  The label is
 * the byte of the label volume, or 0 for every texel while the context holds no labels of the volume's dimensions.
 *   The cuts are in the predicate for free.  The scene keeps byte(t) = (t inside the crop box, kept by the clip plane, label not
 * hidden) ? uncut byte : 0, and min_byte >= 1: a texel a cut removes has byte 0 and is never solid, so the pass evaluates no box,
 * plane or mask arithmetic of its own.  The same holds for a texel of a selected label whose own byte is below min_byte: it is not
 * solid, and the surface runs between it and its neighbours of the same label.
 *   A FACE is a pair (t, dir) with t solid and its neighbour in direction dir not solid; dir 0..5 = -x, +x, -y, +y, -z, +z.  A
 * neighbour outside the request's box, or outside the volume, is not solid, whatever its bytes: the surface of a box that cuts
 * through a segment is closed along the box.
 *   The summary: faces[l][dir] counts the faces of texels with label l; total counts all; for axis a, pos[l][a] is the sum of
 * t[a] + 1 over the +a faces of label l and neg[l][a] the sum of t[a] over its -a faces, both stored as they are.  Summed over
 * the labels, pos - neg is the number of solid texels, on every axis (the divergence theorem on unit cubes: every run of solid
 * texels along a starts with a -a face at t[a] and ends with a +a face at t[a] + 1).  Two solid texels of different labels have
 * no face between them, so per label the identity holds where the label's own surface is closed: always with that label selected
 * alone, and then, with min_byte = 1 and no byte of the segment 0 inside the cuts, pos[l][a] - neg[l][a] is
 * volym_measurement.seg[l].count.  Areas in physical units, the enclosed volume and sphericity are floats the host derives
 * (scene.surface_summary).
 *   The face list: one 8-byte record per face, in ONE order whatever the device layout: ascending (z, y, x, dir).  The same request
 * on the same scene gives the same bytes, every time. */
enum { VOLYM_SURFACE_UNCUT = 1 };                                                            /* flags */
#define VOLYM_SURFACE_SCAN_ROWS 256     /* rows of the request's box (fixed y, z) that one workgroup of the offset scan covers */
typedef struct volym_surface {
    uint32_t box[6];            /* {x0, y0, z0, x1, y1, z1}: lo inclusive, hi exclusive, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint32_t min_byte;          /* 1..255 */
    uint8_t  select[256];       /* label value -> != 0: its texels can be solid */
} volym_surface;                /* 288 bytes */
struct volym_surface_summary {
    uint64_t faces[256][6];     /* per label of the solid texel and direction */
    uint64_t total;
    uint64_t pos[256][3];       /* sum of t[a] + 1 over the +a faces */
    uint64_t neg[256][3];       /* sum of t[a] over the -a faces */
};                              /* 24584 bytes */
struct volym_surface_face {
    uint16_t x, y, z;           /* the solid texel, the coordinates volym_set_crop_box takes */
    uint8_t  dir;               /* 0..5 = -x, +x, -y, +y, -z, +z: the side of the texel the face is on */
    uint8_t  label;             /* label byte of the texel; 0 without labels of the volume's dimensions on the device */
};                              /* 8 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_surface) == 288, "volym_surface is 288 bytes");
static_assert(sizeof(struct volym_surface_summary) == 24584, "volym_surface_summary is 24584 bytes");
static_assert(sizeof(struct volym_surface_face) == 8, "volym_surface_face is 8 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_surface) == 288, "volym_surface is 288 bytes");
_Static_assert(sizeof(struct volym_surface_summary) == 24584, "volym_surface_summary is 24584 bytes");
_Static_assert(sizeof(struct volym_surface_face) == 8, "volym_surface_face is 8 bytes");
#endif
/* Enqueue only, on the first slot's stream, where pick, slice, projection and measure passes go (a caller's stream when one is
 * set): a kernel that zeroes the context's own summary, the count pass (the summary, and the face count of every row of the
 * request's box: fixed y, z) and the scan that turns the counts into the offset of every row's first face.  s == NULL: the whole
 * volume, min_byte 1, every label selected, no flags.  The one blocking path is the first allocation of the summary and the first
 * allocation, or a growth, of the row-offset array (4 bytes per row of the largest box asked for so far).  It needs a volume, but
 * no volym_update, no frame and no transfer function; it ignores the shard (every rank holds the whole volume), writes no frame
 * buffer and needs no events with VOLYM_OPT_FRAMES_IN_FLIGHT = 2: a frame enqueued before or after it is byte for byte the frame
 * without it.  An empty box launches only the zeroing kernel.
 *   VOLYM_E_INVALID: NULL ctx, what volym_surface_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions held
 * in the other device layout than the volume (as volym_measure_pass). */
int   volym_surface_pass(volym_ctx* ctx, const volym_surface* s);
/* Blocks; the summary of the latest pass.  VOLYM_E_STATE before any pass, and after volym_set_volume until the next one. */
int   volym_read_surface(volym_ctx* ctx, struct volym_surface_summary* out);
/* The context's own summary (a struct volym_surface_summary in device memory) after a pass, NULL before any. */
void* volym_surface_device_ptr(volym_ctx* ctx);
/* The emit pass of the latest surface pass: its faces, in canonical order, into target_device (device memory of capacity_faces
 * records, 8-byte aligned), or with target_device == NULL into a buffer the context owns and sizes to the total
 * (volym_read_surface_faces; capacity_faces is then ignored).  The first call after a surface pass blocks to learn the total; the
 * context's own buffer blocks when it has to grow.  The kernel itself is enqueued on the first slot's stream.
 *   VOLYM_E_INVALID: NULL ctx; a caller's capacity_faces below the total, or a misaligned target; a total above UINT32_MAX (the row
 * offsets are 32-bit) -- pure host arithmetic on the summary, nothing is written.  VOLYM_E_STATE: before any surface pass, and
 * after volym_set_volume or any set-up call that changed the bytes the pass read (volym_set_crop_box, volym_set_clip_plane,
 * volym_set_segment_visibility with a change, volym_set_labels, volym_set_importances, which drops the labels): the offsets no
 * longer describe the scene.  volym_set_segment_importances rewrites the importances alone and leaves a surface pass valid. */
int   volym_surface_faces_pass(volym_ctx* ctx, void* target_device, uint64_t capacity_faces);
/* Blocks; copies the faces of the latest volym_surface_faces_pass into the context's own buffer (`total` records of that pass).
 * VOLYM_E_STATE before any such pass; VOLYM_E_INVALID for NULL or capacity_faces below that count. */
int   volym_read_surface_faces(volym_ctx* ctx, struct volym_surface_face* out, uint64_t capacity_faces);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, min_byte outside 1..255.  An empty box is valid: a zero summary and no faces.  Pure host arithmetic. */
int   volym_surface_check(const volym_surface* s, const uint32_t dims[3]);

/* --- connected components (new; the reference has none) ------------------------------------------------------------------ */
/* Is a segment one piece?  The 6-connected components of the solid texels of a request: how many there are, one record per
 * component and one id per texel of the request's box.  A read-only pass over the bytes of the scene as they stand: it writes no
 * label and no scene byte.
 *   The rule (integers only; scene.components_volume of the Python package is its host twin, equal in every byte).  box, flags,
 * min_byte and select are volym_surface's, and SOLID is the surface pass's predicate: the texel lies in the request's box, its
 * density byte is >= min_byte and select[label] != 0; UNCUT reads the uncut copy as it does there; the label is 0 everywhere while
 * the context holds no labels of the volume's dimensions; the cuts are in the bytes for free.  Two solid texels are LINKED iff they
 * differ by 1 on exactly one axis (the adjacency of the surface pass's faces) and, with SPLIT_LABELS, their label bytes are equal.
 * A COMPONENT is a class of the transitive closure of "linked"; links never cross the request's box.
 *   Canonical numbering: a component's ROOT is its first texel in ascending (z, y, x); components are numbered 0, 1, 2, ... in
 * ascending order of their roots.  The same request on the same scene gives the same bytes in either device layout, every time.
 *   The id volume: one uint32_t per texel of the box, box-linear with x fastest, (x - x0) + w * ((y - y0) + h * (z - z0)) -- never
 * the device layout: the component's number, or VOLYM_COMPONENT_NONE for a texel that is not solid.  It lives in a buffer the context
 * owns, which grows to the largest box asked for so far (4 bytes per texel: 4 GiB for 1024^3); a box of more than 2^31 - 2 texels is
 * refused.  The table: record k describes component k, for k < max_components; components numbered from max_components on keep
 * their ids in the id volume and are counted in the summary, but have no record, and nothing is written past that capacity. */
enum { VOLYM_COMPONENTS_UNCUT = 1, VOLYM_COMPONENTS_SPLIT_LABELS = 2 };                        /* flags */
#define VOLYM_COMPONENTS_DEFAULT_MAX 65536u         /* max_components == 0 */
#define VOLYM_COMPONENTS_TABLE_MAX (1u << 24)       /* largest max_components */
#define VOLYM_COMPONENTS_BOX_MAX 0x7ffffffeu        /* 2^31 - 2: most texels of a request's box */
#define VOLYM_COMPONENT_NONE 0xffffffffu            /* id of a texel that is not solid */
typedef struct volym_components {
    uint32_t box[6];            /* {x0, y0, z0, x1, y1, z1}: lo inclusive, hi exclusive, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint32_t min_byte;          /* 1..255 */
    uint8_t  select[256];       /* label value -> != 0: its texels can be solid */
    uint32_t max_components;    /* table records to keep; 0: VOLYM_COMPONENTS_DEFAULT_MAX; at most VOLYM_COMPONENTS_TABLE_MAX */
} volym_components;             /* 292 bytes */
struct volym_components_summary {
    uint64_t n_components;
    uint64_t n_solid;
    uint64_t recorded;          /* min(n_components, max_components): the records of the table */
    uint64_t per_label[256];    /* the components whose root has that label */
};                              /* 2072 bytes */
struct volym_component {
    uint16_t x, y, z;           /* the root texel, the coordinates volym_set_crop_box takes */
    uint8_t  label;             /* the root's label byte; 0 without labels of the volume's dimensions on the device */
    uint8_t  flags;             /* bit 0: some texel lies on a face of the request's box: the piece may continue outside */
    uint32_t count;             /* texels (at most 2^31 - 2) */
    uint16_t box[6];            /* {x0, y0, z0, x1, y1, z1} of its texels, hi INCLUSIVE (as volym_label_counts' boxes) */
};                              /* 24 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_components) == 292, "volym_components is 292 bytes");
static_assert(sizeof(struct volym_components_summary) == 2072, "volym_components_summary is 2072 bytes");
static_assert(sizeof(struct volym_component) == 24, "volym_component is 24 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_components) == 292, "volym_components is 292 bytes");
_Static_assert(sizeof(struct volym_components_summary) == 2072, "volym_components_summary is 2072 bytes");
_Static_assert(sizeof(struct volym_component) == 24, "volym_component is 24 bytes");
#endif
/* Enqueue only, on the first slot's stream, where pick, measure and surface passes go: the kernel that zeroes the summary, the row
 * runs, the merge (a lock-free union-find over the texels of the box, in the id volume itself), the flatten, the numbering with its
 * scan, the relabel that accumulates the records, and their packing.  c == NULL: the whole volume, min_byte 1, every label, no
 * flags, the default capacity.  The one blocking path is the first allocation, or a growth, of its buffers.  It needs a volume, but
 * no volym_update, no frame and no transfer function; it ignores the shard, writes no frame buffer and needs no events with
 * VOLYM_OPT_FRAMES_IN_FLIGHT = 2: a frame enqueued before or after it is byte for byte the frame without it.  An empty box launches
 * only the zeroing kernel.  The results are a snapshot: the reads below stay valid after later edits of the scene.
 *   VOLYM_E_INVALID: NULL ctx, what volym_components_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions
 * held in the other device layout than the volume (as volym_surface_pass). */
int   volym_components_pass(volym_ctx* ctx, const volym_components* c);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis or of more than
 * VOLYM_COMPONENTS_BOX_MAX texels, an unknown flag bit, min_byte outside 1..255, max_components above VOLYM_COMPONENTS_TABLE_MAX.
 * An empty box is valid: a zero summary, no records, no ids.  Pure host arithmetic. */
int   volym_components_check(const volym_components* c, const uint32_t dims[3]);
/* The reads block.  All: VOLYM_E_STATE before any pass, and after volym_set_volume until the next one; VOLYM_E_INVALID for a NULL
 * ctx or output.
 *   volym_read_components: the summary of the latest pass.
 *   volym_read_component_table: its `recorded` records; VOLYM_E_INVALID for a capacity below that.
 *   volym_read_component_ids: the ids of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi, inside the pass's box; NULL:
 * the pass's whole box), box-linear in the sub-box; VOLYM_E_INVALID for a sub-box that reaches outside the pass's box.
 *   volym_component_of: the id of one texel (4 bytes are copied); VOLYM_E_INVALID for a texel outside the pass's box. */
int   volym_read_components(volym_ctx* ctx, struct volym_components_summary* out);
int   volym_read_component_table(volym_ctx* ctx, struct volym_component* out, uint64_t capacity);
int   volym_read_component_ids(volym_ctx* ctx, const uint32_t sub[6], uint32_t* out);
int   volym_component_of(volym_ctx* ctx, uint32_t x, uint32_t y, uint32_t z, uint32_t* id);
/* The context's own results in device memory after a pass (NULL before any, and after volym_set_volume): the summary (a struct
 * volym_components_summary), the id volume of the latest pass's box, the table (struct volym_component records). */
void* volym_components_device_ptr(volym_ctx* ctx);
void* volym_component_ids_device_ptr(volym_ctx* ctx);
void* volym_component_table_device_ptr(volym_ctx* ctx);

/* --- distance maps (new; the reference has none) ------------------------------------------------------------------ */
/* Margins, thickness and clearance: the exact squared Euclidean distance from every texel of a box to the nearest texel of a set.
 * A read-only pass over the bytes of the scene as they stand: it writes no scene byte.
 *   The rule (integers only; scene.distance_volume of the Python package is its host twin, equal in every byte).  box, flags,
 * min_byte and select are volym_surface's.  PRESENT: the texel lies in the box and its density byte is >= min_byte.  SOLID: PRESENT
 * and select[label] != 0, the surface pass's predicate (UNCUT reads the uncut copy; the label is 0 everywhere while the context holds
 * no labels of the volume's dimensions).  d2(p, q) = sum over the axes of weight[a] * (p[a] - q[a])^2: anisotropic spacing as
 * integer weights, 0.5 x 0.5 x 2.5 mm being (1, 1, 25) in units of 0.5 mm.  With 4096 texels per axis d2 <= 3 * 64 * 4095^2 < 2^32.
 *   The map: one uint32_t per texel of the box, box-linear with x fastest like the component ids, never the device layout.
 * Without INSIDE, D(t) = min d2(t, s) over the solid texels s of the box: 0 on a solid texel, VOLYM_DISTANCE_NONE everywhere when
 * the box has none.  With INSIDE, D(t) = min d2(t, u) over the texels u that are not solid, every texel outside the box counting
 * as not solid (the surface pass's convention: a piece the box cuts is closed along the box); the nearest outside texel is the
 * axis-aligned one, so D(t) is the minimum of the in-box value and weight[a] * (t[a] - lo[a] + 1)^2 and weight[a] * (hi[a] - t[a])^2
 * on each axis; 0 on a texel that is not solid, never NONE.
 *   Ties (max_at, near_at) go to the first texel in ascending (z, y, x): the same request on the same scene gives the same bytes
 * in either device layout, every time. */
enum { VOLYM_DISTANCE_UNCUT = 1, VOLYM_DISTANCE_INSIDE = 2 };          /* flags */
#define VOLYM_DISTANCE_WEIGHT_MAX 64u               /* each weight is 1..64 */
#define VOLYM_DISTANCE_BOX_MAX 0x7ffffffeu          /* 2^31 - 2: most texels of a request's box */
#define VOLYM_DISTANCE_NONE 0xffffffffu             /* no seed in the box */
#define VOLYM_DISTANCE_BINS 256
typedef struct volym_distance {
    uint32_t box[6];            /* {x0, y0, z0, x1, y1, z1}: lo inclusive, hi exclusive, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint32_t min_byte;          /* 1..255 */
    uint8_t  select[256];       /* label value -> != 0: its texels can be solid */
    uint32_t weight[3];         /* per axis, 1..VOLYM_DISTANCE_WEIGHT_MAX */
} volym_distance;               /* 300 bytes */
struct volym_distance_summary {
    uint64_t n_solid, n_present;
    uint64_t n_finite;          /* texels of the box with D != NONE */
    uint32_t max_d2;            /* the largest D != NONE; NONE when n_finite == 0 */
    uint32_t max_at[3];         /* the first texel that attains it, volume coordinates; {0, 0, 0} when n_finite == 0 */
    uint32_t near_d2[256];      /* per label byte: the smallest D != NONE over its PRESENT texels, selected or not; NONE: none */
    uint32_t near_at[256][3];   /* ... and the first such texel; {0, 0, 0}: none */
    uint64_t hist[VOLYM_DISTANCE_BINS];   /* texels with D != NONE by min(ceil_sqrt(D), 255): sum over k <= r is the texels with D <= r^2 */
};                              /* 6184 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_distance) == 300, "volym_distance is 300 bytes");
static_assert(sizeof(struct volym_distance_summary) == 6184, "volym_distance_summary is 6184 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_distance) == 300, "volym_distance is 300 bytes");
_Static_assert(sizeof(struct volym_distance_summary) == 6184, "volym_distance_summary is 6184 bytes");
#endif
/* Enqueue only, on the first slot's stream: the kernel that zeroes the summary, the row sweep, the column sweeps along y and z
 * (lower envelopes of parabolas, one lane per column), the finish that applies the INSIDE border and accumulates the summary, and
 * its packing.  d == NULL: the whole volume, min_byte 1, every label, weights 1, no flags.  The one blocking path is the first
 * allocation, or a growth, of its buffers (4 bytes per texel of the box for the map and 8 for the work arrays).  It needs a volume,
 * but no volym_update, no frame and no transfer function; it ignores the shard, writes no frame buffer and needs no events with
 * VOLYM_OPT_FRAMES_IN_FLIGHT = 2.  An empty box launches only the zeroing kernel.  The results are a snapshot: the reads below stay
 * valid after later edits of the scene.
 *   VOLYM_E_INVALID: NULL ctx, what volym_distance_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions held
 * in the other device layout than the volume (as volym_surface_pass). */
int   volym_distance_pass(volym_ctx* ctx, const volym_distance* d);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis or of more than
 * VOLYM_DISTANCE_BOX_MAX texels, an unknown flag bit, min_byte outside 1..255, a weight outside 1..VOLYM_DISTANCE_WEIGHT_MAX.  An
 * empty box is valid.  Pure host arithmetic. */
int   volym_distance_check(const volym_distance* d, const uint32_t dims[3]);
/* The reads block.  All: VOLYM_E_STATE before any pass, and after volym_set_volume until the next one; VOLYM_E_INVALID for a NULL
 * ctx or output.
 *   volym_read_distance: the summary of the latest pass.
 *   volym_read_distance_map: the map of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi, inside the pass's box; NULL:
 * the pass's whole box), box-linear in the sub-box; VOLYM_E_INVALID for a sub-box that reaches outside the pass's box.
 *   volym_distance_at: D of one texel (4 bytes are copied); VOLYM_E_INVALID for a texel outside the pass's box. */
int   volym_read_distance(volym_ctx* ctx, struct volym_distance_summary* out);
int   volym_read_distance_map(volym_ctx* ctx, const uint32_t sub[6], uint32_t* out);
int   volym_distance_at(volym_ctx* ctx, uint32_t x, uint32_t y, uint32_t z, uint32_t* d2);
/* The context's own results in device memory after a pass (NULL before any, and after volym_set_volume): the summary (a struct
 * volym_distance_summary) and the map of the latest pass's box. */
void* volym_distance_device_ptr(volym_ctx* ctx);
void* volym_distance_map_device_ptr(volym_ctx* ctx);

/* --- editing labels (new; the reference has none) ------------------------------------------------------------------ */
/* Acting on what the passes above found: relabel texels on the device by a table, a density window, a piece of the latest
 * components pass and a band of the latest distance map.  The context ends up byte for byte where a context handed the edited labels
 * (volym_set_labels, then the same table, mask, box and plane) would be.
 *   The rule (integers only; scene.relabel_volume of the Python package is its host twin, equal in every byte).  A texel t with label
 * l becomes to[l] iff all of these hold: t lies in box; to[l] != l; its density byte lies in [min_byte, max_byte] -- the scene byte
 * as it stands, with UNCUT the uncut copy as volym_measure_pass reads it; with IDS, its id in the id volume of the latest components
 * pass is not VOLYM_COMPONENT_NONE and lies in [id_lo, id_hi] (with IDS_EXCEPT as well: outside that range); with DISTANCE, its D in
 * the latest distance map is not VOLYM_DISTANCE_NONE and lies in [d2_lo, d2_hi].  Ids and distances are the snapshots they are: a
 * snapshot may be applied again after an edit, without a new pass.  Every texel is decided from the bytes before the edit: the result
 * does not depend on the device layout or on the order of the workgroups.  DRY_RUN fills the result and writes nothing. */
enum { VOLYM_RELABEL_UNCUT = 1, VOLYM_RELABEL_IDS = 2, VOLYM_RELABEL_IDS_EXCEPT = 4, VOLYM_RELABEL_DISTANCE = 8, VOLYM_RELABEL_DRY_RUN = 16 };   /* flags */
typedef struct volym_relabel {
    uint32_t box[6];            /* {x0, y0, z0, x1, y1, z1}: lo inclusive, hi exclusive, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint32_t min_byte, max_byte;   /* 0..255, min <= max: the density window; 0..255 = no window */
    uint8_t  to[256];           /* old label -> new label; to[l] == l: label l is not touched */
    uint32_t id_lo, id_hi;      /* IDS: lo <= hi */
    uint32_t d2_lo, d2_hi;      /* DISTANCE: lo <= hi */
} volym_relabel;                /* 308 bytes */
struct volym_relabel_result {
    uint64_t changed;           /* texels whose label changed (with DRY_RUN: would change) */
    uint64_t left[256];         /* texels that had this label and lost it */
    uint64_t arrived[256];      /* texels that got this label */
    uint32_t box[6];            /* hull of the changed texels, lo inclusive, hi exclusive; all 0 when changed == 0 */
};                              /* 4128 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_relabel) == 308, "volym_relabel is 308 bytes");
static_assert(sizeof(struct volym_relabel_result) == 4128, "volym_relabel_result is 4128 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_relabel) == 308, "volym_relabel is 308 bytes");
_Static_assert(sizeof(struct volym_relabel_result) == 4128, "volym_relabel_result is 4128 bytes");
#endif
/* The edit: a blocking set-up call, like volym_set_segment_visibility (it waits for the frames in flight; the kernel runs on the
 * first slot's stream, behind any components or distance pass).  With changed == 0, or DRY_RUN, nothing else is touched: a surface
 * pass stays valid for volym_surface_faces_pass.  Otherwise the label counts and boxes (volym_label_counts) are those
 * volym_set_labels of the edited labels leaves, density and importances follow under the mask, box and plane, and a surface pass is
 * stale.  out may be NULL.  A failure after the kernel has stored leaves the context asking for volym_set_volume.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_relabel_check refuses, IDS or DISTANCE with a box that reaches outside the box
 * of that pass.  VOLYM_E_STATE: no volume; no labels of the volume's dimensions; labels (or importances of the volume's dimensions)
 * in the other device layout than the volume; IDS or DISTANCE without such a pass since volym_set_volume.
 *   Ids and maps belong to one context: the native multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_edit_labels(volym_ctx* ctx, const volym_relabel* r, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, IDS_EXCEPT without IDS, a window without min_byte <= max_byte <= 255, IDS with id_lo > id_hi, DISTANCE with d2_lo > d2_hi.
 * An empty box is valid: nothing changes.  Pure host arithmetic. */
int   volym_relabel_check(const volym_relabel* r, const uint32_t dims[3]);
/* The labels as they stand, blocking: those of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi <= the labels'
 * dimensions; NULL: the whole label volume), box-linear in the sub-box with x fastest, whatever the device layout.
 * VOLYM_E_STATE: no labels.  VOLYM_E_INVALID: NULL ctx, a sub-box outside the labels, NULL output for a sub-box with texels. */
int   volym_read_labels(volym_ctx* ctx, const uint32_t sub[6], uint8_t* out);

/* --- undo and redo of label edits (new; the reference has none) ---------------------------------------------------- */
/* What an edit destroys is small: the 16-byte label chunks of the device layout in which a byte changed.  While the history is on,
 * every volym_edit_labels and every volym_brush_labels that changes a texel (no DRY_RUN) journals those chunks -- index and the 16 bytes before the edit, 20 bytes
 * per chunk, each chunk once -- from the kernel that stores them, and the journal becomes a step in device memory of its own.  Undo
 * swaps the newest undoable step with the labels; redo swaps the newest undone step back; an edit that records drops the redo steps.
 * scene.LabelHistory of the Python package is the host twin of the bookkeeping, equal in every field of the info.
 *   budget_bytes > 0: keep a history in at most that much device memory.  0: drop the history and free it.  Off in a new context.
 * Changing the budget keeps the steps that still fit: the oldest undoable steps are dropped first, then the redo steps that would be
 * redone last.  An edit journals into a staging area with room for min(items of the request's slab, budget / 20) records; when more
 * chunks change than that, the edit is carried out and returns VOLYM_OK, the whole history (undo and redo steps) is given up, and
 * `lost` counts it: undoing older steps across a gap would be wrong.  The same happens when there is no device memory for the step.
 * After a step that fits, the oldest steps are dropped until used_bytes <= budget_bytes, each adding 1 to dropped_steps.
 *   volym_set_labels, volym_set_volume and volym_set_importances clear the steps (the budget and the two counters stay). */
int   volym_label_history(volym_ctx* ctx, uint64_t budget_bytes);
/* Blocking set-up calls exactly like volym_edit_labels (they wait for the frames in flight and run on the first slot's stream).  The
 * result is computed on the device from the bytes that were swapped: the texels that differ, per label those that lost it and got
 * it, and their hull -- for an undo the edit's result with left and arrived exchanged, for a redo the edit's result.  Afterwards the
 * context is byte for byte where one handed those labels would be, under the box, plane and mask as they stand now (they may have
 * changed since the edit), and a surface pass is stale.  out may be NULL.
 *   VOLYM_E_INVALID: NULL ctx.  VOLYM_E_STATE: the history is off; nothing to undo / redo; the states volym_edit_labels refuses.  A
 * refused call changes nothing.  The native multi-GPU loop has no forward for these calls. */
int   volym_undo_labels(volym_ctx* ctx, struct volym_relabel_result* out);
int   volym_redo_labels(volym_ctx* ctx, struct volym_relabel_result* out);
struct volym_label_history_info {
    uint64_t budget_bytes, used_bytes;      /* used = 20 * records over all kept steps, <= budget */
    uint32_t undo_steps, redo_steps;
    uint64_t next_undo_records, next_redo_records;   /* chunks the next undo / redo would swap; 0: none */
    uint64_t dropped_steps;                 /* steps evicted to stay in the budget, since the history was switched on */
    uint64_t lost;                          /* times the whole history was given up because one edit did not fit */
};                                          /* 56 bytes */
#if defined(__cplusplus)
static_assert(sizeof(struct volym_label_history_info) == 56, "volym_label_history_info is 56 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(struct volym_label_history_info) == 56, "volym_label_history_info is 56 bytes");
#endif
/* VOLYM_E_INVALID: NULL ctx or NULL out.  All 0 while the history is off. */
int   volym_label_history_info(volym_ctx* ctx, struct volym_label_history_info* out);

/* --- brush: paint labels along a stroke of picked texels (new; the reference has none) ------------------------------ */
/* Touching a segmentation up where the user points: the texels within a radius of a polyline of picked texels are relabelled by a
 * table, under a density window, in one call -- one undo step while the history is on.  The context ends up byte for byte where
 * volym_edit_labels leaves it: where a context handed the edited labels would be.
 *   The rule (integers only; scene.brush_volume of the Python package is its host twin, equal in every byte).  The stroke is the
 * union of n_points segments: point i gives the degenerate segment (p_i, p_i), a ball, when i == 0 or point i carries
 * VOLYM_BRUSH_LIFT, else the capsule (p_{i-1}, p_i) -- a LIFT in the middle breaks the polyline (a drag over a pixel without a
 * pick).  With <u, v> = sum over the axes of weight[a] * u[a] * v[a] (the distance pass's metric: a round brush is round in
 * millimetres), d = b - a and w = t - a, texel t lies within segment (a, b) iff
 *     <d,d> == 0 or <w,d> <= 0:   <w,w> <= r2;
 *     else <w,d> >= <d,d>:        <t-b, t-b> <= r2;
 *     else:                       <w,w> * <d,d> - <w,d>^2 <= r2 * <d,d>.
 * Points lie inside a volume of at most 4096 texels per axis and the weights are at most 64: every inner product is at most
 * 3 * 64 * 4095^2 < 2^32, so every product above and r2 * <d,d> is below 2^64, and the difference is non-negative by
 * Cauchy-Schwarz: the rule is exact in unsigned 64-bit arithmetic.  A texel t with label l becomes to[l] iff t lies in box,
 * to[l] != l, its density byte lies in [min_byte, max_byte] (the scene byte as it stands; with UNCUT the uncut copy as
 * volym_measure_pass reads it) and t lies within at least one segment.  Every texel is decided once, from the bytes before the edit:
 * a texel under two capsules and a table that swaps two labels is swapped once.  DRY_RUN fills the result and writes nothing.
 * r2 == 0 paints the texels exactly on the segments. */
#define VOLYM_BRUSH_MAX_POINTS 256u
enum { VOLYM_BRUSH_UNCUT = 1, VOLYM_BRUSH_DRY_RUN = 16 };      /* flags: the values of their VOLYM_RELABEL counterparts */
enum { VOLYM_BRUSH_LIFT = 1 };                                 /* volym_brush_point.flags */
struct volym_brush_point {
    uint16_t x, y, z;           /* a texel of the volume, in the coordinates of struct volym_pick */
    uint16_t flags;             /* VOLYM_BRUSH_LIFT: no capsule from the point before */
};                              /* 8 bytes */
typedef struct volym_brush {
    uint32_t box[6];            /* as volym_relabel: {x0, y0, z0, x1, y1, z1}, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint32_t min_byte, max_byte;   /* 0..255, min <= max: the density window; 0..255 = no window */
    uint8_t  to[256];           /* old label -> new label; to[l] == l: label l is not touched */
    uint32_t weight[3];         /* per axis, 1..VOLYM_DISTANCE_WEIGHT_MAX */
    uint32_t r2;                /* squared radius in the weighted metric; any value */
    uint32_t n_points;          /* 1..VOLYM_BRUSH_MAX_POINTS */
    struct volym_brush_point points[VOLYM_BRUSH_MAX_POINTS];
} volym_brush;                  /* 2360 bytes */
#if defined(__cplusplus)
static_assert(sizeof(struct volym_brush_point) == 8, "volym_brush_point is 8 bytes");
static_assert(sizeof(volym_brush) == 2360, "volym_brush is 2360 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(struct volym_brush_point) == 8, "volym_brush_point is 8 bytes");
_Static_assert(sizeof(volym_brush) == 2360, "volym_brush is 2360 bytes");
#endif
/* The brush: a blocking set-up call with the contract of volym_edit_labels (it waits for the frames in flight; the kernel runs on the
 * first slot's stream; with changed == 0, or DRY_RUN, nothing else is touched and a surface pass stays valid; otherwise counts, boxes,
 * density and importances follow and a surface pass is stale; out may be NULL).  The kernel walks the request's box cut to the
 * stroke's hull (volym_brush_box), not the volume.  While the history is on, a call that changes a texel (no DRY_RUN) is one step of
 * it, journalled into a staging area with room for min(items of that cut box's slab, budget / 20) records: volym_undo_labels and
 * volym_redo_labels take it as they take an edit.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_brush_check refuses.  VOLYM_E_STATE: what volym_edit_labels refuses of the
 * context's state.  The native multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_brush_labels(volym_ctx* ctx, const volym_brush* b, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, a window without min_byte <= max_byte <= 255, a weight outside 1..VOLYM_DISTANCE_WEIGHT_MAX, n_points outside
 * 1..VOLYM_BRUSH_MAX_POINTS, a point outside [0, dims), a point flag other than LIFT.  An empty box is valid: nothing changes.
 * Pure host arithmetic. */
int   volym_brush_check(const volym_brush* b, const uint32_t dims[3]);
/* The box the brush kernel walks: the request's box cut to the stroke's hull -- the points' box grown on axis a by e - 1, e the
 * smallest integer with weight[a] * e * e > r2 (no texel further than that from every point on one axis lies within a segment),
 * clipped to the volume.  box_out = {x0, y0, z0, x1, y1, z1}, hi exclusive; all 0 when the two do not meet.  Pure host arithmetic.
 * VOLYM_E_INVALID for NULL or what volym_brush_check refuses. */
int   volym_brush_box(const volym_brush* b, const uint32_t dims[3], uint32_t box_out[6]);

/* --- lasso: relabel the texels under a screen polygon (new; the reference has none) --------------------------------- */
/* Scissors: a polygon drawn over the picture, and every texel that projects into it -- through the whole volume, or through a range
 * of depths -- is relabelled by a table, under a box and a density window, in one call -- one undo step while the history is on.
 * With OUTSIDE the texels that do NOT project into it are: "keep only what is under the lasso".  The context ends up byte for byte
 * where volym_edit_labels leaves it: where a context handed the edited labels would be.
 *   The rule (integers only; scene.lasso_volume of the Python package is its host twin, equal in every byte).  For texel (x, y, z)
 * let h = (2x + 1, 2y + 1, 2z + 1), its centre in half-texels, and, in 64-bit integers,
 *     X = m[0] . h + c[0],   Y = m[1] . h + c[1],   D = m[2] . h + c[2].
 * With |m| < 2^31, |c| < 2^46 and h < 2^17 (a volume has at most 4096 texels per axis: h < 2^13) no value exceeds 2^51.  The texel
 * LANDS on pixel (px, py) iff depth[0] <= D <= depth[1] (depth[0] >= 1), 0 <= X < width * D and 0 <= Y < height * D; then
 * px = floor(X / D), py = floor(Y / D).  It is INSIDE iff it lands on a pixel of the polygon's mask, and SELECTED iff
 * inside != OUTSIDE: with OUTSIDE everything off screen, behind the eye or outside the depth range is selected.  A selected texel
 * with label l becomes to[l] iff it lies in box, to[l] != l and its density byte lies in [min_byte, max_byte] (the scene byte as it
 * stands; with UNCUT the uncut copy as volym_measure_pass reads it).  Every texel is decided once, from the bytes before the edit: a
 * table that swaps two labels swaps them once.  DRY_RUN fills the result and writes nothing.
 *   The polygon: n_points vertices, pixel positions in [-2^20, 2^20] that may lie off screen, closed implicitly, filled by the
 * even-odd rule with a half-open crossing rule: pixel (px, py) is in the mask iff an odd number of edges (x0, y0) -> (x1, y1) satisfy
 *     (y0 <= py) != (y1 <= py)   and   (px - x0) * (y1 - y0) < (x1 - x0) * (py - y0)  when y1 > y0,  > when y1 < y0
 * -- exact in 64-bit integers (every factor is below 2^22).  Two polygons that share an edge never both claim a pixel and never both
 * miss one; the polygon (x0,y0), (x1,y0), (x1,y1), (x0,y1) covers exactly x0 <= px < x1, y0 <= py < y1; the vertex order does not
 * matter; a bow-tie is empty where it overlaps twice.  The mask's rect is the polygon's bounding box cut to the frame
 * (volym_lasso_rect); if it is empty nothing is inside. */
#define VOLYM_LASSO_MAX_POINTS 1024u
#define VOLYM_LASSO_MAX_FRAME 16384u           /* width and height of the view */
#define VOLYM_LASSO_VERTEX_MAX 1048576         /* |x|, |y| of a vertex: 2^20 */
enum { VOLYM_LASSO_UNCUT = 1, VOLYM_LASSO_DRY_RUN = 16, VOLYM_LASSO_OUTSIDE = 32 };   /* flags: UNCUT and DRY_RUN carry the values of their VOLYM_RELABEL counterparts */
/* The integer view: texel -> (X, Y, D).  volym_lasso_view_from_camera makes one from a frame's camera; any other source (an
 * orthographic view has m[2] = 0 and c[2] > 0) works as well: the rule reads nothing but these integers. */
struct volym_lasso_view {
    int32_t  m[3][3];           /* rows X, Y, D: the coefficients of h; |m| < 2^31 */
    uint32_t width, height;     /* the frame, 1..VOLYM_LASSO_MAX_FRAME each */
    int32_t  scale_log2;        /* s of volym_lasso_view_from_camera (0 from any other source): volym_lasso_view_depth reads it, the rule does not */
    int64_t  c[3];              /* rows X, Y, D: the constant; |c| < 2^46 */
    int64_t  depth[2];          /* 1 <= depth[0] <= depth[1]: the range of D a texel may land from */
};                              /* 88 bytes */
struct volym_lasso_point { int32_t x, y; };     /* a vertex, in pixels */
typedef struct volym_lasso {
    uint32_t box[6];            /* as volym_relabel: {x0, y0, z0, x1, y1, z1}, lo <= hi <= volume size on every axis */
    uint32_t flags;
    uint32_t min_byte, max_byte;   /* 0..255, min <= max: the density window; 0..255 = no window */
    uint8_t  to[256];           /* old label -> new label; to[l] == l: label l is not touched */
    uint32_t n_points;          /* 3..VOLYM_LASSO_MAX_POINTS */
    struct volym_lasso_view view;
    struct volym_lasso_point points[VOLYM_LASSO_MAX_POINTS];
} volym_lasso;                  /* 8576 bytes */
#if defined(__cplusplus)
static_assert(sizeof(struct volym_lasso_view) == 88, "volym_lasso_view is 88 bytes");
static_assert(sizeof(struct volym_lasso_point) == 8, "volym_lasso_point is 8 bytes");
static_assert(sizeof(volym_lasso) == 8576, "volym_lasso is 8576 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(struct volym_lasso_view) == 88, "volym_lasso_view is 88 bytes");
_Static_assert(sizeof(struct volym_lasso_point) == 8, "volym_lasso_point is 8 bytes");
_Static_assert(sizeof(volym_lasso) == 8576, "volym_lasso is 8576 bytes");
#endif
/* The lasso: a blocking set-up call with the contract of volym_brush_labels (it waits for the frames in flight; the kernels run on
 * the first slot's stream; with changed == 0, or DRY_RUN, nothing but the mask is touched and a surface pass stays valid; otherwise
 * counts, boxes, density and importances follow and a surface pass is stale; out may be NULL).  A raster kernel fills the polygon's
 * bit plane over the mask's rect (volym_read_lasso_mask reads it), then the edit kernel walks the request's box.  While the history
 * is on, a call that changes a texel (no DRY_RUN) is one step of it, journalled into a staging area with room for min(items of the
 * box's slab, budget / 20) records: volym_undo_labels and volym_redo_labels take it as they take an edit.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_lasso_check refuses.  VOLYM_E_STATE: what volym_edit_labels refuses of the
 * context's state.  The native multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_lasso_labels(volym_ctx* ctx, const volym_lasso* lasso, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, a window without min_byte <= max_byte <= 255, n_points outside 3..VOLYM_LASSO_MAX_POINTS, a vertex coordinate outside
 * [-VOLYM_LASSO_VERTEX_MAX, VOLYM_LASSO_VERTEX_MAX], an entry of m at -2^31, |c| >= 2^46, depth[0] < 1 or depth[0] > depth[1],
 * width or height outside 1..VOLYM_LASSO_MAX_FRAME.  An empty box is valid: nothing changes.  Pure host arithmetic. */
int   volym_lasso_check(const volym_lasso* lasso, const uint32_t dims[3]);
/* The mask's rect: rect_out = {x0, y0, x1, y1}, hi exclusive -- the polygon's bounding box cut to the frame; all 0 when the two do
 * not meet.  Pure host arithmetic.  VOLYM_E_INVALID for NULL, n_points, a vertex or a frame that volym_lasso_check refuses. */
int   volym_lasso_rect(const volym_lasso* lasso, uint32_t rect_out[4]);
/* The polygon's bit plane of the latest volym_lasso_labels that passed its checks: rect_out as volym_lasso_rect gives it, and, words
 * not NULL, the plane's ceil((x1 - x0) / 32) * (y1 - y0) 32-bit words: pixel (px, py) is bit (px - x0) & 31 of word
 * (py - y0) * ceil((x1 - x0) / 32) + (px - x0) / 32; the bits past x1 are 0.  For a UI that fills the lasso.  Blocks.
 * VOLYM_E_INVALID: NULL ctx or rect_out, capacity (in words) too small.  VOLYM_E_STATE: no lasso yet. */
int   volym_read_lasso_mask(volym_ctx* ctx, uint32_t rect_out[4], uint32_t* words, uint64_t capacity);
/* The integer view of a frame, in the host part of the library: no context, no GPU.  camera: the frame's uniforms (view_matrix and
 * projection_matrix are read), width x height: the frame, dims: the volume, near: the near distance along the view axis in the
 * units of clip w (world units for a perspective projection; <= 0: none).  In double precision
 *     C = projection * view * diag(1 / (2 nx), 1 / (2 ny), 1 / (2 nz), 1)        (the volume is the unit cube; C acts on (h, 1))
 *     row X = (W / 2) (C0 + C3) + C3 / 2,   row Y = (H / 2) (C3 - C1) + C3 / 2,   row D = C3,
 * so that X / D = sx + 1/2 for the texel's screen position sx: the ray of pixel gx passes through the pixel's corner gx / W, and the
 * nearest ray to the texel is that of floor(sx + 1/2).  The three rows are scaled by the largest 2^s, s <= 40, that keeps every
 * rounded entry inside the bounds of volym_lasso_check, and depth = [max(1, round(near * 2^s)), INT64_MAX]; out->scale_log2 = s.
 * VOLYM_E_INVALID: NULL, a frame outside 1..VOLYM_LASSO_MAX_FRAME, a dimension outside 1..4096, a matrix that is
 * not finite, or no such s >= -40. */
int   volym_lasso_view_from_camera(const volym_camera_uniforms* camera, uint32_t width, uint32_t height, const uint32_t dims[3], double near,
                                   struct volym_lasso_view* out);
/* depth of `view` from two distances along the view axis in the units of volym_lasso_view_from_camera's near (scaled by the view's
 * scale_log2): depth = [max(1, round(front * 2^s)), round(back * 2^s)], back = +inf: INT64_MAX.  VOLYM_E_INVALID: NULL, a
 * distance that is not a number, back < front, or a range that rounds to depth[0] > depth[1]. */
int   volym_lasso_view_depth(struct volym_lasso_view* view, double front, double back);

/* --- smooth: a majority filter over a box of texels (new; the reference has none) ------------------------------------- */
/* The first edit that decides a texel from its neighbours' labels: a median filter for one segment, a joint majority filter for all
 * of them.  It removes threshold speckle, fills pinholes and rounds off the staircase a lasso or a brush leaves.  The context ends up
 * byte for byte where volym_read_labels, the host filter and volym_set_labels would have left it, and the history survives.
 *   The rule (integers only; scene.smooth_volume of the Python package is its host twin, equal in every byte).  For texel
 * t = (x, y, z) with label l, N(t) is the set of texels u OF THE VOLUME (not only of the box) with |u_a - t_a| <= radius[a] on every
 * axis; texels outside the volume do not exist and cast no vote.  count[m] = the number of u in N(t) that carry m, for the labels as
 * they stand before the call; hidden, cropped and clipped texels vote like any other (the cuts act through the density window
 * alone).  The candidates are l itself and every m with take[m] != 0.  The winner w is the candidate with the largest count: l if l
 * is among those with the largest count, else the smallest such m.  t becomes w iff t lies in the box, give[l] != 0, w != l and the
 * density byte lies in [min_byte, max_byte] (the scene byte as it stands, or the uncut copy with UNCUT, as volym_edit_labels reads
 * it).  Every texel is decided from the labels before the call: the result depends neither on the device layout nor on the order of
 * the workgroups.  DRY_RUN fills the result and writes nothing. */
#define VOLYM_SMOOTH_MAX_RADIUS 3u
enum { VOLYM_SMOOTH_UNCUT = 1, VOLYM_SMOOTH_DRY_RUN = 16 };   /* flags: they carry the values of their VOLYM_RELABEL counterparts */
typedef struct volym_smooth {
    uint32_t box[6];            /* as in volym_relabel: lo inclusive, hi exclusive, lo <= hi <= dims; an empty box is valid */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window, on the texel that would change */
    uint32_t radius[3];         /* each 0..VOLYM_SMOOTH_MAX_RADIUS, not all 0; (1, 1, 0) smooths inside slices */
    uint8_t  give[256];         /* give[l] != 0: texels that carry l may change */
    uint8_t  take[256];         /* take[m] != 0: label m may receive texels */
} volym_smooth;                 /* 560 bytes */
#ifdef __cplusplus
static_assert(sizeof(volym_smooth) == 560, "volym_smooth is 560 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_smooth) == 560, "volym_smooth is 560 bytes");
#endif
/* The smoothing: a blocking set-up call with the contract of volym_brush_labels (it waits for the frames in flight; the kernels run
 * on the first slot's stream; with changed == 0, or DRY_RUN, no label is touched and a surface pass stays valid; otherwise counts,
 * boxes, density and importances follow and a surface pass is stale; out may be NULL).  Two phases, because a texel's decision reads
 * labels another workgroup would overwrite: a vote kernel reads labels and density and leaves the chunks that change, as they will
 * be, in the journal's staging area; the swap of volym_undo_labels then exchanges them with the labels.  While the history is on, a
 * call that changes a texel (no DRY_RUN) is one step of it, kept if its records <= min(items of the box's slab, budget / 20).
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_smooth_check refuses.  VOLYM_E_STATE: what volym_edit_labels refuses of the
 * context's state.  The native multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_smooth_labels(volym_ctx* ctx, const volym_smooth* smooth, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, a window without min_byte <= max_byte <= 255, a radius above VOLYM_SMOOTH_MAX_RADIUS, all radii 0.  An empty box is valid:
 * nothing changes.  Pure host arithmetic. */
int   volym_smooth_check(const volym_smooth* smooth, const uint32_t dims[3]);

/* --- nearest segment: feature transform and fill by it (new; the reference has none) ------------------------------------ */
/* Which seed is nearest: the argmin beside the distance pass's min.  A read-only pass over the bytes of the scene as they stand.
 *   The rule (integers only; scene.nearest_volume of the Python package is its host twin, equal in every byte).  The request is the
 * distance pass's struct; PRESENT, SOLID and d2 are that pass's definitions; UNCUT is allowed, INSIDE is refused (the nearest texel
 * that is not solid may lie outside the box and has no label).  For a texel t of the box, site(t) is the solid texel s of the box
 * that minimises d2(t, s); ties go to the first s in ascending (z, y, x).  It is stored as the box-linear index of s (x fastest, as
 * in the distance map), or VOLYM_NEAREST_NONE when the box has no solid texel.  near_label(t) is the label byte of site(t) as the
 * labels stand at the pass: 0 while the context holds no labels of the volume's dimensions, and 0 where the site is NONE.  The same
 * request on the same scene gives the same bytes in either device layout, every time.  D is not kept: d2(t, site(t)) is three
 * multiplications.
 *   Memory, per texel of the box: 4 + 1 bytes of results (the site map holds the sweeps' g until the sites replace it), 6 of
 * winners (one uint16_t per axis) and 8 of stacks, for which the distance pass's work arrays serve where the context holds them
 * large enough (both passes run on the same stream, in stream order; its map, a result, is never used).  At 1024^3: 5 GiB of
 * results, 6 GiB of winners, 8 GiB of stacks -- 19 GiB, 11 GiB beside a distance pass of the same box. */
#define VOLYM_NEAREST_NONE 0xffffffffu              /* no solid texel in the box */
struct volym_nearest_summary {
    uint64_t n_solid, n_present;
    uint64_t n_finite;          /* texels of the box with a site */
    uint64_t cell[256];         /* texels of the box whose near_label is this label and whose site is not NONE */
    uint64_t cell_present[256]; /* ... those of them that are PRESENT and not SOLID: what a fill of all the matter would hand the label */
};                              /* 4120 bytes */
struct volym_nearest_site {
    uint32_t at[3];             /* the site, volume coordinates; {0, 0, 0}: none */
    uint32_t d2;                /* d2(t, site(t)) with the weights of the pass; VOLYM_NEAREST_NONE: none */
    uint32_t label;             /* near_label(t) */
};                              /* 20 bytes */
/* The fill: a texel t of box with label l becomes n = near_label(t) of the latest nearest pass iff give[l] != 0, site(t) is not
 * NONE, take[n] != 0, n != l, its density byte lies in [min_byte, max_byte] (the scene byte as it stands, with UNCUT the uncut copy,
 * as volym_edit_labels reads it) and d2_lo <= d2(t, site(t)) <= d2_hi with the weights of that pass.  Every texel is decided from the
 * snapshot and from its own bytes before the edit: the result depends neither on the layout nor on the order of the workgroups.
 * scene.fill_volume is the host twin. */
enum { VOLYM_FILL_UNCUT = 1, VOLYM_FILL_DRY_RUN = 2 };   /* flags */
typedef struct volym_fill {
    uint32_t box[6];            /* as in volym_relabel; it must lie inside the box of the nearest pass */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window, on the texel that would change */
    uint8_t  give[256];         /* give[l] != 0: texels that carry l may change */
    uint8_t  take[256];         /* take[n] != 0: label n may receive texels */
    uint32_t d2_lo, d2_hi;      /* lo <= hi: the band of d2(t, site(t)); 0 .. 0xffffffff = no band */
} volym_fill;                   /* 556 bytes */
#if defined(__cplusplus)
static_assert(sizeof(struct volym_nearest_summary) == 4120, "volym_nearest_summary is 4120 bytes");
static_assert(sizeof(struct volym_nearest_site) == 20, "volym_nearest_site is 20 bytes");
static_assert(sizeof(volym_fill) == 556, "volym_fill is 556 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(struct volym_nearest_summary) == 4120, "volym_nearest_summary is 4120 bytes");
_Static_assert(sizeof(struct volym_nearest_site) == 20, "volym_nearest_site is 20 bytes");
_Static_assert(sizeof(volym_fill) == 556, "volym_fill is 556 bytes");
#endif
/* Enqueue only, on the first slot's stream: the kernel that zeroes the summary, the row sweep, the column sweeps along y and z
 * (each also stores the entry that wins a position), and the resolve kernel that chains the winners into the site, reads its label
 * and accumulates the summary.  d == NULL: the whole volume, min_byte 1, every label, weights 1, no flags.  The one blocking path is
 * the first allocation, or a growth, of its buffers.  It needs what volym_distance_pass needs; an empty box launches only the zeroing
 * kernel.  The results are a snapshot: the reads below, and volym_fill_labels, stay valid after later edits of the scene.
 *   VOLYM_E_INVALID: NULL ctx, what volym_nearest_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions held in
 * the other device layout than the volume. */
int   volym_nearest_pass(volym_ctx* ctx, const volym_distance* d);
/* Validity without a context: what volym_distance_check refuses, and the INSIDE flag.  Pure host arithmetic. */
int   volym_nearest_check(const volym_distance* d, const uint32_t dims[3]);
/* The reads block.  All: VOLYM_E_STATE before any pass, and after volym_set_volume until the next one; VOLYM_E_INVALID for a NULL
 * ctx or output.  The maps are of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi, inside the pass's box; NULL: the
 * pass's whole box), box-linear in the sub-box; the sites they hold stay indices in the pass's box.  volym_nearest_at: the site of one
 * texel of the pass's box as volume coordinates, with its d2 and label (VOLYM_E_INVALID for a texel outside that box). */
int   volym_read_nearest(volym_ctx* ctx, struct volym_nearest_summary* out);
int   volym_read_nearest_sites(volym_ctx* ctx, const uint32_t sub[6], uint32_t* out);
int   volym_read_nearest_labels(volym_ctx* ctx, const uint32_t sub[6], uint8_t* out);
int   volym_nearest_at(volym_ctx* ctx, uint32_t x, uint32_t y, uint32_t z, struct volym_nearest_site* out);
/* The context's own results in device memory after a pass (NULL before any, and after volym_set_volume): the summary (a struct
 * volym_nearest_summary), the site map and the label map of the latest pass's box. */
void* volym_nearest_device_ptr(volym_ctx* ctx);
void* volym_nearest_sites_device_ptr(volym_ctx* ctx);
void* volym_nearest_labels_device_ptr(volym_ctx* ctx);
/* The fill: a blocking set-up call with the contract of volym_edit_labels (it waits for the frames in flight; one kernel, in place,
 * on the first slot's stream; with changed == 0, or DRY_RUN, nothing else is touched; otherwise counts, boxes, density and
 * importances follow; out may be NULL).  While the history is on, a call that changes a texel (no DRY_RUN) is one step of it.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_fill_check refuses, a box that reaches outside the box of the nearest pass.
 * VOLYM_E_STATE: what volym_edit_labels refuses of the context's state; no volym_nearest_pass since volym_set_volume.  The native
 * multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_fill_labels(volym_ctx* ctx, const volym_fill* f, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, a window without min_byte <= max_byte <= 255, d2_lo > d2_hi.  An empty box is valid: nothing changes.  Pure host arithmetic. */
int   volym_fill_check(const volym_fill* f, const uint32_t dims[3]);

/* --- geodesic growth: steps through the matter, and the flood by them (new; the reference has none) ---------------------- */
/* How far through the matter, and from which seed: the growth that stays inside a medium, where the distance and nearest passes
 * measure straight through anything.  A read-only pass over the bytes of the scene as they stand.
 *   The rule (integers only; scene.geodesic_volume of the Python package is its host twin, equal in every byte).  The density byte
 * and the label are read as the distance pass reads them: the scene as it stands, the uncut copy with UNCUT, label 0 everywhere
 * while the context holds no labels of the volume's dimensions.  IN: the density byte lies in [min_byte, max_byte].  SEED(t): t lies
 * in the box, and either IN and seed[label], or t is one of `points` (a point is a seed unconditionally).  MEDIUM(t): t lies in the
 * box, IN and through[label].  steps(t) is 0 on a seed; otherwise, for a MEDIUM texel, the length k of the shortest chain
 * s = p0, p1, ..., pk = t whose consecutive texels differ by 1 on exactly one axis, all in the box, s a seed, p1 .. pk MEDIUM; it is
 * VOLYM_GEODESIC_NONE if there is no such chain, if k > max_steps, or if t is neither seed nor medium.  geo_label(t) is the smallest
 * label byte among the seeds that have such a chain of exactly steps(t) to t, with the labels as they stand at the pass: a seed has
 * its own label, any other reached texel the smallest geo_label among its neighbours that have steps - 1.
 *   The map holds one key per texel of the box, box-linear with x fastest like the distance map: steps << 8 | geo_label, or
 * VOLYM_GEODESIC_NONE.  key(t) = min over the neighbours u of key(u) + 256 is monotone and has exactly one fixed point under the
 * step limit, so the same request on the same scene gives the same bytes in either device layout, whatever ran in which order.
 *   Memory: 4 bytes per texel of the box for the keys, and 16 bytes per tile of 32 x 8 x 8 texels. */
enum { VOLYM_GEODESIC_UNCUT = 1 };                  /* flags */
#define VOLYM_GEODESIC_POINTS_MAX 64u
#define VOLYM_GEODESIC_STEPS_MAX  0xfffffdu         /* 2^24 - 3: the largest step count a key holds */
#define VOLYM_GEODESIC_BOX_MAX    0x7ffffffeu       /* texels of a box */
#define VOLYM_GEODESIC_NONE       0xffffffffu       /* not reached */
typedef struct volym_geodesic {
    uint32_t box[6];            /* lo inclusive, hi exclusive, as volym_distance */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window of the medium and of the labelled seeds: min <= max <= 255 */
    uint8_t  seed[256];         /* label -> != 0: its texels in the window are seeds */
    uint8_t  through[256];      /* label -> != 0: its texels in the window are medium */
    uint32_t max_steps;         /* 0: VOLYM_GEODESIC_STEPS_MAX; else 1..VOLYM_GEODESIC_STEPS_MAX */
    uint32_t n_points;          /* 0..VOLYM_GEODESIC_POINTS_MAX */
    uint32_t points[VOLYM_GEODESIC_POINTS_MAX][3];  /* seed texels, volume coordinates, inside box; duplicates allowed */
} volym_geodesic;               /* 1324 bytes */
struct volym_geodesic_summary {
    uint64_t n_seed, n_medium, n_reached;   /* n_medium: MEDIUM and not SEED; n_reached: key != NONE, seeds included */
    uint32_t max_steps;         /* the largest steps reached; VOLYM_GEODESIC_NONE when n_reached == 0 */
    uint32_t max_at[3];         /* the first texel in ascending (z, y, x) that attains it, volume coordinates; {0, 0, 0}: none */
    uint64_t cell[256];         /* reached texels by geo_label */
    uint64_t cell_medium[256];  /* ... those of them that are not seeds: what a flood of everything would hand the label */
    uint64_t hist[256];         /* reached texels by min(steps, 255) */
};                              /* 6184 bytes */
struct volym_geodesic_site { uint32_t steps, label; };   /* VOLYM_GEODESIC_NONE, 0 where not reached */
/* The flood: a texel t of box with label l becomes n = to[g], g = geo_label(t) of the latest geodesic pass, iff give[l] != 0,
 * key(t) is not NONE, take[g] != 0, n != l, its density byte lies in [min_byte, max_byte] (the scene byte as it stands, with UNCUT the
 * uncut copy, as volym_edit_labels reads it) and steps_lo <= steps(t) <= steps_hi.  With `to` the identity it is the geodesic sibling
 * of volym_fill_labels; `to` lets a wand work from an unlabelled click, where the seed's label is 0 and to[0] the new segment.  Every
 * texel is decided from the snapshot and from its own bytes before the edit.  scene.flood_volume is the host twin. */
enum { VOLYM_FLOOD_UNCUT = 1, VOLYM_FLOOD_DRY_RUN = 2 };  /* flags */
typedef struct volym_flood {
    uint32_t box[6];            /* as in volym_relabel; it must lie inside the box of the latest geodesic pass */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window, on the texel that would change */
    uint8_t  give[256];         /* give[l] != 0: texels that carry l may change */
    uint8_t  take[256];         /* take[g] != 0: texels whose geo_label is g may change */
    uint8_t  to[256];           /* the label a texel of geo_label g becomes */
    uint32_t steps_lo, steps_hi;/* lo <= hi: the band of steps(t); 0 .. 0xffffffff = no band */
} volym_flood;                  /* 812 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_geodesic) == 1324, "volym_geodesic is 1324 bytes");
static_assert(sizeof(struct volym_geodesic_summary) == 6184, "volym_geodesic_summary is 6184 bytes");
static_assert(sizeof(struct volym_geodesic_site) == 8, "volym_geodesic_site is 8 bytes");
static_assert(sizeof(volym_flood) == 812, "volym_flood is 812 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_geodesic) == 1324, "volym_geodesic is 1324 bytes");
_Static_assert(sizeof(struct volym_geodesic_summary) == 6184, "volym_geodesic_summary is 6184 bytes");
_Static_assert(sizeof(struct volym_geodesic_site) == 8, "volym_geodesic_site is 8 bytes");
_Static_assert(sizeof(volym_flood) == 812, "volym_flood is 812 bytes");
#endif
/* A BLOCKING call, unlike the other passes: the rounds of its relaxation are enqueued in batches on the first slot's stream, and
 * after each batch the host reads 4 bytes, the number of tiles still marked, and stops at 0.  g == NULL: the whole volume, window
 * 1..255, every label but 0 a seed, label 0 the medium, no points.  It needs what volym_distance_pass needs.  The results are a
 * snapshot: the reads below, and volym_flood_labels, stay valid after later edits of the scene.  No scene byte is written.
 *   VOLYM_E_INVALID: NULL ctx, what volym_geodesic_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions held
 * in the other device layout than the volume.  VOLYM_E_HIP: a HIP error, or more rounds than the box has texels (a defect). */
int   volym_geodesic_pass(volym_ctx* ctx, const volym_geodesic* g);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis or with more
 * than VOLYM_GEODESIC_BOX_MAX texels, an unknown flag bit, a window without min_byte <= max_byte <= 255, max_steps or n_points above
 * their maxima, a point outside the box.  An empty box (without points) is valid.  Pure host arithmetic. */
int   volym_geodesic_check(const volym_geodesic* g, const uint32_t dims[3]);
/* The reads block.  All: VOLYM_E_STATE before any pass, and after volym_set_volume until the next one; VOLYM_E_INVALID for a NULL
 * ctx or output.  The map is of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi, inside the pass's box; NULL: the
 * pass's whole box), box-linear in the sub-box.  volym_geodesic_at: the key of one texel of the pass's box, taken apart
 * (VOLYM_E_INVALID for a texel outside that box). */
int   volym_read_geodesic(volym_ctx* ctx, struct volym_geodesic_summary* out);
int   volym_read_geodesic_map(volym_ctx* ctx, const uint32_t sub[6], uint32_t* out);
int   volym_geodesic_at(volym_ctx* ctx, uint32_t x, uint32_t y, uint32_t z, struct volym_geodesic_site* out);
/* The context's own results in device memory after a pass (NULL before any, and after volym_set_volume): the summary (a struct
 * volym_geodesic_summary) and the key map of the latest pass's box. */
void* volym_geodesic_device_ptr(volym_ctx* ctx);
void* volym_geodesic_map_device_ptr(volym_ctx* ctx);
/* The flood: a blocking set-up call with the contract of volym_edit_labels and volym_fill_labels (one kernel, in place, on the first
 * slot's stream; with changed == 0, or DRY_RUN, nothing else is touched; out may be NULL).  While the history is on, a call that
 * changes a texel (no DRY_RUN) is one step of it.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_flood_check refuses, a box that reaches outside the box of the geodesic pass.
 * VOLYM_E_STATE: what volym_edit_labels refuses of the context's state; no volym_geodesic_pass since volym_set_volume.  The native
 * multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_flood_labels(volym_ctx* ctx, const volym_flood* f, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, an unknown flag
 * bit, a window without min_byte <= max_byte <= 255, steps_lo > steps_hi.  An empty box is valid.  Pure host arithmetic. */
int   volym_flood_check(const volym_flood* f, const uint32_t dims[3]);

/* --- grow from seeds: cost-weighted growth through the matter, and the spread by it (new; the reference has none) -------- */
/* Where two growing segments meet is for the image to say: a step through the medium costs more the more the density changes
 * across it, and each texel goes to the seed it can be reached from most cheaply.  A read-only pass over the bytes of the scene
 * as they stand, the sibling of volym_geodesic_pass, whose steps all cost the same.
 *   The rule (integers only; scene.cost_volume of the Python package is its host twin, equal in every byte).  IN, SEED(t) and
 * MEDIUM(t) are exactly those of volym_geodesic above -- the box, the window [min_byte, max_byte], the seed and through tables, the
 * points (seeds unconditionally), UNCUT -- and the density byte b(t) and the label are read as that pass reads them.  A step from
 * a texel u to a texel t that differs from it by 1 on exactly one axis, both in the box, costs
 *     step(u, t) = step_cost + contrast_cost * |b(t) - b(u)|        (1 <= step_cost <= 255, 0 <= contrast_cost <= 255),
 * at most 255 + 255 * 255 = 65 280, and the same in either direction.  cost(t) is 0 on a seed; otherwise, for a MEDIUM texel, the
 * smallest sum of step costs over the chains s = p0, p1, ..., pk = t of such steps, s a seed, p1 .. pk MEDIUM.  cost_label(t) is
 * the smallest label byte among the seeds that have a chain of exactly cost(t) to t, with the labels as they stand at the pass.
 * The key is cost << 8 | cost_label; it is VOLYM_COST_NONE if there is no chain, if t is neither seed nor medium, or if
 * cost(t) > max_cost (0: VOLYM_COST_MAX).  A chain within the limit has only prefixes within it (costs are not negative), so the
 * map under a limit is the map without one, cut off.
 *   The map holds one key per texel of the box, box-linear with x fastest.  key(t) = min over the neighbours u of
 * key(u) + (step(u, t) << 8) is monotone, and because every step costs at least 1 it has exactly one fixed point under the limit:
 * the same request on the same scene gives the same bytes in either device layout, whatever ran in which order.  The sum can pass
 * 2^32 where key + 256 could not: it is formed saturating at 2^32 - 1 = VOLYM_COST_NONE, which is above every admitted key.
 *   Memory: 5 bytes per texel of the box (the keys, and the density bytes the relaxation reads), and 16 bytes per tile of
 * 32 x 8 x 8 texels. */
enum { VOLYM_COST_UNCUT = 1 };                      /* flags */
#define VOLYM_COST_POINTS_MAX 64u
#define VOLYM_COST_MAX        0xfffffdu             /* 2^24 - 3: the largest cost a key holds */
#define VOLYM_COST_STEP_MAX   65280u                /* 255 + 255 * 255: the most one step costs */
#define VOLYM_COST_BOX_MAX    0x7ffffffeu           /* texels of a box */
#define VOLYM_COST_NONE       0xffffffffu           /* not reached */
#define VOLYM_COST_HIST_SHIFT_MAX 16u
typedef struct volym_cost {
    uint32_t box[6];            /* lo inclusive, hi exclusive, as volym_geodesic */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window of the medium and of the labelled seeds: min <= max <= 255 */
    uint8_t  seed[256];         /* label -> != 0: its texels in the window are seeds */
    uint8_t  through[256];      /* label -> != 0: its texels in the window are medium */
    uint32_t max_cost;          /* 0: VOLYM_COST_MAX; else 1..VOLYM_COST_MAX */
    uint32_t n_points;          /* 0..VOLYM_COST_POINTS_MAX */
    uint32_t points[VOLYM_COST_POINTS_MAX][3];      /* seed texels, volume coordinates, inside box; duplicates allowed */
    uint32_t step_cost;         /* 1..255: what every step costs */
    uint32_t contrast_cost;     /* 0..255: what every unit of |b(t) - b(u)| adds; 0 with step_cost 1 is the geodesic pass */
    uint32_t hist_shift;        /* 0..16: the summary's histogram bins by min(cost >> hist_shift, 255) */
} volym_cost;                   /* 1336 bytes */
struct volym_cost_summary {
    uint64_t n_seed, n_medium, n_reached;   /* n_medium: MEDIUM and not SEED; n_reached: key != NONE, seeds included */
    uint32_t max_cost;          /* the largest cost reached; VOLYM_COST_NONE when n_reached == 0 */
    uint32_t max_at[3];         /* the first texel in ascending (z, y, x) that attains it, volume coordinates; {0, 0, 0}: none */
    uint64_t cell[256];         /* reached texels by cost_label */
    uint64_t cell_medium[256];  /* ... those of them that are not seeds: what a spread of everything would hand the label */
    uint64_t hist[256];         /* reached texels by min(cost >> hist_shift, 255) */
};                              /* 6184 bytes */
struct volym_cost_site { uint32_t cost, label; };    /* VOLYM_COST_NONE, 0 where not reached */
/* The spread: volym_flood_labels' rule read from the cost snapshot.  A texel t of box with label l becomes n = to[g],
 * g = cost_label(t) of the latest cost pass, iff give[l] != 0, key(t) is not NONE, take[g] != 0, n != l, its density byte lies in
 * [min_byte, max_byte] (the scene byte as it stands, with UNCUT the uncut copy) and cost_lo <= cost(t) <= cost_hi.  Every texel is
 * decided from the snapshot and from its own bytes before the edit.  scene.spread_volume is the host twin. */
enum { VOLYM_SPREAD_UNCUT = 1, VOLYM_SPREAD_DRY_RUN = 2 };  /* flags */
typedef struct volym_spread {
    uint32_t box[6];            /* as in volym_relabel; it must lie inside the box of the latest cost pass */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window, on the texel that would change */
    uint8_t  give[256];         /* give[l] != 0: texels that carry l may change */
    uint8_t  take[256];         /* take[g] != 0: texels whose cost_label is g may change */
    uint8_t  to[256];           /* the label a texel of cost_label g becomes */
    uint32_t cost_lo, cost_hi;  /* lo <= hi: the band of cost(t); 0 .. 0xffffffff = no band */
} volym_spread;                 /* 812 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_cost) == 1336, "volym_cost is 1336 bytes");
static_assert(sizeof(struct volym_cost_summary) == 6184, "volym_cost_summary is 6184 bytes");
static_assert(sizeof(struct volym_cost_site) == 8, "volym_cost_site is 8 bytes");
static_assert(sizeof(volym_spread) == 812, "volym_spread is 812 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_cost) == 1336, "volym_cost is 1336 bytes");
_Static_assert(sizeof(struct volym_cost_summary) == 6184, "volym_cost_summary is 6184 bytes");
_Static_assert(sizeof(struct volym_cost_site) == 8, "volym_cost_site is 8 bytes");
_Static_assert(sizeof(volym_spread) == 812, "volym_spread is 812 bytes");
#endif
/* A BLOCKING call, as volym_geodesic_pass is: the rounds of its relaxation are enqueued in batches on the first slot's stream, and
 * after each batch the host reads 4 bytes, the number of tiles still marked, and stops at 0.  q == NULL: the whole volume, window
 * 1..255, every label but 0 a seed, label 0 the medium, no points, step_cost 1, contrast_cost 16, no limit, hist_shift 4.  It needs
 * what volym_distance_pass needs.  The results are a snapshot of the pass's own -- summary, key map, the density bytes of the box
 * as the pass read them, tile state and box; it aliases no other pass's buffers -- so the reads below, and volym_spread_labels,
 * stay valid after later edits, tables, cuts and volym_set_labels; volym_set_volume drops it.  No scene byte is written.
 *   VOLYM_E_INVALID: NULL ctx, what volym_cost_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's dimensions held in
 * the other device layout than the volume.  VOLYM_E_HIP: a HIP error, or more rounds than the box has texels (a defect). */
int   volym_cost_pass(volym_ctx* ctx, const volym_cost* q);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for: NULL; a box without lo <= hi <= dims on every axis; a box with
 * more than VOLYM_COST_BOX_MAX texels; a flag bit other than UNCUT; a window without min_byte <= max_byte <= 255; step_cost
 * outside 1..255; contrast_cost above 255; max_cost above VOLYM_COST_MAX; hist_shift above 16; n_points above
 * VOLYM_COST_POINTS_MAX; a point outside the box.  An empty box (without points) is valid.  Pure host arithmetic. */
int   volym_cost_check(const volym_cost* q, const uint32_t dims[3]);
/* The reads block.  All: VOLYM_E_STATE before any pass, and after volym_set_volume until the next one; VOLYM_E_INVALID for a NULL
 * ctx or output.  The map is of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi, inside the pass's box; NULL: the
 * pass's whole box), box-linear in the sub-box.  volym_cost_at: the key of one texel of the pass's box, taken apart
 * (VOLYM_E_INVALID for a texel outside that box). */
int   volym_read_cost(volym_ctx* ctx, struct volym_cost_summary* out);
int   volym_read_cost_map(volym_ctx* ctx, const uint32_t sub[6], uint32_t* out);
int   volym_cost_at(volym_ctx* ctx, uint32_t x, uint32_t y, uint32_t z, struct volym_cost_site* out);
/* The context's own results in device memory after a pass (NULL before any, and after volym_set_volume): the summary (a struct
 * volym_cost_summary) and the key map of the latest pass's box. */
void* volym_cost_device_ptr(volym_ctx* ctx);
void* volym_cost_map_device_ptr(volym_ctx* ctx);
/* The spread: a blocking set-up call with the contract of volym_flood_labels (one kernel, in place, on the first slot's stream;
 * with changed == 0, or DRY_RUN, nothing else is touched; out may be NULL; the labels that may receive texels are
 * {to[g] : take[g]}).  While the history is on, a call that changes a texel (no DRY_RUN) is one step of it.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_spread_check refuses, a box that reaches outside the box of the cost pass.
 * VOLYM_E_STATE: what volym_edit_labels refuses of the context's state; no volym_cost_pass since volym_set_volume.  The native
 * multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_spread_labels(volym_ctx* ctx, const volym_spread* s, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, a flag bit
 * other than UNCUT and DRY_RUN, a window without min_byte <= max_byte <= 255, cost_lo > cost_hi.  An empty box is valid.  Pure
 * host arithmetic. */
int   volym_spread_check(const volym_spread* s, const uint32_t dims[3]);

/* --- fill between slices: interpolate a segment across gaps (new; the reference has none) ------------------------------ */
/* A segment painted on some slices is filled in on the slices between them: shape-based interpolation (Raya and Udupa) with the
 * distance pass's exact metric, decided by comparing squares.  A read-only pass over the bytes of the scene as they stand, and an
 * edit by its snapshot.
 *   The rule (integers only; scene.interpolate_volume of the Python package is its host twin, equal in every byte).  The SLICES are
 * the planes of box perpendicular to `axis`.  A texel of box is SHAPE when its density byte (the scene byte as it stands, with UNCUT
 * the uncut copy) is >= min_byte and select[label] != 0; min_byte may be 0 here -- labels alone decide -- and the label is 0
 * everywhere while the context holds no labels of the volume's dimensions.  Without KEYS the KEY slices are the slices that hold a
 * SHAPE texel; with KEYS they are the slices whose bit is set (bit c & 31 of keys[c >> 5], c the slice's volume coordinate along
 * axis), whether they hold a SHAPE texel or not.  A GAP is a maximal run of slices that are no keys between two keys z0 < z1; it is
 * fillable unless max_gap != 0 and the run is longer than max_gap.  Slices before the first key, after the last, or in a refused
 * gap are left alone.
 *   The signed planar map holds one uint32_t per texel of box, box-linear with x fastest: VOLYM_INTERPOLATE_NONE on a slice that is
 * no key.  On a key slice a SHAPE texel holds Din << 1 | 1, Din the smallest weighted squared distance within the slice (the two
 * weights of the in-plane axes; weight[axis] is not read) to a texel of the slice that is not SHAPE, texels outside box counting as
 * not SHAPE; a texel that is not SHAPE holds Dout << 1, Dout the distance to the nearest SHAPE texel of the slice, or NONE when the
 * slice has none (a KEYS slice without SHAPE: infinitely far outside).  D <= 2 * 64 * 4095^2 < 2^31.
 *   A texel of slice z of a fillable gap, with a = z1 - z, b = z - z0 and m0, m1 the words at its in-plane position in z0 and z1, is
 * INSIDE iff both words are SHAPE; or m0 is SHAPE, m1 is neither SHAPE nor NONE and a^2 D0 > b^2 D1; or m1 is SHAPE, m0 is neither
 * SHAPE nor NONE and b^2 D1 > a^2 D0 (D = m >> 1).  Equality is outside; the products are below 2^24 * 2^31, exact in 64 bits.
 * Nothing joins shapes that do not overlap in projection: each only shrinks towards the other key inside its own projection, and
 * the texels between them stay outside.  That is the method's known limit.
 *   The state map holds one byte per texel of box, box-linear: SHAPE (the texel was SHAPE at the pass) | INSIDE (on a key slice
 * equal to SHAPE, on a slice of a fillable gap the decision, else 0) | GAP (the slice belongs to a fillable gap).
 *   Memory: 17 bytes per texel of box (the two maps, and 12 bytes of work arrays), 17 GiB at 1024^3. */
enum { VOLYM_INTERPOLATE_UNCUT = 1, VOLYM_INTERPOLATE_KEYS = 2 };          /* volym_interpolate.flags */
enum { VOLYM_INTERPOLATE_SHAPE = 1, VOLYM_INTERPOLATE_INSIDE = 2, VOLYM_INTERPOLATE_GAP = 4 };   /* bits of a state byte */
enum { VOLYM_INTERPOLATE_SLICE_OUTSIDE = 0, VOLYM_INTERPOLATE_SLICE_KEY = 1, VOLYM_INTERPOLATE_SLICE_GAP = 2, VOLYM_INTERPOLATE_SLICE_REFUSED = 3 };
#define VOLYM_INTERPOLATE_NONE 0xffffffffu          /* no key slice, or a key slice without SHAPE */
#define VOLYM_INTERPOLATE_SLICES 4096
typedef struct volym_interpolate {
    uint32_t box[6];            /* lo inclusive, hi exclusive, as volym_distance */
    uint32_t flags;
    uint32_t min_byte;          /* 0..255 */
    uint8_t  select[256];
    uint32_t weight[3];         /* per axis, 1..VOLYM_DISTANCE_WEIGHT_MAX; the two in-plane ones are used */
    uint32_t axis;              /* 0, 1 or 2: x, y or z */
    uint32_t max_gap;           /* 0: no limit; else a gap of more slices is refused */
    uint32_t keys[VOLYM_INTERPOLATE_SLICES / 32];   /* KEYS only */
} volym_interpolate;            /* 820 bytes */
struct volym_interpolate_slice {
    uint32_t kind;              /* VOLYM_INTERPOLATE_SLICE_* */
    uint32_t key_lo, key_hi;    /* volume coordinates along axis: of the two keys about a GAP or REFUSED slice, of a KEY slice
                                 * itself; VOLYM_INTERPOLATE_NONE on an OUTSIDE slice */
    uint32_t count;             /* KEY: the slice's SHAPE texels; GAP: its INSIDE texels; else 0 */
};
struct volym_interpolate_summary {
    uint32_t n_slices;          /* the box's extent along axis (0: an empty box) */
    uint32_t n_keys;
    uint32_t n_gaps, n_gap_slices;      /* the fillable gaps and their slices */
    uint32_t n_refused;         /* the gaps max_gap refused */
    uint32_t reserved;          /* 0 */
    uint64_t n_shape;           /* SHAPE texels of the box */
    uint64_t n_inside;          /* INSIDE texels on gap slices */
    uint64_t n_new;             /* ... of them not SHAPE: what a fill adds */
    uint64_t n_stale;           /* SHAPE and not INSIDE on gap slices: what `out` erases */
    struct volym_interpolate_slice slice[VOLYM_INTERPOLATE_SLICES];   /* slice k of the box (coordinate box[axis] + k); 0 past n_slices */
};                              /* 65592 bytes */
/* The edit: a texel of box is considered when its state has GAP and its density byte lies in [min_byte, max_byte]; with label l it
 * becomes to[l] when its state has INSIDE and out[l] otherwise.  Identity tables touch nothing; `out` is what erases a stale earlier
 * fill.  It reads only the snapshot and the labels as they stand.  scene.interpolate_labels_volume is the host twin. */
enum { VOLYM_INTERPOLATE_EDIT_UNCUT = 1, VOLYM_INTERPOLATE_EDIT_DRY_RUN = 2 };      /* volym_interpolate_edit.flags */
typedef struct volym_interpolate_edit {
    uint32_t box[6];            /* as in volym_relabel; it must lie inside the box of the latest interpolate pass */
    uint32_t flags;
    uint32_t min_byte, max_byte;/* the density window, on the texel that would change */
    uint8_t  to[256];           /* the label an INSIDE texel of label l becomes */
    uint8_t  out[256];          /* ... and a texel of a gap slice that is not INSIDE */
} volym_interpolate_edit;       /* 548 bytes */
#if defined(__cplusplus)
static_assert(sizeof(volym_interpolate) == 820, "volym_interpolate is 820 bytes");
static_assert(sizeof(struct volym_interpolate_slice) == 16, "volym_interpolate_slice is 16 bytes");
static_assert(sizeof(struct volym_interpolate_summary) == 65592, "volym_interpolate_summary is 65592 bytes");
static_assert(sizeof(volym_interpolate_edit) == 548, "volym_interpolate_edit is 548 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(volym_interpolate) == 820, "volym_interpolate is 820 bytes");
_Static_assert(sizeof(struct volym_interpolate_slice) == 16, "volym_interpolate_slice is 16 bytes");
_Static_assert(sizeof(struct volym_interpolate_summary) == 65592, "volym_interpolate_summary is 65592 bytes");
_Static_assert(sizeof(volym_interpolate_edit) == 548, "volym_interpolate_edit is 548 bytes");
#endif
/* Enqueue one pass on the first slot's stream, as volym_distance_pass does: a handful of launches; it blocks only for the first
 * allocation, or a growth, of its buffers.  q must not be NULL.  It needs what volym_distance_pass needs; an empty box launches only
 * the zeroing kernel.  The results are a snapshot of the pass's own -- summary, signed map, state map and box; it aliases no other
 * pass's buffers -- so the reads below, and volym_interpolate_labels, stay valid after later edits, cuts and volym_set_labels;
 * volym_set_volume drops it.  No scene byte is written.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_interpolate_check refuses.  VOLYM_E_STATE: no volume; labels of the volume's
 * dimensions held in the other device layout than the volume.  VOLYM_E_NOMEM: an allocation failed (no snapshot is left). */
int   volym_interpolate_pass(volym_ctx* ctx, const volym_interpolate* q);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for: NULL; a box without lo <= hi <= dims on every axis; a box with more
 * than VOLYM_DISTANCE_BOX_MAX texels; an unknown flag bit; min_byte above 255; a weight outside 1..VOLYM_DISTANCE_WEIGHT_MAX; an
 * axis above 2; an extent above VOLYM_INTERPOLATE_SLICES.  An empty box is valid.  Pure host arithmetic. */
int   volym_interpolate_check(const volym_interpolate* q, const uint32_t dims[3]);
/* The reads block.  All: VOLYM_E_STATE before any pass, and after volym_set_volume until the next one; VOLYM_E_INVALID for a NULL
 * ctx or output.  The maps are of sub = {x0, y0, z0, x1, y1, z1} (volume coordinates, lo <= hi, inside the pass's box; NULL: the
 * pass's whole box), box-linear in the sub-box.  volym_interpolate_at: the signed word and the state byte of one texel of the
 * pass's box (VOLYM_E_INVALID for a texel outside it); either output may be NULL, not both. */
int   volym_read_interpolate(volym_ctx* ctx, struct volym_interpolate_summary* out);
int   volym_read_interpolate_map(volym_ctx* ctx, const uint32_t sub[6], uint32_t* out);
int   volym_read_interpolate_state(volym_ctx* ctx, const uint32_t sub[6], uint8_t* out);
int   volym_interpolate_at(volym_ctx* ctx, uint32_t x, uint32_t y, uint32_t z, uint32_t* word, uint8_t* state);
/* The context's own results in device memory after a pass (NULL before any, and after volym_set_volume): the summary (a struct
 * volym_interpolate_summary), the signed map and the state map of the latest pass's box. */
void* volym_interpolate_device_ptr(volym_ctx* ctx);
void* volym_interpolate_map_device_ptr(volym_ctx* ctx);
void* volym_interpolate_state_device_ptr(volym_ctx* ctx);
/* The edit: a blocking set-up call with the contract of volym_edit_labels (one kernel, in place, on the first slot's stream; with
 * changed == 0, or DRY_RUN, nothing else is touched; out may be NULL; the labels that may receive texels are those either table
 * moves a label to).  While the history is on, a call that changes a texel (no DRY_RUN) is one step of it.
 *   VOLYM_E_INVALID: NULL ctx or request, what volym_interpolate_labels_check refuses, a box that reaches outside the box of the
 * interpolate pass.  VOLYM_E_STATE: what volym_edit_labels refuses of the context's state; no volym_interpolate_pass since
 * volym_set_volume.  The native multi-GPU loop (volym_mgpu_*) has no forward for this call. */
int   volym_interpolate_labels(volym_ctx* ctx, const volym_interpolate_edit* e, struct volym_relabel_result* out);
/* Validity without a context: VOLYM_OK, or VOLYM_E_INVALID for NULL, a box without lo <= hi <= dims on every axis, a flag bit other
 * than UNCUT and DRY_RUN, a window without min_byte <= max_byte <= 255.  An empty box is valid.  Pure host arithmetic. */
int   volym_interpolate_labels_check(const volym_interpolate_edit* e, const uint32_t dims[3]);

/* --- measurement ------------------------------------------------------------------ */
int volym_stats_pass(volym_ctx* ctx, volym_stats* out);
/* n back-to-back compute passes timed with HIP events on the context's stream;
 * ms_each[n] receives each pass's duration (kernel only, inputs resident). */
int volym_time_passes(volym_ctx* ctx, uint32_t n, float* ms_each);
/* the same with ONE event pair around all n passes (no event packets between the kernels): total milliseconds */
int volym_time_batch(volym_ctx* ctx, uint32_t n, float* ms_total);
/* Self-test of the ray set-up for the frame of the last volym_update (wgsl:221-241; the reference has no counterpart): both
 * forms of its divisions -- shared reciprocals as the march kernels run them, plain IEEE divisions as the shader writes them --
 * for every pixel, compared bit for bit on the device.  out[0] = rays that differ in any bit of direction, entry, exit or hit
 * (must be 0), out[1] = rays of waves that fell back to the plain divisions, out[2] = rays.  Blocks. */
int volym_selftest_ray_setup(volym_ctx* ctx, unsigned long long out[3]);
/* Self-test of the texel selection of VOLYM_OPT_TEXEL_BYTES: clamp(floor(x), 0, 255) as the general kernels compute it
 * (v_cvt_flr_i32_f32, v_med3_i32) against the saturating byte conversion (v_cvt_pk_u8_f32), on the device, for every float x of
 * magnitude in [2^-10, 512) with both signs, +-0, the smallest and largest denormals, +-2^40, +-inf and four NaNs.
 * out[0] = values other than NaN on which the form the library is built with differs (must be 0), out[1] = NaNs on which it differs,
 * out[2], out[3] = the same two counts for the conversion with no floor in front of it, out[4] = values compared.  Needs no volume
 * and no frame.  Blocks. */
int volym_selftest_texel256(volym_ctx* ctx, unsigned long long out[5]);
/* 1 when the latest compute pass ran volym_raymarch_cube256_kernel (VOLYM_OPT_TEXEL_BYTES), 0 when it ran a general kernel or
 * there has been none. */
int volym_texel_bytes_in_use(volym_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
