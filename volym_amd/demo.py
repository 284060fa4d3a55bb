"""Python mirror of the reference's compute-plugin boundary over the C ABI.

    trait ComputeDemo { init(ctx, state, output_texture); update_gpu_state(ctx, state);
                        compute_pass(ctx) }              -- src/demos/mod.rs:9-17
    struct Simple                                        -- src/demos/simple/mod.rs:26-121

`GpuContext` stands where gpu_context.rs + GpuWriteTexture2D stood: a device, a stream
and a W x H rgba8 output.  All compute happens in libvolym_hip.so (HIP, gfx950).
"""
import ctypes as C

import numpy as np

from . import _lib, scene, synth


class GpuContext:
    """src/gpu_context.rs:20-62 + src/gpu_resources/texture.rs:40-59, headless."""

    def __init__(self, width, height, device_id=-1):
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        rc = _lib.lib().volym_create(C.byref(self._h), self.width, self.height, int(device_id))
        if rc != _lib.OK:
            raise _lib.VolymError(rc, (_lib.lib().volym_last_error(None) or b"").decode())

    @classmethod
    def borrow(cls, handle, width, height):
        """A view of a context somebody else owns (the native multi-GPU loop's): close() leaves it alone."""
        self = cls.__new__(cls)
        self.width, self.height = int(width), int(height)
        self._h = handle
        self._borrowed = True
        return self

    @property
    def handle(self):
        if not self._h:
            raise RuntimeError("GpuContext is closed")
        return self._h

    def _ck(self, rc):
        if rc != _lib.OK:
            raise _lib.VolymError(rc, (_lib.lib().volym_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            if not getattr(self, "_borrowed", False):
                _lib.lib().volym_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- options / sharding -----------------------------------------------------------------
    def set_option(self, key, value):
        self._ck(_lib.lib().volym_set_option(self.handle, int(key), int(value)))

    def set_stream(self, hip_stream):
        self._ck(_lib.lib().volym_set_stream(self.handle, C.c_void_p(hip_stream)))

    def set_shard(self, rank, world):
        self._ck(_lib.lib().volym_set_shard(self.handle, int(rank), int(world)))

    def bind_output(self, shard_ptr, frame_ptr):
        self._ck(_lib.lib().volym_bind_output(self.handle, C.c_void_p(shard_ptr), C.c_void_p(frame_ptr)))

    # ---- resources --------------------------------------------------------------------------
    def set_volume(self, voxels, dims, filter=_lib.FILTER_NEAREST):
        v = np.ascontiguousarray(voxels, np.uint8).ravel()
        nx, ny, nz = dims
        if v.size != nx * ny * nz:
            raise ValueError("volume has %d bytes, dims say %d" % (v.size, nx * ny * nz))
        self._ck(_lib.lib().volym_set_volume(self.handle, scene._u8p(v), nx, ny, nz, int(filter)))
        self._volume_dims, self._components_box = (int(nx), int(ny), int(nz)), None      # (read_component_ids shapes its result by them)
        self._distance_box = None
        self._nearest_box = None
        self._geodesic_box = None
        self._cost_box = None

    def set_importances(self, importances, dims):
        v = np.ascontiguousarray(importances, np.uint8).ravel()
        nx, ny, nz = dims
        if v.size != nx * ny * nz:
            raise ValueError("importances have %d bytes, dims say %d" % (v.size, nx * ny * nz))
        self._ck(_lib.lib().volym_set_importances(self.handle, scene._u8p(v), nx, ny, nz))

    def set_transfer_function(self, rgba8):
        t = np.ascontiguousarray(rgba8, np.uint8).ravel()
        self._ck(_lib.lib().volym_set_transfer_function(self.handle, scene._u8p(t), t.size // 4))

    def set_labels(self, labels, dims):
        """Prepared label bytes (scene.prepare_volume), kept on the device for set_segment_importances."""
        v = np.ascontiguousarray(labels, np.uint8).ravel()
        nx, ny, nz = dims
        if v.size != nx * ny * nz:
            raise ValueError("labels have %d bytes, dims say %d" % (v.size, nx * ny * nz))
        self._ck(_lib.lib().volym_set_labels(self.handle, scene._u8p(v), nx, ny, nz))
        self._label_dims = (int(nx), int(ny), int(nz))

    def set_segment_importances(self, table):
        """importance = table[label] for every voxel, on the device (table: 256 bytes, scene.segment_table)."""
        t = scene.check_segment_table(table)
        self._ck(_lib.lib().volym_set_segment_importances(self.handle, scene._u8p(t)))

    def label_counts(self):
        """Voxels per label value of the labels on the device (np.uint64[256])."""
        out = np.zeros(256, np.uint64)
        self._ck(_lib.lib().volym_label_counts(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def set_crop_box(self, lo, hi):
        """Crop box in texels of the prepared volume (lo inclusive, hi exclusive, x first): density and importances outside
        it count as 0 from the next compute pass on.  No upload; the device rewrites the slabs between the old and new faces."""
        lo3, hi3 = (C.c_uint32 * 3)(*[int(v) for v in lo]), (C.c_uint32 * 3)(*[int(v) for v in hi])
        self._ck(_lib.lib().volym_set_crop_box(self.handle, lo3, hi3))

    def crop_box(self):
        """(lo, hi) of the current crop box in texels; the whole volume when nothing is cropped."""
        lo3, hi3 = (C.c_uint32 * 3)(), (C.c_uint32 * 3)()
        self._ck(_lib.lib().volym_get_crop_box(self.handle, lo3, hi3))
        return tuple(int(v) for v in lo3), tuple(int(v) for v in hi3)

    def set_clip_plane(self, n, d):
        """Clip plane in texels of the prepared volume: texel (x, y, z) is kept iff n . (x, y, z) <= d, and density and
        importances of the others count as 0 from the next compute pass on; ((0, 0, 0), 0) lifts the plane.  No upload; the
        device rewrites the chunks in which a texel changes side."""
        n, d = scene.check_clip_plane(n, d)
        self._ck(_lib.lib().volym_set_clip_plane(self.handle, (C.c_int32 * 3)(*n), d))

    def clip_plane(self):
        """(n, d) of the current clip plane; ((0, 0, 0), 0) when there is none."""
        n3, d = (C.c_int32 * 3)(), C.c_int32(0)
        self._ck(_lib.lib().volym_get_clip_plane(self.handle, n3, C.byref(d)))
        return tuple(int(v) for v in n3), int(d.value)

    def set_segment_visibility(self, visible):
        """256 flags, one per label value (nonzero = visible): density and importances of the hidden segments count as 0 from
        the next compute pass on.  Needs the labels on the device (set_labels).  No upload; the device rewrites the texels
        inside the boxes of the labels that flipped."""
        v = scene.check_segment_visibility(visible)
        self._ck(_lib.lib().volym_set_segment_visibility(self.handle, scene._u8p(v)))

    def segment_visibility(self):
        """The current mask (np.uint8[256] of 0 / 1); all 1 when nothing is hidden."""
        out = np.zeros(256, np.uint8)
        self._ck(_lib.lib().volym_get_segment_visibility(self.handle, scene._u8p(out)))
        return out

    # ---- per frame --------------------------------------------------------------------------
    def update(self, camera_uniforms, parameter_uniforms):
        self._ck(_lib.lib().volym_update(self.handle, C.byref(camera_uniforms), C.byref(parameter_uniforms)))

    def compute_pass(self):
        self._ck(_lib.lib().volym_compute_pass(self.handle))

    def sync(self):
        self._ck(_lib.lib().volym_sync(self.handle))

    def throttle(self, max_in_flight=3):
        """Frame-loop back-pressure (the swap chain's role, src/event_loop.rs:114): at most `max_in_flight` frames ahead."""
        self._ck(_lib.lib().volym_throttle(self.handle, int(max_in_flight)))

    def settle(self):
        """Wait until a re-deal of the work lists in flight (cost feedback) has been adopted."""
        self._ck(_lib.lib().volym_settle(self.handle))

    def blit(self, out_w, out_h, target_ptr=None):
        """RenderPipeline::render_pass (src/render_pipeline.rs:88-130): frame -> out_w x out_h target."""
        self._blit_size = (int(out_h), int(out_w))
        self._ck(_lib.lib().volym_blit(self.handle, C.c_void_p(target_ptr), int(out_w), int(out_h)))

    def read_blit(self):
        h, w = self._blit_size
        out = np.empty((h, w, 4), np.uint8)
        self._ck(_lib.lib().volym_read_blit(self.handle, scene._u8p(out)))
        return out

    # ---- output -----------------------------------------------------------------------------
    def read_rgba8(self):
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._ck(_lib.lib().volym_read_rgba8(self.handle, scene._u8p(out)))
        return out

    def read_rgba32f(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(_lib.lib().volym_read_rgba32f(self.handle, scene._f32p(out)))
        return out

    def read_tile_bounds(self):
        """The tile mask and depth bounds of the latest pass's view (volym_read_tile_bounds): (mask, near, far), each of shape
        (8x8 tiles per column, per row); mask is bool.  VolymError E_STATE while the view has no mask."""
        L = _lib.lib()
        tx, ty, words = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(L.volym_tile_bounds_size(self.handle, C.byref(tx), C.byref(ty), C.byref(words)))
        bits = np.zeros(max(words.value, 1), np.uint32)
        near = np.zeros(32 * max(words.value, 1), np.float32)
        far = np.zeros_like(near)
        self._ck(L.volym_read_tile_bounds(self.handle, bits.ctypes.data_as(C.POINTER(C.c_uint32)), scene._f32p(near), scene._f32p(far)))
        n = tx.value * ty.value
        mask = ((bits[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)
        shape = (ty.value, tx.value)
        return mask.reshape(shape), near[:n].reshape(shape), far[:n].reshape(shape)

    def local_tiles(self):
        return int(_lib.lib().volym_local_tiles(self.handle))

    def shard_bytes(self):
        return int(_lib.lib().volym_shard_bytes(self.handle))

    def shard_device_ptr(self):
        return _lib.lib().volym_shard_device_ptr(self.handle)

    def frame_device_ptr(self):
        return _lib.lib().volym_frame_device_ptr(self.handle)

    def read_shard(self):
        out = np.empty(self.shard_bytes(), np.uint8)
        self._ck(_lib.lib().volym_read_shard(self.handle, scene._u8p(out)))
        return out

    def assemble(self, gathered_device_ptr):
        self._ck(_lib.lib().volym_assemble(self.handle, C.c_void_p(gathered_device_ptr)))

    def packed_shard_bytes(self, tiles):
        return int(_lib.lib().volym_packed_shard_bytes(self.handle, int(tiles)))

    def pack_shard(self, packed_device_ptr, capacity_bytes):
        self._ck(_lib.lib().volym_pack_shard(self.handle, C.c_void_p(packed_device_ptr), int(capacity_bytes)))

    def packed_tiles(self):
        """(tiles stored by the last pack, overflow flag); synchronises."""
        used, over = C.c_uint32(0), C.c_uint32(0)
        self._ck(_lib.lib().volym_packed_tiles(self.handle, C.byref(used), C.byref(over)))
        return int(used.value), int(over.value)

    def assemble_packed(self, gathered_device_ptr, stride_bytes):
        self._ck(_lib.lib().volym_assemble_packed(self.handle, C.c_void_p(gathered_device_ptr), int(stride_bytes)))

    def assemble_host(self, gathered):
        g = np.ascontiguousarray(gathered, np.uint8).ravel()
        self._ck(_lib.lib().volym_assemble_host(self.handle, scene._u8p(g)))

    # ---- pick ---------------------------------------------------------------------------------
    def pick_pass(self, rect=None, alpha_min=0.0):
        """Enqueue one pick march of rect = (x0, y0, w, h) (None: the whole frame) behind what is enqueued: per pixel the first
        composited sample after which alpha >= alpha_min (include/volym_hip.h volym_pick_pass)."""
        r = None
        if rect is not None:
            if len(rect) != 4:
                raise ValueError("a pick rect is (x0, y0, w, h)")
            r = (C.c_uint32 * 4)(*[int(v) for v in rect])
        self._ck(_lib.lib().volym_pick_pass(self.handle, r, float(alpha_min)))
        self._pick_size = (int(rect[3]), int(rect[2])) if rect is not None else (self.height, self.width)

    def read_picks(self):
        """The records of the latest pick pass: a structured array (_lib.PICK_DTYPE) of shape (h, w).  Blocks."""
        size = getattr(self, "_pick_size", None)
        out = np.zeros(size if size else (1, 1), _lib.PICK_DTYPE)
        self._ck(_lib.lib().volym_read_picks(self.handle, out.ctypes.data_as(C.POINTER(_lib.Pick))))
        return out

    def pick_device_ptr(self):
        """Device buffer of the latest pick pass (None before any)."""
        return _lib.lib().volym_pick_device_ptr(self.handle)

    def pick(self, x, y, alpha_min=0.0):
        """The record of pixel (x, y): a pass over one pixel plus the read (np.void of _lib.PICK_DTYPE).  Blocks."""
        out = np.zeros(1, _lib.PICK_DTYPE)
        self._ck(_lib.lib().volym_pick(self.handle, int(x), int(y), float(alpha_min), out.ctypes.data_as(C.POINTER(_lib.Pick))))
        self._pick_size = (1, 1)
        return out[0]

    # ---- outline ------------------------------------------------------------------------------
    def outline_pass(self, selected, ring_rgba, fill_rgba=(0, 0, 0, 0), radius=2, records_ptr=None, rect=None, target_ptr=None):
        """Enqueue one outline pass (include/volym_hip.h volym_outline_pass; scene.outline_frame is its definition): the frame of the
        latest compute pass with a ring of `radius` pixels in ring_rgba round the pixels whose pick record shows a label with
        selected[label] != 0, and those pixels tinted with fill_rgba.  records_ptr / rect: device memory of w * h records covering
        rect = (x0, y0, w, h); both None: the records of the latest pick pass.  target_ptr: device memory of W * H * 4 bytes (it may
        be frame_device_ptr()); None: a target the context owns (read_outline)."""
        o = _lib.Outline()
        C.memmove(o.selected, scene._u8p(scene.check_selection(selected)), 256)
        for name, c in (("ring_rgba", ring_rgba), ("fill_rgba", fill_rgba)):
            v = [int(x) for x in c]
            if len(v) != 4 or not all(0 <= x <= 255 for x in v):
                raise ValueError("%s is four bytes (r, g, b, a)" % name)
            setattr(o, name, (C.c_uint8 * 4)(*v))
        if not 0 <= int(radius) < 2 ** 32:
            raise ValueError("the radius is 1..8")
        o.radius = int(radius)
        r = None
        if rect is not None:
            if len(rect) != 4:
                raise ValueError("a rect is (x0, y0, w, h)")
            r = (C.c_uint32 * 4)(*[int(v) for v in rect])
        self._ck(_lib.lib().volym_outline_pass(self.handle, C.byref(o), C.c_void_p(records_ptr), r, C.c_void_p(target_ptr)))

    def read_outline(self):
        """The context's own outline target: (H, W, 4) uint8.  Blocks."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._ck(_lib.lib().volym_read_outline(self.handle, scene._u8p(out)))
        return out

    def outline_device_ptr(self):
        """The context's own outline target after the latest pass into it (None before any)."""
        return _lib.lib().volym_outline_device_ptr(self.handle)

    # ---- slice --------------------------------------------------------------------------------
    def slice_pass(self, slice, target_ptr=None):
        """Enqueue one slice pass (include/volym_hip.h volym_slice_pass; scene.slice_frame is its definition): `slice` is a
        scene.Slice (scene.slice_axis, scene.slice_through).  target_ptr: device memory of width * height * 4 bytes; None: a
        target the context owns (read_slice).  Needs a volume, nothing else: no update, no frame."""
        c = slice.to_c()
        self._ck(_lib.lib().volym_slice_pass(self.handle, C.byref(c), C.c_void_p(target_ptr)))
        if target_ptr is None:
            self._slice_size = (slice.height, slice.width)

    def read_slice(self):
        """The latest slice into the context's own target: (height, width, 4) uint8.  Blocks."""
        h, w = getattr(self, "_slice_size", None) or (1, 1)
        out = np.empty((h, w, 4), np.uint8)
        self._ck(_lib.lib().volym_read_slice(self.handle, scene._u8p(out)))
        return out

    def slice_device_ptr(self):
        """The context's own slice target after the latest pass into it (None before any)."""
        return _lib.lib().volym_slice_device_ptr(self.handle)

    # ---- projection ---------------------------------------------------------------------------
    def project_pass(self, projection, rect=None, records_ptr=None, image_ptr=None, own_image=False):
        """Enqueue one projection pass (include/volym_hip.h volym_project_pass; scene.project_frame is its definition): maximum and
        mean intensity along the rays of rect = (x0, y0, w, h) (None: the whole frame) of the last update's view.  `projection`
        is a scene.Projection.  records_ptr: device memory of w * h records; None: records the context owns (read_projection).
        image_ptr: device memory of w * h * 4 bytes; None: no image -- unless own_image, which puts records and image both into
        buffers the context owns (volym_project_image_pass; read_projection_image)."""
        c = projection.to_c()
        r = None
        if rect is not None:
            if len(rect) != 4:
                raise ValueError("a projection rect is (x0, y0, w, h)")
            r = (C.c_uint32 * 4)(*[int(v) for v in rect])
        if own_image:
            if records_ptr is not None or image_ptr is not None:
                raise ValueError("own_image puts records and image into the context's own buffers")
            self._ck(_lib.lib().volym_project_image_pass(self.handle, C.byref(c), r))
        else:
            self._ck(_lib.lib().volym_project_pass(self.handle, C.byref(c), r, C.c_void_p(records_ptr), C.c_void_p(image_ptr)))

    def _projection_shape(self, fn):
        """(h, w) of the latest pass into one of the context's own buffers, asked of the context"""
        size = (C.c_uint32 * 2)()
        self._ck(fn(self.handle, size))
        return int(size[1]), int(size[0])

    def read_projection(self):
        """The records of the latest projection pass into the context's own records: a structured array (_lib.PROJECTION_DTYPE) of
        shape (h, w).  Blocks."""
        h, w = self._projection_shape(_lib.lib().volym_projection_size)
        out = np.zeros((max(h, 1), max(w, 1)), _lib.PROJECTION_DTYPE)       # (before any pass the read refuses)
        self._ck(_lib.lib().volym_read_projection(self.handle, out.ctypes.data_as(C.POINTER(_lib.Projection))))
        return out

    def read_projection_image(self):
        """The image of the latest projection pass with own_image: (h, w, 4) uint8.  Blocks."""
        h, w = self._projection_shape(_lib.lib().volym_projection_image_size)
        out = np.empty((max(h, 1), max(w, 1), 4), np.uint8)
        self._ck(_lib.lib().volym_read_projection_image(self.handle, scene._u8p(out)))
        return out

    def projection_device_ptr(self):
        """The context's own projection records after the latest pass into them (None before any)."""
        return _lib.lib().volym_projection_device_ptr(self.handle)

    def projection_image_device_ptr(self):
        """The context's own projection image after the latest pass into it (None before any)."""
        return _lib.lib().volym_projection_image_device_ptr(self.handle)

    def project_at(self, x, y, step):
        """The record of pixel (x, y): a pass over one pixel plus the read (np.void of _lib.PROJECTION_DTYPE).  Blocks.  The
        context's own records stay what the latest project_pass made them."""
        out = np.zeros(1, _lib.PROJECTION_DTYPE)
        self._ck(_lib.lib().volym_project_at(self.handle, int(x), int(y), float(step), out.ctypes.data_as(C.POINTER(_lib.Projection))))
        return out[0]

    # ---- measuring segments -----------------------------------------------------------------
    def measure_pass(self, measure=None):
        """Enqueue one measure pass (include/volym_hip.h volym_measure_pass; scene.measure_volume is its definition): per-label
        statistics and grouped density histograms of the scene under its cuts.  `measure` is a scene.Measure; None: the whole
        volume, every label in group 0.  Needs a volume, nothing else: no update, no frame."""
        c = None if measure is None else C.byref(measure.to_c())
        self._ck(_lib.lib().volym_measure_pass(self.handle, c))

    def read_measure(self):
        """The result of the latest measure pass: (records, hist) -- a structured array of 256 _lib.SEGMENT_STATS_DTYPE records, one
        per label value, and a uint64[8, 256] array of histograms.  Blocks."""
        out = np.zeros(C.sizeof(_lib.Measurement), np.uint8)
        self._ck(_lib.lib().volym_read_measure(self.handle, out.ctypes.data_as(C.POINTER(_lib.Measurement))))
        n = 256 * _lib.SEGMENT_STATS_DTYPE.itemsize
        return out[:n].view(_lib.SEGMENT_STATS_DTYPE).copy(), out[n:].view(np.uint64).reshape(_lib.MEASURE_GROUPS, 256).copy()

    def measure_device_ptr(self):
        """The context's own result (a volym_measurement in device memory) after a pass (None before any)."""
        return _lib.lib().volym_measure_device_ptr(self.handle)

    # ---- segment surfaces ----------------------------------------------------------------------
    def surface_pass(self, surface=None):
        """Enqueue one surface pass (include/volym_hip.h volym_surface_pass; scene.surface_volume is its definition): the boundary
        faces of the solid texels of the scene as it stands, counted per label and direction, and the offset of every row's first
        face.  `surface` is a scene.Surface; None: the whole volume, min_byte 1, every label."""
        c = None if surface is None else C.byref(surface.to_c())
        self._ck(_lib.lib().volym_surface_pass(self.handle, c))

    def read_surface(self):
        """The summary of the latest surface pass: an np.void of _lib.SURFACE_SUMMARY_DTYPE (faces, total, pos, neg).  Blocks."""
        out = np.zeros(1, _lib.SURFACE_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_surface(self.handle, out.ctypes.data_as(C.POINTER(_lib.SurfaceSummary))))
        return out[0]

    def surface_device_ptr(self):
        """The context's own summary (a volym_surface_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_surface_device_ptr(self.handle)

    def surface_faces_pass(self, target_ptr=None, capacity_faces=0):
        """The emit pass of the latest surface pass (volym_surface_faces_pass): its faces in ascending (z, y, x, dir) into device
        memory of capacity_faces 8-byte records at target_ptr, or (None) into a buffer the context owns (read_surface_faces)."""
        self._ck(_lib.lib().volym_surface_faces_pass(self.handle, target_ptr, int(capacity_faces)))

    def read_surface_faces(self, total=None):
        """The face records of the latest surface_faces_pass into the context's own buffer (_lib.SURFACE_FACE_DTYPE).  total: how
        many the pass wrote, when the caller has read the summary already (None: it is read here).  Blocks."""
        n = int(self.read_surface()["total"]) if total is None else int(total)
        out = np.zeros(n, _lib.SURFACE_FACE_DTYPE)
        self._ck(_lib.lib().volym_read_surface_faces(self.handle, out.ctypes.data_as(C.POINTER(_lib.SurfaceFace)), n))
        return out

    # ---- connected components ----------------------------------------------------------------
    def components_pass(self, components=None):
        """Enqueue one components pass (include/volym_hip.h volym_components_pass; scene.components_volume is its definition): the
        6-connected pieces of the solid texels of the scene as it stands, numbered in the order of their first texels.
        `components` is a scene.Components; None: the whole volume, min_byte 1, every label, the default table capacity."""
        c = None if components is None else C.byref(components.to_c())
        self._ck(_lib.lib().volym_components_pass(self.handle, c))
        box = ((0, 0, 0), getattr(self, "_volume_dims", (0, 0, 0))) if components is None else components.box
        self._components_box = box if all(a < b for a, b in zip(*box)) else None

    def read_components(self):
        """The summary of the latest components pass: an np.void of _lib.COMPONENTS_SUMMARY_DTYPE (n_components, n_solid, recorded,
        per_label).  Blocks."""
        out = np.zeros(1, _lib.COMPONENTS_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_components(self.handle, out.ctypes.data_as(C.POINTER(_lib.ComponentsSummary))))
        return out[0]

    def read_component_table(self, recorded=None):
        """The records of the latest components pass (_lib.COMPONENT_DTYPE): record k describes component k.  recorded: how many the
        pass kept, when the caller has read the summary already (None: it is read here).  Blocks."""
        n = int(self.read_components()["recorded"]) if recorded is None else int(recorded)
        out = np.zeros(n, _lib.COMPONENT_DTYPE)
        self._ck(_lib.lib().volym_read_component_table(self.handle, out.ctypes.data_as(C.POINTER(_lib.Component)), n))
        return out

    def read_component_ids(self, sub=None):
        """The ids of the latest components pass as a uint32 array [z, y, x]: of its whole box (None) or of the sub-box (lo, hi) in
        texels of the volume, which must lie inside the pass's box.  _lib.COMPONENT_NONE marks a texel that is not solid.  Blocks."""
        box = getattr(self, "_components_box", None) if sub is None else (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        if box is None:                                        # no pass yet (the library refuses), or a pass over an empty box
            self._ck(_lib.lib().volym_read_component_ids(self.handle, None, None))
            return np.zeros((0, 0, 0), np.uint32)
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        shape = tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0))
        out = np.zeros(shape, np.uint32)
        self._ck(_lib.lib().volym_read_component_ids(self.handle, c, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def component_of(self, x, y, z):
        """The id of texel (x, y, z) in the latest components pass (_lib.COMPONENT_NONE: not solid).  Blocks; copies 4 bytes."""
        out = C.c_uint32(0)
        self._ck(_lib.lib().volym_component_of(self.handle, int(x), int(y), int(z), C.byref(out)))
        return int(out.value)

    def components_device_ptr(self):
        """The context's own summary (a volym_components_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_components_device_ptr(self.handle)

    def component_ids_device_ptr(self):
        """The id volume of the latest components pass in device memory (None before any)."""
        return _lib.lib().volym_component_ids_device_ptr(self.handle)

    def component_table_device_ptr(self):
        """The records of the latest components pass in device memory (None before any)."""
        return _lib.lib().volym_component_table_device_ptr(self.handle)

    # ---- distance maps ---------------------------------------------------------------------------
    def distance_pass(self, distance=None):
        """Enqueue one distance pass (include/volym_hip.h volym_distance_pass; scene.distance_volume is its definition): the exact
        weighted squared distance from every texel of the request's box to the nearest solid texel (INSIDE: to the nearest texel
        that is not solid) of the scene as it stands.  `distance` is a scene.Distance; None: the whole volume, min_byte 1, every
        label, weights 1, no flags."""
        d = None if distance is None else C.byref(distance.to_c())
        self._ck(_lib.lib().volym_distance_pass(self.handle, d))
        box = ((0, 0, 0), getattr(self, "_volume_dims", (0, 0, 0))) if distance is None else distance.box
        self._distance_box = box if all(a < b for a, b in zip(*box)) else None

    def read_distance(self):
        """The summary of the latest distance pass: an np.void of _lib.DISTANCE_SUMMARY_DTYPE.  Blocks."""
        out = np.zeros(1, _lib.DISTANCE_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_distance(self.handle, out.ctypes.data_as(C.POINTER(_lib.DistanceSummary))))
        return out[0]

    def read_distance_map(self, sub=None):
        """The map of the latest distance pass as a uint32 array [z, y, x]: of its whole box (None) or of the sub-box (lo, hi) in
        texels of the volume, which must lie inside the pass's box.  _lib.DISTANCE_NONE: the box holds no seed.  Blocks."""
        box = getattr(self, "_distance_box", None) if sub is None else (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        if box is None:                                        # no pass yet (the library refuses), or a pass over an empty box
            self._ck(_lib.lib().volym_read_distance_map(self.handle, None, None))
            return np.zeros((0, 0, 0), np.uint32)
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        shape = tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0))
        out = np.zeros(shape, np.uint32)
        self._ck(_lib.lib().volym_read_distance_map(self.handle, c, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def distance_at(self, x, y, z):
        """D of texel (x, y, z) in the latest distance pass (_lib.DISTANCE_NONE: no seed).  Blocks; copies 4 bytes."""
        out = C.c_uint32(0)
        self._ck(_lib.lib().volym_distance_at(self.handle, int(x), int(y), int(z), C.byref(out)))
        return int(out.value)

    def distance_device_ptr(self):
        """The context's own summary (a volym_distance_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_distance_device_ptr(self.handle)

    def distance_map_device_ptr(self):
        """The map of the latest distance pass in device memory (None before any)."""
        return _lib.lib().volym_distance_map_device_ptr(self.handle)

    # ---- nearest segment -------------------------------------------------------------------------
    def nearest_pass(self, distance=None):
        """Enqueue one nearest pass (include/volym_hip.h volym_nearest_pass; scene.nearest_volume is its definition): for every texel
        of the request's box the nearest solid texel of the box -- the first in (z, y, x) among equals -- and its label, of the scene
        as it stands.  `distance` is a scene.Distance without INSIDE; None: the whole volume, min_byte 1, every label, weights 1."""
        d = None if distance is None else C.byref(distance.to_c())
        self._ck(_lib.lib().volym_nearest_pass(self.handle, d))
        box = ((0, 0, 0), getattr(self, "_volume_dims", (0, 0, 0))) if distance is None else distance.box
        self._nearest_box = box if all(a < b for a, b in zip(*box)) else None

    def read_nearest(self):
        """The summary of the latest nearest pass: an np.void of _lib.NEAREST_SUMMARY_DTYPE.  Blocks."""
        out = np.zeros(1, _lib.NEAREST_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_nearest(self.handle, out.ctypes.data_as(C.POINTER(_lib.NearestSummary))))
        return out[0]

    def _read_nearest_map(self, call, dtype, ctype, sub):
        box = getattr(self, "_nearest_box", None) if sub is None else (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        if box is None:                                        # no pass yet (the library refuses), or a pass over an empty box
            self._ck(call(self.handle, None, None))
            return np.zeros((0, 0, 0), dtype)
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        out = np.zeros(tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0)), dtype)
        self._ck(call(self.handle, c, out.ctypes.data_as(C.POINTER(ctype))))
        return out

    def read_nearest_sites(self, sub=None):
        """The site map of the latest nearest pass as a uint32 array [z, y, x]: of its whole box (None) or of the sub-box (lo, hi) in
        texels of the volume, which must lie inside the pass's box.  A site is an index in the pass's box, x fastest;
        _lib.NEAREST_NONE: the box holds no solid texel.  Blocks."""
        return self._read_nearest_map(_lib.lib().volym_read_nearest_sites, np.uint32, C.c_uint32, sub)

    def read_nearest_labels(self, sub=None):
        """The label of every texel's site in the latest nearest pass as a uint8 array [z, y, x], as read_nearest_sites.  Blocks."""
        return self._read_nearest_map(_lib.lib().volym_read_nearest_labels, np.uint8, C.c_uint8, sub)

    def nearest_at(self, x, y, z):
        """The site of texel (x, y, z) in the latest nearest pass: {"at": its volume coordinates (None: no solid texel in the box),
        "d2", "label"}.  Blocks."""
        out = _lib.NearestSite()
        self._ck(_lib.lib().volym_nearest_at(self.handle, int(x), int(y), int(z), C.byref(out)))
        none = int(out.d2) == _lib.NEAREST_NONE
        return {"at": None if none else tuple(int(v) for v in out.at), "d2": None if none else int(out.d2), "label": int(out.label)}

    def nearest_device_ptr(self):
        """The context's own summary (a volym_nearest_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_nearest_device_ptr(self.handle)

    def nearest_sites_device_ptr(self):
        """The site map of the latest nearest pass in device memory (None before any)."""
        return _lib.lib().volym_nearest_sites_device_ptr(self.handle)

    def nearest_labels_device_ptr(self):
        """The label map of the latest nearest pass in device memory (None before any)."""
        return _lib.lib().volym_nearest_labels_device_ptr(self.handle)

    def fill_labels(self, fill):
        """One fill on the device (include/volym_hip.h volym_fill_labels; scene.fill_volume is its definition): a texel of the box
        whose label gives becomes the label of its site in the latest nearest pass, where the take table, the density window and the
        band say so.  `fill` is a scene.Fill.  Everything follows as after edit_labels, and the call is one step of the history.
        Blocks.  Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_fill_labels(self.handle, C.byref(fill.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    # ---- geodesic growth -------------------------------------------------------------------------
    def geodesic_pass(self, geodesic=None):
        """One geodesic pass (include/volym_hip.h volym_geodesic_pass; scene.geodesic_volume is its definition): for every texel of
        the request's box the number of 6-connected steps through the medium to the nearest seed, and the smallest label among the
        seeds that near, of the scene as it stands.  `geodesic` is a scene.Geodesic; None: the whole volume, window 1..255, every
        label but 0 a seed, label 0 the medium.  Blocks, unlike the other passes: the host counts the rounds."""
        g = None if geodesic is None else C.byref(geodesic.to_c())
        self._ck(_lib.lib().volym_geodesic_pass(self.handle, g))
        box = ((0, 0, 0), getattr(self, "_volume_dims", (0, 0, 0))) if geodesic is None else geodesic.box
        self._geodesic_box = box if all(a < b for a, b in zip(*box)) else None

    def read_geodesic(self):
        """The summary of the latest geodesic pass: an np.void of _lib.GEODESIC_SUMMARY_DTYPE.  Blocks."""
        out = np.zeros(1, _lib.GEODESIC_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_geodesic(self.handle, out.ctypes.data_as(C.POINTER(_lib.GeodesicSummary))))
        return out[0]

    def read_geodesic_map(self, sub=None):
        """The keys of the latest geodesic pass (steps << 8 | geo_label; _lib.GEODESIC_NONE: not reached) as a uint32 array
        [z, y, x]: of its whole box (None) or of the sub-box (lo, hi) in texels of the volume, which must lie inside the pass's
        box.  Blocks."""
        box = getattr(self, "_geodesic_box", None) if sub is None else (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        call = _lib.lib().volym_read_geodesic_map
        if box is None:                                        # no pass yet (the library refuses), or a pass over an empty box
            self._ck(call(self.handle, None, None))
            return np.zeros((0, 0, 0), np.uint32)
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        out = np.zeros(tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0)), np.uint32)
        self._ck(call(self.handle, c, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def geodesic_at(self, x, y, z):
        """The key of texel (x, y, z) in the latest geodesic pass, taken apart: {"steps" (None: not reached), "label"}.  Blocks."""
        out = _lib.GeodesicSite()
        self._ck(_lib.lib().volym_geodesic_at(self.handle, int(x), int(y), int(z), C.byref(out)))
        none = int(out.steps) == _lib.GEODESIC_NONE
        return {"steps": None if none else int(out.steps), "label": int(out.label)}

    def geodesic_device_ptr(self):
        """The context's own summary (a volym_geodesic_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_geodesic_device_ptr(self.handle)

    def geodesic_map_device_ptr(self):
        """The key map of the latest geodesic pass in device memory (None before any)."""
        return _lib.lib().volym_geodesic_map_device_ptr(self.handle)

    def flood_labels(self, flood):
        """One flood on the device (include/volym_hip.h volym_flood_labels; scene.flood_volume is its definition): a texel of the
        box whose label gives becomes to[g], g its geo label in the latest geodesic pass, where the take table, the density window
        and the band of steps say so.  `flood` is a scene.Flood.  Everything follows as after edit_labels, and the call is one step
        of the history.  Blocks.  Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_flood_labels(self.handle, C.byref(flood.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    # ---- grow from seeds: cost-weighted growth -----------------------------------------------------
    def cost_pass(self, cost=None):
        """One cost pass (include/volym_hip.h volym_cost_pass; scene.cost_volume is its definition): for every texel of the request's
        box the cost of the cheapest chain of 6-connected steps through the medium from a seed, where a step costs more the more the
        density changes across it, and the smallest label among the seeds that attain it, of the scene as it stands.  `cost` is a
        scene.Cost; None: the whole volume, window 1..255, every label but 0 a seed, label 0 the medium, step 1, contrast 16.  Blocks,
        as geodesic_pass does: the host counts the rounds."""
        q = None if cost is None else C.byref(cost.to_c())
        self._ck(_lib.lib().volym_cost_pass(self.handle, q))
        box = ((0, 0, 0), getattr(self, "_volume_dims", (0, 0, 0))) if cost is None else cost.box
        self._cost_box = box if all(a < b for a, b in zip(*box)) else None

    def read_cost(self):
        """The summary of the latest cost pass: an np.void of _lib.COST_SUMMARY_DTYPE.  Blocks."""
        out = np.zeros(1, _lib.COST_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_cost(self.handle, out.ctypes.data_as(C.POINTER(_lib.CostSummary))))
        return out[0]

    def read_cost_map(self, sub=None):
        """The keys of the latest cost pass (cost << 8 | cost_label; _lib.COST_NONE: not reached) as a uint32 array [z, y, x]: of its
        whole box (None) or of the sub-box (lo, hi) in texels of the volume, which must lie inside the pass's box.  Blocks."""
        box = getattr(self, "_cost_box", None) if sub is None else (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        call = _lib.lib().volym_read_cost_map
        if box is None:                                        # no pass yet (the library refuses), or a pass over an empty box
            self._ck(call(self.handle, None, None))
            return np.zeros((0, 0, 0), np.uint32)
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        out = np.zeros(tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0)), np.uint32)
        self._ck(call(self.handle, c, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def cost_at(self, x, y, z):
        """The key of texel (x, y, z) in the latest cost pass, taken apart: {"cost" (None: not reached), "label"}.  Blocks."""
        out = _lib.CostSite()
        self._ck(_lib.lib().volym_cost_at(self.handle, int(x), int(y), int(z), C.byref(out)))
        none = int(out.cost) == _lib.COST_NONE
        return {"cost": None if none else int(out.cost), "label": int(out.label)}

    def cost_device_ptr(self):
        """The context's own summary (a volym_cost_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_cost_device_ptr(self.handle)

    def cost_map_device_ptr(self):
        """The key map of the latest cost pass in device memory (None before any)."""
        return _lib.lib().volym_cost_map_device_ptr(self.handle)

    def spread_labels(self, spread):
        """One spread on the device (include/volym_hip.h volym_spread_labels; scene.spread_volume is its definition): a texel of the
        box whose label gives becomes to[g], g its cost label in the latest cost pass, where the take table, the density window and
        the band of cost say so.  `spread` is a scene.Spread.  Everything follows as after edit_labels, and the call is one step of
        the history.  Blocks.  Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_spread_labels(self.handle, C.byref(spread.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    # ---- fill between slices ----------------------------------------------------------------------
    def interpolate_pass(self, interpolate):
        """Enqueue one interpolate pass (include/volym_hip.h volym_interpolate_pass; scene.interpolate_volume is its definition): the
        key slices of the request's box along its axis, the signed planar distance of the selected shape on each of them, and for
        every texel of the slices between two keys whether the interpolated shape holds it.  `interpolate` is a scene.Interpolate."""
        self._ck(_lib.lib().volym_interpolate_pass(self.handle, C.byref(interpolate.to_c())))
        box = interpolate.box
        self._interpolate_box = box if all(a < b for a, b in zip(*box)) else None

    def read_interpolate(self):
        """The summary of the latest interpolate pass: an np.void of _lib.INTERPOLATE_SUMMARY_DTYPE.  Blocks."""
        out = np.zeros(1, _lib.INTERPOLATE_SUMMARY_DTYPE)
        self._ck(_lib.lib().volym_read_interpolate(self.handle, out.ctypes.data_as(C.POINTER(_lib.InterpolateSummary))))
        return out[0]

    def _read_interpolate_map(self, call, dtype, ctype, sub):
        box = getattr(self, "_interpolate_box", None) if sub is None else (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        if box is None:                                        # no pass yet (the library refuses), or a pass over an empty box
            self._ck(call(self.handle, None, None))
            return np.zeros((0, 0, 0), dtype)
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        out = np.zeros(tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0)), dtype)
        self._ck(call(self.handle, c, out.ctypes.data_as(C.POINTER(ctype))))
        return out

    def read_interpolate_map(self, sub=None):
        """The signed planar map of the latest interpolate pass as a uint32 array [z, y, x]: of its whole box (None) or of the sub-box
        (lo, hi) in texels of the volume, which must lie inside the pass's box.  On a key slice D << 1 | 1 inside the shape and
        D << 1 outside it; _lib.INTERPOLATE_NONE elsewhere.  Blocks."""
        return self._read_interpolate_map(_lib.lib().volym_read_interpolate_map, np.uint32, C.c_uint32, sub)

    def read_interpolate_state(self, sub=None):
        """The state bytes of the latest interpolate pass (_lib.INTERPOLATE_SHAPE | INSIDE | GAP) as a uint8 array [z, y, x], as
        read_interpolate_map.  Blocks."""
        return self._read_interpolate_map(_lib.lib().volym_read_interpolate_state, np.uint8, C.c_uint8, sub)

    def interpolate_at(self, x, y, z):
        """The signed word and the state byte of texel (x, y, z) in the latest interpolate pass: {"word", "state"}.  Blocks."""
        word, state = C.c_uint32(0), C.c_uint8(0)
        self._ck(_lib.lib().volym_interpolate_at(self.handle, int(x), int(y), int(z), C.byref(word), C.byref(state)))
        return {"word": int(word.value), "state": int(state.value)}

    def interpolate_device_ptr(self):
        """The context's own summary (a volym_interpolate_summary in device memory) after a pass (None before any)."""
        return _lib.lib().volym_interpolate_device_ptr(self.handle)

    def interpolate_map_device_ptr(self):
        """The signed map of the latest interpolate pass in device memory (None before any)."""
        return _lib.lib().volym_interpolate_map_device_ptr(self.handle)

    def interpolate_state_device_ptr(self):
        """The state map of the latest interpolate pass in device memory (None before any)."""
        return _lib.lib().volym_interpolate_state_device_ptr(self.handle)

    def interpolate_labels(self, edit):
        """One edit by the latest interpolate pass on the device (include/volym_hip.h volym_interpolate_labels;
        scene.interpolate_labels_volume is its definition): a texel of a gap slice in the box becomes to[label] where the interpolated
        shape holds it and out[label] where it does not, within the density window.  `edit` is a scene.InterpolateEdit.  Everything
        follows as after edit_labels, and the call is one step of the history.  Blocks.  Returns the result: an np.void of
        _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_interpolate_labels(self.handle, C.byref(edit.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    # ---- editing labels --------------------------------------------------------------------------
    def edit_labels(self, relabel):
        """One edit of the labels on the device (include/volym_hip.h volym_edit_labels; scene.relabel_volume is its definition):
        texels of the request's box become to[label] where the table, the density window, the ids of the latest components pass
        and the latest distance map say so.  `relabel` is a scene.Relabel.  Density, importances, label counts and boxes follow,
        as if the edited labels had been uploaded.  Blocks.  Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_edit_labels(self.handle, C.byref(relabel.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    def brush_labels(self, brush):
        """One stroke of the brush on the device (include/volym_hip.h volym_brush_labels; scene.brush_volume is its definition): the
        texels within the stroke's radius of its polyline become to[label] where the table, the box and the density window say so.
        `brush` is a scene.Brush.  Everything follows as after edit_labels, and the call is one step of the history.  Blocks.
        Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_brush_labels(self.handle, C.byref(brush.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    def lasso_labels(self, lasso):
        """One cut of the scissors on the device (include/volym_hip.h volym_lasso_labels; scene.lasso_volume is its definition): the
        texels that project into the polygon of `lasso` (a scene.Lasso) -- with LASSO_OUTSIDE, those that do not -- become to[label]
        where the table, the box and the density window say so.  Everything follows as after edit_labels, and the call is one step of
        the history.  Blocks.  Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_lasso_labels(self.handle, C.byref(lasso.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    def smooth_labels(self, smooth):
        """One pass of the majority filter on the device (include/volym_hip.h volym_smooth_labels; scene.smooth_volume is its
        definition): a texel of the box whose label gives becomes the label that wins the vote of its neighbourhood among its own
        and those that take, where the density window says so.  `smooth` is a scene.Smooth.  Everything follows as after
        edit_labels, and the call is one step of the history.  Blocks.  Returns the result: an np.void of _lib.RELABEL_RESULT_DTYPE."""
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(_lib.lib().volym_smooth_labels(self.handle, C.byref(smooth.to_c()), out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    def read_lasso_mask(self):
        """The polygon's bit plane of the latest lasso_labels (include/volym_hip.h volym_read_lasso_mask): (rect, words) -- rect =
        (x0, y0, x1, y1), hi exclusive, words = np.uint32[(y1 - y0) * ceil((x1 - x0) / 32)], as scene.lasso_mask_words lays them out."""
        rect = (C.c_uint32 * 4)()
        self._ck(_lib.lib().volym_read_lasso_mask(self.handle, rect, None, 0))
        x0, y0, x1, y1 = (int(v) for v in rect)
        words = np.zeros(((x1 - x0 + 31) // 32) * (y1 - y0), np.uint32)
        if words.size:
            self._ck(_lib.lib().volym_read_lasso_mask(self.handle, rect, words.ctypes.data_as(C.POINTER(C.c_uint32)), words.size))
        return (x0, y0, x1, y1), words

    def label_history(self, budget_bytes):
        """Keep a history of label edits in at most `budget_bytes` of device memory (20 bytes per changed 16-byte chunk); 0 drops
        and frees it (include/volym_hip.h volym_label_history; scene.LabelHistory is the definition of the bookkeeping)."""
        self._ck(_lib.lib().volym_label_history(self.handle, int(budget_bytes)))

    def _swap_labels(self, call):
        out = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)
        self._ck(call(self.handle, out.ctypes.data_as(C.POINTER(_lib.RelabelResult))))
        return out[0]

    def undo_labels(self):
        """Take the newest undoable edit back on the device.  Blocks.  Returns what the swap changed, an np.void of
        _lib.RELABEL_RESULT_DTYPE: the edit's result with left and arrived exchanged.  E_STATE: nothing to undo, history off."""
        return self._swap_labels(_lib.lib().volym_undo_labels)

    def redo_labels(self):
        """Carry the newest undone edit out again on the device.  Blocks.  Returns the edit's result."""
        return self._swap_labels(_lib.lib().volym_redo_labels)

    def label_history_info(self):
        """volym_label_history_info as a dict: budget_bytes, used_bytes, undo_steps, redo_steps, next_undo_records,
        next_redo_records, dropped_steps, lost."""
        info = _lib.LabelHistoryInfo()
        self._ck(_lib.lib().volym_label_history_info(self.handle, C.byref(info)))
        return info.as_dict()

    def read_labels(self, sub=None):
        """The labels on the device as a uint8 array [z, y, x]: the whole label volume (None) or the sub-box (lo, hi) in texels.
        Blocks."""
        if sub is None:
            dims = getattr(self, "_label_dims", None)
            if dims is None:                                   # no labels yet: the library refuses
                self._ck(_lib.lib().volym_read_labels(self.handle, None, None))
                return np.zeros((0, 0, 0), np.uint8)
            box = ((0, 0, 0), dims)
        else:
            box = (tuple(int(v) for v in sub[0]), tuple(int(v) for v in sub[1]))
        c = None if sub is None else (C.c_uint32 * 6)(*(list(box[0]) + list(box[1])))
        out = np.zeros(tuple(max(int(box[1][a]) - int(box[0][a]), 0) for a in (2, 1, 0)), np.uint8)
        self._ck(_lib.lib().volym_read_labels(self.handle, c, scene._u8p(out) if out.size else None))
        return out

    # ---- measurement ------------------------------------------------------------------------
    def stats_pass(self):
        s = _lib.Stats()
        self._ck(_lib.lib().volym_stats_pass(self.handle, C.byref(s)))
        return s.as_dict()

    def selftest_ray_setup(self):
        """(rays whose shared-reciprocal set-up differs from plain divisions, rays of waves that fell back, rays)."""
        out = (C.c_ulonglong * 3)()
        self._ck(_lib.lib().volym_selftest_ray_setup(self.handle, out))
        return int(out[0]), int(out[1]), int(out[2])

    def selftest_texel256(self):
        """(values on which the byte conversion in use differs from clamp(floor(x), 0, 255), NaNs on which it does, the same two counts
        for the conversion without a floor, values compared)."""
        out = (C.c_ulonglong * 5)()
        self._ck(_lib.lib().volym_selftest_texel256(self.handle, out))
        return tuple(int(v) for v in out)

    def texel_bytes_in_use(self):
        """whether the latest compute pass ran the kernel of 256-cubed volumes (VOLYM_OPT_TEXEL_BYTES)"""
        return bool(_lib.lib().volym_texel_bytes_in_use(self.handle))

    def time_batch(self, n):
        """n back-to-back passes between one pair of HIP events: total milliseconds."""
        ms = C.c_float(0.0)
        self._ck(_lib.lib().volym_time_batch(self.handle, int(n), C.byref(ms)))
        return float(ms.value)

    def time_passes(self, n):
        ms = np.zeros(int(n), np.float32)
        self._ck(_lib.lib().volym_time_passes(self.handle, int(n), scene._f32p(ms)))
        return ms


class ComputeDemo:
    """src/demos/mod.rs:9-17"""

    @classmethod
    def init(cls, ctx, state, **kw):
        raise NotImplementedError

    def update_gpu_state(self, ctx, state):
        raise NotImplementedError

    def compute_pass(self, ctx):
        raise NotImplementedError


class Simple(ComputeDemo):
    """src/demos/simple/mod.rs:35-121.  The reference hard-codes its asset paths
    (:40-55); here the caller passes raw bytes (a real .raw read from disk, or the
    synthetic stand-ins of volym_amd.synth) and the segments table."""

    def __init__(self, dims):
        self.dims = dims

    @classmethod
    def init(cls, ctx, state, volume_raw=None, labels_raw=None, segments=None, dims=(256, 256, 256),
             filter=_lib.FILTER_NEAREST, transfer_function=None):
        if volume_raw is None:   # the reference's default asset, synthesised (.MISSING_LARGE_BLOBS)
            volume_raw, labels_raw = synth.synth_teapot()
            segments = synth.TEAPOT_SEGMENTS
        if labels_raw is None:
            labels_raw = np.zeros(0, np.uint8)
        segments = scene.load_segments(segments if segments is not None else [])
        # GpuVolume::init (src/gpu_resources/volume.rs:35-101)
        volume = scene.prepare_volume(volume_raw, dims, flip_y=True)
        ctx.set_volume(volume, dims, filter)
        # GpuImportances::init (src/demos/simple/importance.rs:45-137): map, then pad/flip
        importances = scene.prepare_volume(scene.map_segments_to_importance(labels_raw, segments), dims, flip_y=True)
        ctx.set_importances(importances, dims)
        # TransferFunction::default() + bake (src/demos/simple/mod.rs:64-66)
        tf = transfer_function if transfer_function is not None else scene.TransferFunction.default()
        ctx.set_transfer_function(tf.bake_rgba8())
        self = cls(dims)
        self._labels_raw = np.ascontiguousarray(labels_raw, np.uint8).ravel()
        self._labels_on_device = False
        self._segments = segments
        self.update_gpu_state(ctx, state)   # GpuCamera::new / GpuParameters::new upload initial state
        return self

    def update_gpu_state(self, ctx, state):
        """BaseDemo::update_gpu_state (src/demos/pipeline.rs:208-212)"""
        ctx.update(state.camera_uniforms(), state.parameter_uniforms())
        self._records_for = None        # (highlight: the pick records of the old view are stale)
        self._camera_uniforms = state.camera_uniforms()                 # (lasso: the view of the latest frame)
        self._eye = tuple(float(v) for v in state.camera.position)      # (clip_at: the plane faces the eye)
        self._dense_step = 0.25 * float(state.parameter_uniforms().raymarching_step_size)      # (project: the march's dense step)

    def compute_pass(self, ctx):
        """BaseDemo::compute_pass -> DemoPipeline::compute_pass (src/demos/pipeline.rs:62-102, :214-225)"""
        ctx.compute_pass()

    def set_crop(self, ctx, lo01, hi01):
        """Crop box in unit-cube coordinates in [0, 1] (the cube the camera orbits; y as the prepared, flipped volume has it):
        texel = floor(p * n + 0.5) clamped to [0, n] (scene.crop_box_texels).  Returns the texel box."""
        lo, hi = scene.crop_box_texels(lo01, hi01, self.dims)
        ctx.set_crop_box(lo, hi)
        self._records_for = None
        return lo, hi

    def set_clip_plane(self, ctx, normal, point):
        """Oblique clip plane through `point` with the given normal, both in the unit-cube coordinates set_crop takes: what lies
        on the side the normal points to is cut away (scene.clip_plane_texels).  normal=None lifts the plane.  Returns the
        integer plane (n, d)."""
        n, d = ((0, 0, 0), 0) if normal is None else scene.clip_plane_texels(normal, point, self.dims)
        ctx.set_clip_plane(n, d)
        self._records_for = None
        return n, d

    def clip_at(self, ctx, x, y, alpha_min=0.5):
        """Click to cut: pick pixel (x, y), then set the clip plane through the picked texel's centre with the normal pointing
        from there to the eye, so that everything between the eye and the clicked point is cut away and the texel itself stays.
        Returns the plane (n, d), or None when the pixel shows nothing (the plane then stays as it is)."""
        p = self.pick(ctx, x, y, alpha_min)
        if p["status"] != "hit":
            return None
        n, _ = scene.clip_plane_texels([e - q for e, q in zip(self._eye, p["pos"])], p["pos"], self.dims)
        d = sum(a * t for a, t in zip(n, p["texel"]))       # exactly through the texel: it is kept
        ctx.set_clip_plane(n, d)
        self._records_for = None
        return n, d

    def set_hidden(self, ctx, hidden):
        """Hide the given segments and show all others (an editor's "hide the cup so that I can see the lobster").  `hidden`:
        ids of the segments JSON ("Segment_4") or raw label values (3), mixed freely.  The labels go to the device first if
        they are not there yet; the importances stay what they were.  Returns the hidden label values, sorted."""
        by_id = {s["id"]: s["label_value"] for s in getattr(self, "_segments", []) if "id" in s}
        values = set()
        for h in hidden:
            if isinstance(h, str):
                if h not in by_id:
                    raise ValueError("no segment with id %r" % h)
                values.add(by_id[h])
            else:
                values.add(int(h))
        mask = scene.visibility_mask(values)
        if not self._labels_on_device:
            if not values:
                return []
            self.set_labels(ctx, self._labels_raw)
        ctx.set_segment_visibility(mask)
        self._records_for = None
        return sorted(values)

    def _label_values(self, segments):
        """Label values of `segments`: names or ids of the segments JSON ("Canopy", "canopy") or raw label values, mixed freely"""
        by_key = {}
        for s in reversed(getattr(self, "_segments", [])):
            for k in ("name", "id"):
                if k in s:
                    by_key[s[k]] = s["label_value"]
        values = set()
        for h in segments:
            if isinstance(h, str):
                if h not in by_key:
                    raise ValueError("no segment with name or id %r" % h)
                values.add(by_key[h])
            else:
                values.add(int(h))
        return sorted(values)

    def _current_records(self, ctx, alpha_min):
        """A whole-frame pick pass, unless the records of one for the current view, scene and alpha_min are there already"""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        if getattr(self, "_records_for", None) != (id(ctx), float(alpha_min)):
            ctx.pick_pass(None, alpha_min)
            self._records_for = (id(ctx), float(alpha_min))
            self._records_host = None

    def highlight(self, ctx, segments, ring_rgba=(255, 255, 0, 255), fill_rgba=(255, 255, 0, 48), radius=2, alpha_min=0.5, target_ptr=None):
        """Outline and tint the given segments (names, ids or label values) in the frame of the latest compute pass: one outline
        pass over the records of a whole-frame pick pass, which runs only if the demo has none for the current view and scene
        (update_gpu_state, set_crop, set_clip_plane, set_hidden, set_segments and set_labels make the records stale).  A hover that moves to
        another segment costs the outline pass alone.  The image goes to target_ptr, or to the context's own target
        (ctx.read_outline()).  Returns the selected label values."""
        values = self._label_values(segments)
        self._current_records(ctx, alpha_min)
        ctx.outline_pass(scene.selection_mask(values), ring_rgba, fill_rgba, radius, target_ptr=target_ptr)
        return values

    def highlight_at(self, ctx, x, y, alpha_min=0.5, **kw):
        """Hover: outline the segment pixel (x, y) shows (nothing when it shows no labelled sample: the image is then the
        frame).  The label comes from the current records, which are read back once per view and scene: the hovers after
        the first cost the outline pass alone.  Returns what pick returns."""
        if not (0 <= int(x) < ctx.width and 0 <= int(y) < ctx.height):
            raise ValueError("pixel (%r, %r) is not inside the %d x %d frame" % (x, y, ctx.width, ctx.height))
        self._current_records(ctx, alpha_min)
        if self._records_host is None:
            self._records_host = ctx.read_picks()
        p = self._describe_pick(x, y, self._records_host[int(y), int(x)])
        self.highlight(ctx, [p["label"]] if p["status"] == "hit" and p["label"] is not None else [], alpha_min=alpha_min, **kw)
        return p

    def pick(self, ctx, x, y, alpha_min=0.5):
        """What pixel (x, y) of the frame shows: the first sample of its ray after which alpha >= alpha_min (GpuContext.pick), as
        a dict: status ("miss" / "none" / "hit"), label (None without labels), segment and segment_id (name and id of the segments
        JSON entry with that label value, else None), texel (x, y, z) in the prepared volume, pos (the texel's centre in the unit-cube coordinates
        set_crop takes), t (along the ray from the eye), alpha and density.  The labels go to the device first if they are not
        there yet (the importances stay what they were)."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        r = ctx.pick(x, y, alpha_min)
        self._records_for = None        # (the one-pixel pass took the place of a whole frame's records)
        return self._describe_pick(x, y, r)

    def _describe_pick(self, x, y, r):
        """the dict of pick for the record r of pixel (x, y)"""
        status = ("miss", "none", "hit")[int(r["status"])]
        out = {"x": int(x), "y": int(y), "status": status, "label": None, "segment": None, "segment_id": None, "texel": None, "pos": None, "t": None,
               "alpha": int(r["alpha8"]) / 255.0, "density": None}
        if status == "hit":
            texel = (int(r["x"]), int(r["y"]), int(r["z"]))
            out.update(texel=texel, pos=tuple((i + 0.5) / n for i, n in zip(texel, self.dims)), t=float(r["t"]), density=int(r["density"]))
            if int(r["has_labels"]):
                out["label"] = int(r["label"])
                seg = next((s for s in getattr(self, "_segments", []) if s["label_value"] == out["label"]), None)
                if seg is not None:
                    out["segment"], out["segment_id"] = seg.get("name"), seg.get("id")
        return out

    def segment_palette(self, strength=96):
        """A colour per label value of the segments JSON for the slice overlay (alpha = strength); every other label, 0 included,
        is left transparent.  The hues are spread by the golden angle over the label values, so that they do not depend on the
        order of the JSON."""
        import colorsys
        pal = np.zeros((256, 4), np.uint8)
        for s in getattr(self, "_segments", []):
            l = int(s["label_value"])
            if l:
                r, g, b = colorsys.hsv_to_rgb((l * 0.61803398875) % 1.0, 0.85, 1.0)
                pal[l] = (int(r * 255.0 + 0.5), int(g * 255.0 + 0.5), int(b * 255.0 + 0.5), int(strength))
        return pal

    def slice(self, ctx, axis, index, mode=_lib.SLICE_DENSITY, labels=True, mark_cut=True, uncut=False, palette=None,
              cut_rgba=(255, 0, 0, 96), background=(0, 0, 0, 255), target_ptr=None):
        """The slice view beside the 3-D picture: the plane normal to `axis` ("x", "y", "z") through texel `index` of the prepared
        volume, one texel per pixel (scene.slice_axis).  mode: the density bytes, the transfer function's colours (_lib.SLICE_TF)
        or the importances; labels: the segments as a colour overlay (segment_palette, or `palette`) -- the labels go to the device
        first if they are not there yet; mark_cut: the texels the crop box, the clip plane and the hidden segments remove are
        tinted with cut_rgba; uncut: show the density before the cuts, so that the tint lies over what was cut away.  One kernel,
        no update and no frame needed.  The image goes to target_ptr, or to the context's own target (ctx.read_slice()).
        Returns the scene.Slice, whose map scene.slice_texel inverts a click with."""
        flags = (_lib.SLICE_MARK_CUT if mark_cut else 0) | (_lib.SLICE_UNCUT if uncut else 0)
        if labels and (self._labels_on_device or self._labels_raw.size):
            if not self._labels_on_device:
                self.set_labels(ctx, self._labels_raw)
            flags |= _lib.SLICE_LABELS
        s = scene.slice_axis(axis, index, self.dims, mode=mode, flags=flags, palette=self.segment_palette() if palette is None else palette,
                             cut_rgba=cut_rgba, background=background)
        ctx.slice_pass(s, target_ptr)
        return s

    def slices_at(self, ctx, x, y, alpha_min=0.5, **kw):
        """Click to look inside: the three orthogonal slices through the texel pixel (x, y) of the frame shows.  Returns the pick
        (its "slices" entry: {"x": image, "y": image, "z": image}, each (height, width, 4) uint8, read back), or the pick alone
        with "slices" None when the pixel shows nothing.  Keywords go to slice."""
        p = self.pick(ctx, x, y, alpha_min)
        p["slices"] = self._slices_through(ctx, p["texel"], **kw) if p["status"] == "hit" else None
        return p

    def _slices_through(self, ctx, texel, **kw):
        """the three orthogonal slices through `texel`, read back: {"x": image, "y": image, "z": image}"""
        out = {}
        for a, axis in enumerate("xyz"):
            self.slice(ctx, axis, texel[a], **kw)
            out[axis] = ctx.read_slice()
        return out

    def project(self, ctx, mode, step=None, tf=False, labels=True, no_skip=False, palette=None, background=(0, 0, 0, 255), rect=None):
        """The projection view: maximum (_lib.PROJECT_MAX, or "MAX") or mean ("MEAN", the X-ray) intensity along the rays of the
        current view, through the scene as it stands.  step: the distance between samples, by default the march's dense step,
        0.25 * raymarching_step_size; tf: colour through the transfer function; labels (MAX only): the segment of the brightest
        sample as a colour overlay (segment_palette, or `palette`) -- the labels go to the device first if they are not there yet.
        Records and image go to the context's own buffers (ctx.read_projection(), ctx.read_projection_image()).  Returns the
        scene.Projection."""
        if isinstance(mode, str):
            if mode.upper() not in ("MAX", "MEAN"):
                raise ValueError("a projection mode is MAX or MEAN, got %r" % (mode,))
            mode = _lib.PROJECT_MEAN if mode.upper() == "MEAN" else _lib.PROJECT_MAX
        flags = (_lib.PROJECT_TF if tf else 0) | (_lib.PROJECT_NO_SKIP if no_skip else 0)
        if self._labels_raw.size and not self._labels_on_device:
            self.set_labels(ctx, self._labels_raw)              # (the records name the segment either way)
        if labels and mode == _lib.PROJECT_MAX and self._labels_on_device:
            flags |= _lib.PROJECT_LABELS
        p = scene.check_projection(scene.Projection(self._dense_step if step is None else step, mode, flags, background,
                                                    self.segment_palette() if palette is None else palette))
        ctx.project_pass(p, rect, own_image=True)
        return p

    def project_at(self, ctx, x, y, step=None):
        """The brightest sample of the ray of pixel (x, y) (GpuContext.project_at), as a dict: status ("miss" / "empty" / "hit"),
        max, mean, n_samples, and on a hit label (None without labels), segment and segment_id (name and id of the segments JSON
        entry with that label value, else None), texel (x, y, z) in the prepared volume, pos (the texel's centre in the unit-cube
        coordinates set_crop takes) and t (along the ray from the eye).  The labels go to the device first if they are not there
        yet."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        r = ctx.project_at(x, y, self._dense_step if step is None else step)
        status = ("miss", "empty", "hit")[int(r["status"])]
        out = {"x": int(x), "y": int(y), "status": status, "max": int(r["max"]), "mean": int(r["mean"]), "n_samples": int(r["n_samples"]),
               "label": None, "segment": None, "segment_id": None, "texel": None, "pos": None, "t": None}
        if status == "hit":
            texel = (int(r["x"]), int(r["y"]), int(r["z"]))
            out.update(texel=texel, pos=tuple((i + 0.5) / n for i, n in zip(texel, self.dims)), t=float(r["t"]))
            if self._labels_on_device:
                out["label"] = int(r["label"])
                seg = next((s for s in getattr(self, "_segments", []) if s["label_value"] == out["label"]), None)
                if seg is not None:
                    out["segment"], out["segment_id"] = seg.get("name"), seg.get("id")
        return out

    def brightest_slices_at(self, ctx, x, y, step=None, **kw):
        """Click the bright spot: the three orthogonal slices through the texel of the maximum along the ray of pixel (x, y).
        Returns what project_at returns with a "slices" entry as slices_at's; None when the ray shows nothing.  Keywords go to
        slice."""
        p = self.project_at(ctx, x, y, step)
        p["slices"] = self._slices_through(ctx, p["texel"], **kw) if p["status"] == "hit" else None
        return p

    def _segment_name(self, label):
        seg = next((s for s in getattr(self, "_segments", []) if s["label_value"] == label), None)
        return (seg.get("name") or seg.get("id")) if seg is not None else None

    def measure(self, ctx, segments=None, box01=None, uncut=False, spacing=(1, 1, 1)):
        """Measure segments of the scene as it stands (crop box, clip plane and hidden segments applied; uncut=True: as it was
        uploaded): one measure pass plus the read.  segments: names, ids or label values (None: every label value that has texels
        in view); box01: (lo, hi) in the unit-cube coordinates set_crop takes (None: the whole volume).  Returns {name: summary}
        in label order, the name being the segments JSON's, or "label N" for a value it does not list; a summary is
        scene.segment_summary's dict with "label" and "in_view" (the share of the segment's texels that were counted, from the
        label counts of the device) added, or None for a segment with no texel in view.  The labels go to the device first if they
        are not there yet; without labels everything is label 0."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        box = None if box01 is None else scene.crop_box_texels(box01[0], box01[1], self.dims)
        m = scene.check_measure(scene.Measure(box, _lib.MEASURE_UNCUT if uncut else 0, dims=self.dims), self.dims)
        ctx.measure_pass(m)
        rec, _ = ctx.read_measure()
        totals = ctx.label_counts() if self._labels_on_device else None
        values = self._label_values(segments) if segments is not None else [int(l) for l in np.flatnonzero(rec["count"])]
        out = {}
        for l in values:
            s = scene.segment_summary(rec[l], spacing)
            if s is not None:
                total = int(totals[l]) if totals is not None else self.dims[0] * self.dims[1] * self.dims[2]
                s.update(label=l, in_view=s["count"] / total if total else 0.0)
            out[self._segment_name(l) or "label %d" % l] = s
        return out

    def _surface_request(self, ctx, values, min_byte, box01, uncut):
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        box = None if box01 is None else scene.crop_box_texels(box01[0], box01[1], self.dims)
        select = None if values is None else scene.surface_select(values)
        return scene.check_surface(scene.Surface(box, _lib.SURFACE_UNCUT if uncut else 0, min_byte, select, dims=self.dims), self.dims)

    def surface(self, ctx, segments=None, min_byte=1, box01=None, uncut=False, spacing=(1, 1, 1)):
        """The surface of each of `segments` in the scene as it stands (crop box, clip plane and hidden segments applied; uncut=True:
        as it was uploaded): one surface pass per segment -- each selected alone, so that its surface is closed and includes the
        faces it shares with other segments -- one measure pass over the same box, and the reads.  segments: names, ids or label
        values (None: every label value that has texels in view); min_byte: 1..255, the density byte from which a texel is solid;
        box01: (lo, hi) in the unit-cube coordinates set_crop takes (None: the whole volume).  Returns {name: summary} in label
        order for every segment that has faces: scene.surface_summary's dict (faces, pairs, area, enclosed, volume, sphericity)
        with "measured", the measure pass's count of the segment's texels in the box -- equal to "enclosed" when min_byte is 1 and
        no texel of the segment in view has density 0.  The labels go to the device first if they are not there yet; without
        labels everything is label 0, the isosurface density >= min_byte."""
        s = self._surface_request(ctx, None, min_byte, box01, uncut)
        ctx.measure_pass(scene.Measure(s.box, _lib.MEASURE_UNCUT if uncut else 0, dims=self.dims))
        rec, _ = ctx.read_measure()
        values = self._label_values(segments) if segments is not None else [int(l) for l in np.flatnonzero(rec["count"])]
        out = {}
        for l in values:
            ctx.surface_pass(s.replace(select=scene.surface_select([l])))
            one = scene.surface_summary(ctx.read_surface(), l, spacing, rec[l])
            if one is not None:
                out[self._segment_name(l) or "label %d" % l] = one
        return out

    def surface_faces(self, ctx, segments=None, min_byte=1, box01=None, uncut=False):
        """The boundary of the union of `segments` (None: of every label) as face records in ascending (z, y, x, dir): one surface
        pass with all of them selected, one emit pass into the context's own buffer, and the reads.  Returns (summary, faces):
        the np.void of _lib.SURFACE_SUMMARY_DTYPE and the records of _lib.SURFACE_FACE_DTYPE (scene.surface_mesh makes the mesh)."""
        s = self._surface_request(ctx, None if segments is None else self._label_values(segments), min_byte, box01, uncut)
        ctx.surface_pass(s)
        ctx.surface_faces_pass()
        summary = ctx.read_surface()
        return summary, ctx.read_surface_faces(summary["total"])

    def surface_at(self, ctx, x, y, alpha_min=0.5, **kw):
        """Click for the surface: pick pixel (x, y), then the surface of the segment it shows.  Returns the pick with a "surface"
        entry (the summary of that segment, as surface gives it), None when the pixel shows no labelled sample or the segment has
        no face.  Keywords go to surface."""
        p = self.pick(ctx, x, y, alpha_min)
        p["surface"] = None
        if p["status"] == "hit" and p["label"] is not None:
            p["surface"] = next(iter(self.surface(ctx, [p["label"]], **kw).values()), None)
        return p

    def export_surface(self, ctx, path, segments=None, min_byte=1, box01=None, uncut=False, spacing=(1, 1, 1), origin=(0, 0, 0)):
        """Write the boundary of the union of `segments` (surface_faces) to `path`: binary STL or OBJ by the name's ending
        (mesh.write).  Vertices are at origin + texel corner * spacing.  Returns scene.surface_summary of all the selected labels
        together (None, and an empty mesh, without faces)."""
        from . import mesh
        summary, faces = self.surface_faces(ctx, segments, min_byte, box01, uncut)
        mesh.write(path, faces, spacing, origin)
        return scene.surface_summary(summary, None, spacing)

    def components(self, ctx, names=None, min_byte=1, box01=None, uncut=False, spacing=(1, 1, 1), below=8, max_components=0):
        """Is each segment one piece?  One components pass per segment of `names` (names, ids or label values; None: every label
        value that has texels in view), each selected alone as surface selects them, in the scene as it stands (uncut=True: as it
        was uploaded), and the reads of summary and table.  Returns {name: summary} in label order for every segment with a solid
        texel: {"label", "pieces", "solid" (its solid texels), "recorded", "largest", "share", "small" (scene.components_summary:
        the pieces of fewer than `below` texels), "top": the ten largest recorded pieces, largest first, as scene.component_dict
        gives them}.  The labels go to the device first if they are not there yet; without labels everything is label 0."""
        s = self._surface_request(ctx, None, min_byte, box01, uncut)
        flags = _lib.COMPONENTS_UNCUT if uncut else 0
        if names is not None:
            values = self._label_values(names)
        else:
            ctx.measure_pass(scene.Measure(s.box, _lib.MEASURE_UNCUT if uncut else 0, dims=self.dims))
            values = [int(l) for l in np.flatnonzero(ctx.read_measure()[0]["count"])]
        out = {}
        for l in values:
            ctx.components_pass(scene.check_components(scene.Components(s.box, flags, min_byte, scene.surface_select([l]), max_components), self.dims))
            summary = ctx.read_components()
            if not int(summary["n_solid"]):
                continue
            table = ctx.read_component_table(summary["recorded"])
            one = scene.components_summary(summary, table, spacing, below)[l]
            order = np.argsort(-table["count"].astype(np.int64), kind="stable")[:10]
            one.update(label=l, solid=int(summary["n_solid"]), top=[scene.component_dict(table[k], k, spacing) for k in order.tolist()])
            out[self._segment_name(l) or "label %d" % l] = one
        return out

    def component_at(self, ctx, x, y, alpha_min=0.5, min_byte=1, spacing=(1, 1, 1)):
        """Click for the piece: pick pixel (x, y), then one components pass for the segment it shows, selected alone, and one measure
        pass.  Returns the pick with a "component" entry: the record of the piece under the pixel (scene.component_dict) with
        "pieces" (how many the segment has) and "segment_count" (the segment's texels in view, from the measure pass) added; None
        when the pixel shows no labelled sample, the picked texel is not solid at min_byte, or the piece has no record."""
        p = self.pick(ctx, x, y, alpha_min)
        p["component"] = None
        if p["status"] == "hit" and p["label"] is not None:
            l = p["label"]
            ctx.components_pass(scene.Components(None, 0, min_byte, scene.surface_select([l]), dims=self.dims))
            number = ctx.component_of(*p["texel"])
            summary = ctx.read_components()
            if number != _lib.COMPONENT_NONE and number < int(summary["recorded"]):
                ctx.measure_pass(scene.Measure(dims=self.dims))
                rec, _ = ctx.read_measure()
                one = scene.component_dict(ctx.read_component_table(summary["recorded"])[number], number, spacing)
                one.update(pieces=int(summary["n_components"]), segment_count=int(rec["count"][l]))
                p["component"] = one
        return p

    def _distance_request(self, ctx, values, inside, min_byte, box01, uncut, spacing):
        s = self._surface_request(ctx, values, min_byte, box01, uncut)
        weights, unit = scene.distance_weights(spacing)
        flags = (_lib.DISTANCE_UNCUT if uncut else 0) | (_lib.DISTANCE_INSIDE if inside else 0)
        return scene.check_distance(scene.Distance(s.box, flags, min_byte, s.select, weights), self.dims), unit

    def distance(self, ctx, names=None, inside=False, min_byte=1, box01=None, uncut=False, spacing=(1, 1, 1)):
        """The distance map of the union of the segments `names` (names, ids or label values; None: every label) in the scene as it
        stands (uncut=True: as it was uploaded): one distance pass and the read of its summary; the map stays on the device for
        ctx.read_distance_map and ctx.distance_at.  inside=False: distances from the set, for margins and clearance; inside=True:
        distances to the set's complement, for thickness.  spacing: the texel spacing, integer multiples (1..8) of its smallest
        (scene.distance_weights).  Returns scene.distance_summary's dict -- distances in the units of `spacing` -- with "unit",
        "weights" and, in "clearance", the segments' names added.  The labels go to the device first if they are not there yet."""
        values = None if names is None else self._label_values(names)
        d, unit = self._distance_request(ctx, values, inside, min_byte, box01, uncut, spacing)
        ctx.distance_pass(d)
        out = scene.distance_summary(ctx.read_distance(), unit)
        out.update(unit=unit, weights=d.weight)
        for l, c in out["clearance"].items():
            c["segment"] = self._segment_name(l) or "label %d" % l
        return out

    def thickness(self, ctx, name, min_byte=1, box01=None, uncut=False, spacing=(1, 1, 1)):
        """Where is segment `name` thickest?  One INSIDE distance pass with the segment selected alone.  Returns {"at": the deepest
        texel (the first in ascending (z, y, x) of equals), "d2", "radius": the radius of the largest ball round it that fits
        inside the segment, in the units of `spacing`, "thickness": twice that, "solid": the segment's solid texels}; None when
        the segment has no solid texel."""
        out = self.distance(ctx, [name], True, min_byte, box01, uncut, spacing)
        if not out["n_solid"]:
            return None
        return {"at": out["max_at"], "d2": out["max_d2"], "radius": out["max"], "thickness": 2.0 * out["max"], "solid": out["n_solid"]}

    def clearance(self, ctx, a, b, min_byte=1, box01=None, uncut=False, spacing=(1, 1, 1)):
        """How close does segment `a` come to segment `b`?  Two distance passes: one with `a` selected, whose near_at[b] is the texel
        of `b` nearest to `a`; one with `b` selected, whose near_at[a] is its partner in `a` (both passes find the same smallest
        distance, and each texel is the first of equals in ascending (z, y, x) on its side).  Returns {"d2", "distance" (units of
        `spacing`), "at_a", "at_b"}; None when either segment has no present texel or `a` == `b`."""
        (la,), (lb,) = self._label_values([a]), self._label_values([b])
        if la == lb:
            return None
        from_a = self.distance(ctx, [la], False, min_byte, box01, uncut, spacing)["clearance"].get(lb)
        from_b = self.distance(ctx, [lb], False, min_byte, box01, uncut, spacing)["clearance"].get(la)
        if from_a is None or from_b is None:
            return None
        return {"d2": from_a["d2"], "distance": from_a["distance"], "at_a": from_b["at"], "at_b": from_a["at"]}

    def distance_at(self, ctx, x, y, alpha_min=0.5, inside=False, **kw):
        """Click for the distance map: pick pixel (x, y), then one distance pass for the segment it shows, selected alone.  Returns
        the pick with a "distance" entry (what distance gives, with "d2_here": D at the picked texel); None when the pixel shows
        no labelled sample.  Keywords go to distance."""
        p = self.pick(ctx, x, y, alpha_min)
        p["distance"] = None
        if p["status"] == "hit" and p["label"] is not None:
            one = self.distance(ctx, [p["label"]], inside, **kw)
            box = ctx._distance_box
            if box is not None and all(lo <= t < hi for t, lo, hi in zip(p["texel"], *box)):
                one["d2_here"] = ctx.distance_at(*p["texel"])
            p["distance"] = one
        return p

    def histogram(self, ctx, segments=None):
        """The density histogram of the visible scene (segments=None), or of the given segments (names, ids or label values) as far
        as they are visible: np.uint64[256], the curve a transfer-function editor draws behind its control points.  One measure
        pass plus the read."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        group = None if segments is None else scene.measure_groups(self._label_values(segments))
        ctx.measure_pass(scene.check_measure(scene.Measure(None, 0, group, dims=self.dims), self.dims))
        return ctx.read_measure()[1][0]

    def measure_at(self, ctx, x, y, alpha_min=0.5, **kw):
        """Click to measure: pick pixel (x, y), then measure the segment it shows.  Returns the pick with a "measure" entry (the
        summary of that segment, as measure gives it), None when the pixel shows no labelled sample.  Keywords go to measure."""
        p = self.pick(ctx, x, y, alpha_min)
        p["measure"] = None
        if p["status"] == "hit" and p["label"] is not None:
            p["measure"] = next(iter(self.measure(ctx, [p["label"]], **kw).values()))
        return p

    def hide_at(self, ctx, x, y, alpha_min=0.5):
        """Click to hide: pick pixel (x, y), then set_hidden with that label added to the hidden ones.  Returns the pick (its
        "hidden" entry: the label values hidden now); nothing changes when the pixel shows no labelled sample."""
        p = self.pick(ctx, x, y, alpha_min)
        hidden = [int(l) for l in np.flatnonzero(ctx.segment_visibility() == 0)] if self._labels_on_device else []
        if p["status"] == "hit" and p["label"] is not None:
            hidden = self.set_hidden(ctx, sorted(set(hidden) | {p["label"]}))
        p["hidden"] = hidden
        return p

    def set_labels(self, ctx, labels_raw):
        """Keep the label map on the device (new; the reference maps it once on the host), so that set_segments can change
        segment importances without mapping or uploading the volume again."""
        labels_raw = np.ascontiguousarray(labels_raw, np.uint8).ravel()
        ctx.set_labels(scene.prepare_volume(labels_raw, self.dims, flip_y=True), self.dims)
        self._labels_raw = labels_raw
        self._labels_on_device = True
        self._records_for = None
        self._segments_on_device = False        # (the table went with the old labels)
        self._labels_edited = False

    def set_segments(self, ctx, segments):
        """New segment importances for the labels of set_labels (an editor's "show me the lobster instead of the cup").
        The table runs on the device.  One case differs from the reference's flow: it maps labels BEFORE padding them to the
        volume (importance.rs:148-158, then volume.rs:38-61), so the padding of a label file shorter than the volume has
        importance 0 there, table[0] here.  When that matters (table[0] != 0 and padding exists) the host map runs instead."""
        segments = scene.load_segments(segments)
        table = scene.segment_table(segments)
        self._records_for = None
        padded = self._labels_raw.size < self.dims[0] * self.dims[1] * self.dims[2]
        if padded and table[0] != 0:
            if getattr(self, "_labels_edited", False):           # (the host copy predates the edits on the device)
                self._labels_raw, self._labels_edited = self._labels_from_device(ctx), False
            importances = scene.map_segments_to_importance(self._labels_raw, segments)
            ctx.set_importances(scene.prepare_volume(importances, self.dims, flip_y=True), self.dims)   # (drops the labels)
            self._labels_on_device = self._segments_on_device = False
            return
        if not self._labels_on_device:
            self.set_labels(ctx, self._labels_raw)
        ctx.set_segment_importances(table)
        self._segments_on_device = True

    # ---- editing labels: pick, then the pass, then the edit ---------------------------------------
    def _labels_from_device(self, ctx):
        """The labels on the device as raw bytes in the orientation prepare_volume read (the y flip undone)."""
        return np.ascontiguousarray(ctx.read_labels()[:, ::-1, :]).ravel()

    def _ready_to_edit(self, ctx):
        """Labels on the device and importances mapped from them through the segments' table, so that they follow an edit."""
        if not self._labels_raw.size and not self._labels_on_device:
            raise ValueError("the demo has no labels to edit")
        if not self._labels_on_device or not getattr(self, "_segments_on_device", False):
            self.set_segments(ctx, self._segments)
        if not self._labels_on_device:
            raise ValueError("the labels are shorter than the volume and label 0 is important: they cannot stay on the device")

    def _edit(self, ctx, relabel):
        result = ctx.edit_labels(scene.check_relabel(relabel, self.dims))
        if int(result["changed"]) and not relabel.flags & _lib.RELABEL_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def history(self, ctx, budget_mb=256):
        """Switch the history of label edits on (budget_mb megabytes of device memory; 0: off), so that undo and redo can take
        relabel, paint, split_at, keep_largest, grow, shrink and core back.  The labels go to the device first if they are not
        there: handing labels to the context clears the history, so this must come after them."""
        if budget_mb:
            self._ready_to_edit(ctx)
        ctx.label_history(int(budget_mb * (1 << 20)))

    def _swap(self, ctx, redo):
        if not ctx.label_history_info()["redo_steps" if redo else "undo_steps"]:
            return None
        result = ctx.redo_labels() if redo else ctx.undo_labels()
        self._labels_edited = True
        self._records_for = None
        return scene.relabel_result_dict(result)

    def undo(self, ctx):
        """Take the latest edit back on the device.  Returns scene.relabel_result_dict's dict of what changed (the edit's with left
        and arrived exchanged), or None when there is nothing to take back (history off, no step, or the step was evicted)."""
        return self._swap(ctx, False)

    def redo(self, ctx):
        """Carry the latest undone edit out again.  Returns its result's dict, or None when there is none."""
        return self._swap(ctx, True)

    def _new_segment(self, ctx, name, like):
        """The label value of segment `name`: that of the segments JSON entry of that name or id, or a new entry with the smallest
        label value that no entry names and no texel carries, and the importance of label `like`.  The table is re-sent."""
        if not isinstance(name, str):
            return int(name)
        for s in self._segments:
            if name in (s.get("name"), s.get("id")):
                return int(s["label_value"])
        used = {int(s["label_value"]) for s in self._segments}
        counts = ctx.label_counts()
        value = next((v for v in range(1, 256) if v not in used and not int(counts[v])), None)
        if value is None:
            raise ValueError("no label value is free for segment %r" % name)
        source = next((s for s in self._segments if s["label_value"] == like), None)
        self._segments = list(self._segments) + [{"id": "Segment_%d" % value, "name": name, "label_value": value,
                                                  "importance": int(source["importance"]) if source else 0}]
        self.set_segments(ctx, self._segments)
        return value

    def relabel(self, ctx, mapping, box01=None, window=(0, 255), uncut=False, dry_run=False):
        """Merge or swap segments by the table alone, or threshold-paint: every texel of a segment in `mapping` ({from: to}, names,
        ids or label values; `to` may name a new segment) inside box01 (unit-cube coordinates as set_crop takes them; None: the
        whole volume) whose density byte lies in `window` gets the new label.  Returns scene.relabel_result_dict's dict."""
        self._ready_to_edit(ctx)
        table = {}
        for old, new in mapping.items():
            (l,) = self._label_values([old])
            table[l] = self._new_segment(ctx, new, l)
        box = None if box01 is None else scene.crop_box_texels(box01[0], box01[1], self.dims)
        flags = (_lib.RELABEL_UNCUT if uncut else 0) | (_lib.RELABEL_DRY_RUN if dry_run else 0)
        return self._edit(ctx, scene.Relabel(box, flags, window, table, dims=self.dims))

    def paint(self, ctx, name, window, box01=None, over=(0,), uncut=False):
        """Threshold-paint: the texels of the segments `over` (default: the unlabelled ones) inside box01 whose density byte lies in
        `window` = (min_byte, max_byte) join segment `name`."""
        return self.relabel(ctx, {o: name for o in over}, box01, window, uncut)

    def split_at(self, ctx, x, y, name, alpha_min=0.5, min_byte=1):
        """Click to split: pick pixel (x, y), one components pass for the segment it shows, selected alone, and the piece under the
        pixel becomes segment `name` (a name or id of the segments JSON, a label value, or a new name, which gets an entry with
        the source's importance).  Returns the pick with a "relabel" entry (the result's dict, "label": the piece's new label);
        None there when the pixel shows no labelled sample or the picked texel is not solid at min_byte."""
        self._ready_to_edit(ctx)
        p = self.pick(ctx, x, y, alpha_min)
        p["relabel"] = None
        if p["status"] == "hit" and p["label"] is not None:
            l = p["label"]
            ctx.components_pass(scene.Components(None, 0, min_byte, scene.surface_select([l]), dims=self.dims))
            k = ctx.component_of(*p["texel"])
            if k != _lib.COMPONENT_NONE:
                value = self._new_segment(ctx, name, l)
                p["relabel"] = self._edit(ctx, scene.Relabel(None, _lib.RELABEL_IDS, to={l: value}, ids=(k, k), dims=self.dims))
                p["relabel"]["label"] = value
        return p

    def keep_largest(self, ctx, name, rest=0, min_byte=1):
        """Keep the largest piece of segment `name` and send its other pieces to `rest` (a segment, or label 0): one components pass
        with the segment selected alone, then the edit with IDS_EXCEPT.  Returns the result's dict with "pieces" and "kept" (the
        largest piece's number) added; None when the segment has no solid texel."""
        self._ready_to_edit(ctx)
        (l,) = self._label_values([name])
        ctx.components_pass(scene.Components(None, 0, min_byte, scene.surface_select([l]), dims=self.dims))
        summary = ctx.read_components()
        if not int(summary["recorded"]):
            return None
        k = int(np.argmax(ctx.read_component_table(summary["recorded"])["count"]))
        to = self._new_segment(ctx, rest, l)
        out = self._edit(ctx, scene.Relabel(None, _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT, to={l: to}, ids=(k, k), dims=self.dims))
        out.update(pieces=int(summary["n_components"]), kept=k)
        return out

    def _band(self, unit, r):
        """the largest D with sqrt(D) * unit <= r"""
        return int(np.floor((float(r) / unit) ** 2 + 1e-9))

    def grow(self, ctx, name, r, into=(0,), spacing=(1, 1, 1), min_byte=1):
        """Grow segment `name` by a margin of r (units of `spacing`) into the segments `into` (default: the unlabelled texels): one
        distance pass from the segment, then the texels of `into` at a distance of at most r join it."""
        self._ready_to_edit(ctx)
        (l,) = self._label_values([name])
        d, unit = self._distance_request(ctx, [l], False, min_byte, None, False, spacing)
        ctx.distance_pass(d)
        table = {v: l for v in self._label_values(into) if v != l}
        return self._edit(ctx, scene.Relabel(None, _lib.RELABEL_DISTANCE, to=table, d2=(0, self._band(unit, r)), dims=self.dims))

    def shrink(self, ctx, name, r, to=0, spacing=(1, 1, 1), min_byte=1):
        """Shrink segment `name` by r (units of `spacing`): one INSIDE distance pass, then its texels within r of its outside go to
        `to` (a segment, or label 0)."""
        self._ready_to_edit(ctx)
        (l,) = self._label_values([name])
        d, unit = self._distance_request(ctx, [l], True, min_byte, None, False, spacing)
        ctx.distance_pass(d)
        return self._edit(ctx, scene.Relabel(None, _lib.RELABEL_DISTANCE, to={l: self._new_segment(ctx, to, l)}, d2=(0, self._band(unit, r)), dims=self.dims))

    def core(self, ctx, name, r, to, spacing=(1, 1, 1), min_byte=1):
        """The thick core of segment `name`: its texels deeper than r (units of `spacing`) inside it become segment `to`."""
        self._ready_to_edit(ctx)
        (l,) = self._label_values([name])
        d, unit = self._distance_request(ctx, [l], True, min_byte, None, False, spacing)
        ctx.distance_pass(d)
        return self._edit(ctx, scene.Relabel(None, _lib.RELABEL_DISTANCE, to={l: self._new_segment(ctx, to, l)},
                                             d2=(self._band(unit, r) + 1, _lib.DISTANCE_NONE - 1), dims=self.dims))

    def _nearest_request(self, ctx, values, min_byte, spacing):
        weights, unit = scene.distance_weights(spacing)
        return scene.check_nearest(scene.Distance(None, 0, min_byte, scene.surface_select(values), weights, dims=self.dims), self.dims), unit

    def nearest(self, ctx, names=None, min_byte=1, spacing=(1, 1, 1)):
        """Which segment is nearest?  One nearest pass from the union of the segments `names` (names, ids or label values; None:
        every label but 0) and the read of its summary; the maps stay on the device for ctx.read_nearest_sites,
        ctx.read_nearest_labels, ctx.nearest_at and a fill.  Returns scene.nearest_summary's dict, the cells by segment name ("label
        N" for a value the segments JSON does not list): "texels" of the volume are nearest to the segment, "fill" of them are
        present and in none of the segments.  The labels go to the device first if they are not there yet."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        values = list(range(1, 256)) if names is None else self._label_values(names)
        d, unit = self._nearest_request(ctx, values, min_byte, spacing)
        ctx.nearest_pass(d)
        out = scene.nearest_summary(ctx.read_nearest(), {l: self._segment_name(l) or "label %d" % l for l in range(256)})
        out.update(unit=unit, weights=d.weight)
        return out

    def _fill(self, ctx, fill):
        result = ctx.fill_labels(scene.check_fill(fill, self.dims))
        if int(result["changed"]) and not fill.flags & _lib.FILL_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def fill(self, ctx, names=None, r=None, into=(0,), window=(0, 255), spacing=(1, 1, 1), min_byte=1):
        """Grow several segments at once: one nearest pass from the union of `names` (names, ids or label values; None: every label
        but those of `into`), then one fill -- every texel of the segments `into` (default: the unlabelled texels) with a density
        byte in `window` joins the segment it is nearest to, the first in (z, y, x) among equals, if that is at most r away (units of
        `spacing`; None: however far).  One call, one undo step.  Returns the result's dict."""
        self._ready_to_edit(ctx)
        gives = self._label_values(into)
        seeds = [l for l in (range(256) if names is None else self._label_values(names)) if l not in gives]
        d, unit = self._nearest_request(ctx, seeds, min_byte, spacing)
        ctx.nearest_pass(d)
        band = (0, 0xFFFFFFFF if r is None else self._band(unit, r))
        return self._fill(ctx, scene.Fill(None, 0, window, scene.smooth_table(gives), scene.smooth_table(seeds), band, dims=self.dims))

    def separate(self, ctx, name, r, most=8, spacing=(1, 1, 1), min_byte=1):
        """Separate touching objects of segment `name`: its core at depth r (units of `spacing`) falls into pieces, the `most`
        largest of them become segments "<name> 1", "<name> 2", ... (largest first), the rest of the core goes back, and what is
        left of `name` goes to the piece it is nearest to.  A composition: core, one components pass, the edits by id, one nearest
        pass from the new labels and one fill -- each edit an undo step of its own.  Returns [{"name", "label", "texels"}, ...] of the
        pieces after the fill, largest core first; [] when the segment has no core that deep."""
        self._ready_to_edit(ctx)
        (l,) = self._label_values([name])
        base = self._segment_name(l) or "label %d" % l
        first = self._new_segment(ctx, "%s 1" % base, l)
        self.core(ctx, l, r, first, spacing, min_byte)
        ctx.components_pass(scene.Components(None, 0, min_byte, scene.surface_select([first]), dims=self.dims))
        summary = ctx.read_components()
        if not int(summary["recorded"]):
            return []
        counts = ctx.read_component_table(summary["recorded"])["count"].astype(np.int64)
        order = np.argsort(-counts, kind="stable")[:max(int(most), 1)].tolist()
        pieces = [first]
        for rank, k in enumerate(order[1:], 2):
            value = self._new_segment(ctx, "%s %d" % (base, rank), l)
            self._edit(ctx, scene.Relabel(None, _lib.RELABEL_IDS, to={first: value}, ids=(k, k), dims=self.dims))
            pieces.append(value)
        # what still carries the first piece's label and is not that piece: the pieces beyond `most`
        self._edit(ctx, scene.Relabel(None, _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT, to={first: l}, ids=(order[0], order[0]), dims=self.dims))
        d, _unit = self._nearest_request(ctx, pieces, min_byte, spacing)
        ctx.nearest_pass(d)
        self._fill(ctx, scene.Fill(None, 0, (0, 255), scene.smooth_table([l]), scene.smooth_table(pieces), dims=self.dims))
        after = ctx.label_counts()
        return [{"name": self._segment_name(v), "label": v, "texels": int(after[v])} for v in pieces]

    # ---- geodesic growth: steps through the matter ------------------------------------------------
    def _flood(self, ctx, flood):
        result = ctx.flood_labels(scene.check_flood(flood, self.dims))
        if int(result["changed"]) and not flood.flags & _lib.FLOOD_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def reach(self, ctx, names, through=(0,), window=(1, 255), r=None):
        """How far through the matter?  One geodesic pass from the union of the segments `names` (names, ids or label values; None:
        every label but those of `through`) through the segments `through` (default: the unlabelled texels) with a density byte in
        `window`, at most r steps (None: however far), and the read of its summary; the map stays on the device for
        ctx.read_geodesic_map, ctx.geodesic_at and a flood.  Returns scene.geodesic_summary's dict, the cells by segment name.  The
        labels go to the device first if they are not there yet."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        medium = self._label_values(through)
        seeds = [l for l in (range(256) if names is None else self._label_values(names)) if l not in medium]
        g = scene.check_geodesic(scene.Geodesic(None, 0, window, scene.smooth_table(seeds), scene.smooth_table(medium), 0 if r is None else int(r), dims=self.dims), self.dims)
        ctx.geodesic_pass(g)
        return scene.geodesic_summary(ctx.read_geodesic(), {l: self._segment_name(l) or "label %d" % l for l in range(256)})

    def grow_through(self, ctx, names, r, into=(0,), window=(1, 255)):
        """Grow several segments at once, each only through matter it touches: one geodesic pass from the union of `names` (None:
        every label but those of `into`) through the segments `into` with a density byte in `window`, at most r steps (None:
        however far), then one flood -- every texel reached joins the segment whose seed is the fewest steps away, the smallest label
        among equals.  Where Simple.fill measures straight through anything, this stays inside the matter: an air gap is no
        bridge.  One undo step.  Returns the result's dict."""
        self._ready_to_edit(ctx)
        gives = self._label_values(into)
        seeds = [l for l in (range(256) if names is None else self._label_values(names)) if l not in gives]
        limit = 0 if r is None else int(r)
        if limit < 0 or (r is not None and limit == 0):
            raise ValueError("grow_through: r is at least 1 step, or None")
        ctx.geodesic_pass(scene.check_geodesic(scene.Geodesic(None, 0, window, scene.smooth_table(seeds), scene.smooth_table(gives), limit, dims=self.dims), self.dims))
        return self._flood(ctx, scene.Flood(None, 0, (0, 255), scene.smooth_table(gives), scene.smooth_table(seeds), None, (1, 0xFFFFFFFF), dims=self.dims))

    def wand_at(self, ctx, x, y, name, tolerance, r=None, over=(0,), alpha_min=0.5):
        """The magic wand: pick pixel (x, y); the texel it shows is the one seed of a geodesic pass through the segments `over`
        (default: the unlabelled texels) whose density byte lies within `tolerance` of the picked texel's, at most r steps (None:
        however far); everything reached joins segment `name` (a name or id of the segments JSON, a label value, or a new name, as
        in split_at), the picked texel included where its label is one of `over`.  Returns the pick with a "relabel" entry (the
        result's dict, "label": the segment's label, "window"); None there when the pixel shows nothing."""
        self._ready_to_edit(ctx)
        p = self.pick(ctx, x, y, alpha_min)
        p["relabel"] = None
        if p["status"] == "hit" and p["texel"] is not None:
            medium = self._label_values(over)
            window = (max(int(p["density"]) - int(tolerance), 0), min(int(p["density"]) + int(tolerance), 255))
            value = self._new_segment(ctx, name, p["label"] or 0)
            ctx.geodesic_pass(scene.check_geodesic(scene.Geodesic(None, 0, window, scene.smooth_table([]), scene.smooth_table(medium), 0 if r is None else int(r),
                                                                  [p["texel"]], dims=self.dims), self.dims))
            # the seed carries the picked texel's label, whatever it is: every geo label takes, and all of them become `value`
            p["relabel"] = self._flood(ctx, scene.Flood(None, 0, (0, 255), scene.smooth_table(medium), None, np.full(256, value, np.int64), dims=self.dims))
            p["relabel"].update(label=value, window=window)
        return p

    # ---- grow from seeds: cost-weighted growth ------------------------------------------------------
    def _spread(self, ctx, spread):
        result = ctx.spread_labels(scene.check_spread(spread, self.dims))
        if int(result["changed"]) and not spread.flags & _lib.SPREAD_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def _cost_request(self, seeds, medium, contrast, step, window, max_cost, points=()):
        limit = 0 if max_cost is None else int(max_cost)
        return scene.check_cost(scene.Cost(None, 0, window, scene.smooth_table(seeds), scene.smooth_table(medium), step, contrast, limit, points, 8, dims=self.dims), self.dims)

    def cost_reach(self, ctx, names, through=(0,), contrast=16, step=1, window=(1, 255), max_cost=0):
        """How cheaply through the matter?  One cost pass from the union of the segments `names` (names, ids or label values; None:
        every label but those of `through`) through the segments `through` (default: the unlabelled texels) with a density byte in
        `window`, where a step costs step + contrast * |change of density byte|, at most max_cost in all (0: however much), and the
        read of its summary; the map stays on the device for ctx.read_cost_map, ctx.cost_at and a spread.  Returns
        scene.cost_summary's dict, the cells by segment name.  The labels go to the device first if they are not there yet."""
        if not self._labels_on_device and self._labels_raw.size:
            self.set_labels(ctx, self._labels_raw)
        medium = self._label_values(through)
        seeds = [l for l in (range(256) if names is None else self._label_values(names)) if l not in medium]
        ctx.cost_pass(self._cost_request(seeds, medium, contrast, step, window, max_cost))
        return scene.cost_summary(ctx.read_cost(), {l: self._segment_name(l) or "label %d" % l for l in range(256)})

    def grow_from_seeds(self, ctx, names, into=(0,), contrast=16, step=1, window=(1, 255), max_cost=0):
        """Grow from seeds: one cost pass from the union of `names` (None: every label but those of `into`) through the segments
        `into` with a density byte in `window`, then one spread -- every texel of `into` that is reached goes to the segment that
        reaches it most cheaply, the smallest label among equals.  Where grow_through lets two segments meet halfway in steps, here
        they meet where the density changes: crossing a boundary costs contrast per byte of change.  One undo step.  Returns the
        result's dict."""
        self._ready_to_edit(ctx)
        gives = self._label_values(into)
        seeds = [l for l in (range(256) if names is None else self._label_values(names)) if l not in gives]
        ctx.cost_pass(self._cost_request(seeds, gives, contrast, step, window, max_cost))
        return self._spread(ctx, scene.Spread(None, 0, (0, 255), scene.smooth_table(gives), scene.smooth_table(seeds), None, (1, 0xFFFFFFFF), dims=self.dims))

    def smart_wand_at(self, ctx, x, y, name, contrast, max_cost, step=1, over=(0,), window=(1, 255), alpha_min=0.5):
        """The wand that stops at edges rather than at a tolerance: pick pixel (x, y); the texel it shows is the one seed of a cost
        pass through the segments `over` (default: the unlabelled texels) in `window`, and everything it reaches for at most max_cost
        joins segment `name` (a name or id of the segments JSON, a label value, or a new name, as in split_at), the picked texel
        included where its label is one of `over`.  Returns the pick with a "relabel" entry (the result's dict and "label": the
        segment's label); None there when the pixel shows nothing."""
        self._ready_to_edit(ctx)
        p = self.pick(ctx, x, y, alpha_min)
        p["relabel"] = None
        if p["status"] == "hit" and p["texel"] is not None:
            medium = self._label_values(over)
            value = self._new_segment(ctx, name, p["label"] or 0)
            ctx.cost_pass(self._cost_request([], medium, contrast, step, window, max_cost, [p["texel"]]))
            # the seed carries the picked texel's label, whatever it is: every cost label takes, and all of them become `value`
            p["relabel"] = self._spread(ctx, scene.Spread(None, 0, (0, 255), scene.smooth_table(medium), None, np.full(256, value, np.int64), dims=self.dims))
            p["relabel"].update(label=value)
        return p

    # ---- fill between slices ----------------------------------------------------------------------
    def fill_between(self, ctx, names, axis, max_gap=0, keys=None, replace=False, min_byte=0, spacing=(1, 1, 1)):
        """Fill between slices: each segment of `names` (names, ids or label values), painted on some slices perpendicular to `axis`
        ("x", "y", "z" or 0, 1, 2), is interpolated across the slices between them -- one interpolate pass and one edit per segment,
        each one undo step.  The unlabelled texels the interpolated shape holds join the segment.  max_gap: gaps of more slices are
        left alone (0: no limit); keys: the slices (volume coordinates along axis) that count as painted -- the way to redo a fill
        after a key slice was repainted, when the slices filled last time must not count; None: every slice that holds the segment;
        replace: texels of the segment on the filled slices that the shape does not hold go back to label 0.  Nothing joins shapes that
        do not overlap when seen along the axis: each only shrinks towards the other key inside its own outline.  Returns [{"name", "label", "summary", "relabel"}] per segment."""
        self._ready_to_edit(ctx)
        weights, _unit = scene.distance_weights(spacing)
        flags = 0 if keys is None else _lib.INTERPOLATE_KEYS
        out = []
        for l in self._label_values(names):
            q = scene.check_interpolate(scene.Interpolate(None, flags, min_byte, scene.surface_select([l]), weights, axis, max_gap, keys or (), dims=self.dims), self.dims)
            ctx.interpolate_pass(q)
            edit = scene.check_interpolate_edit(scene.InterpolateEdit(None, 0, (0, 255), {0: l}, {l: 0} if replace else None, dims=self.dims), self.dims)
            result = ctx.interpolate_labels(edit)
            if int(result["changed"]):
                self._labels_edited = True
                self._records_for = None
            out.append({"name": self._segment_name(l) or "label %d" % l, "label": l, "summary": scene.interpolate_summary(ctx.read_interpolate()),
                        "relabel": scene.relabel_result_dict(result)})
        return out

    def fill_between_at(self, ctx, x, y, axis, max_gap=0, alpha_min=0.5):
        """Fill between slices for the segment under pixel (x, y): pick, then fill_between of the label the pixel shows.  Returns the
        pick with a "fill_between" entry (fill_between's entry for the segment); None there when the pixel shows nothing or an
        unlabelled texel."""
        self._ready_to_edit(ctx)
        p = self.pick(ctx, x, y, alpha_min)
        p["fill_between"] = None
        if p["status"] == "hit" and p["texel"] is not None and p["label"]:
            p["fill_between"] = self.fill_between(ctx, [int(p["label"])], axis, max_gap)[0]
        return p

    def _brush(self, ctx, brush):
        result = ctx.brush_labels(scene.check_brush(brush, self.dims))
        if int(result["changed"]) and not brush.flags & _lib.BRUSH_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def _brush_table(self, ctx, name, over):
        """the table of a stroke that paints segment `name` (None: erases to label 0) over the segments `over` (None: every label)"""
        sources = list(range(256)) if over is None else self._label_values(over)
        value = 0 if name is None else self._new_segment(ctx, name, sources[0] if sources else 0)
        return {l: value for l in sources if l != value}

    def stroke(self, ctx, pixels, name, radius, over=(0,), window=(0, 255), spacing=(1, 1, 1), alpha_min=0.5, uncut=False):
        """Paint along a drag: one pick pass over the rect of `pixels` [(x, y), ...], then the texels within `radius` (texels of the
        finest axis of `spacing`) of the polyline of the picked texels, of the segments `over` (names, ids or label values; None:
        every label) and with a density byte in `window`, join segment `name` (as split_at takes it; None erases to label 0).  A
        pixel without a pick breaks the polyline: the next picked point starts a new piece of it.  More than 256 picked points
        become several calls of the brush, the last point of one repeated as the first of the next -- and EACH CALL IS AN UNDO
        STEP of its own.  Returns {"picked", "missed", "calls", "relabel": the results' dicts summed (changed, left, arrived; box:
        the hull), None when no pixel picks}."""
        self._ready_to_edit(ctx)
        pixels = [(int(x), int(y)) for x, y in pixels]
        if not pixels:
            raise ValueError("a stroke needs at least one pixel")
        for x, y in pixels:
            if not (0 <= x < ctx.width and 0 <= y < ctx.height):
                raise ValueError("pixel (%r, %r) is not inside the %d x %d frame" % (x, y, ctx.width, ctx.height))
        x0, y0 = min(p[0] for p in pixels), min(p[1] for p in pixels)
        ctx.pick_pass((x0, y0, max(p[0] for p in pixels) - x0 + 1, max(p[1] for p in pixels) - y0 + 1), alpha_min)
        records = ctx.read_picks()
        self._records_for = None        # (the rect's pass took the place of a whole frame's records)
        points, lift = [], False
        for x, y in pixels:
            r = records[y - y0, x - x0]
            if int(r["status"]) != _lib.PICK_HIT:
                lift = True
                continue
            points.append((int(r["x"]), int(r["y"]), int(r["z"]), _lib.BRUSH_LIFT if lift and points else 0))
            lift = False
        out = {"picked": len(points), "missed": len(pixels) - len(points), "calls": 0, "relabel": None}
        if not points:
            return out
        weights, unit = scene.distance_weights(spacing)
        table = self._brush_table(ctx, name, over)
        flags = _lib.BRUSH_UNCUT if uncut else 0
        total = None
        first = 0
        while first < len(points):
            part = points[first:first + _lib.BRUSH_MAX_POINTS]
            part[0] = part[0][:3] + (0,)
            res = self._brush(ctx, scene.Brush(part, self._band(1.0, radius), None, flags, window, table, weights, dims=self.dims))
            out["calls"] += 1
            if total is None:
                total = res
            elif res["changed"]:
                for k in ("left", "arrived"):
                    for l, v in res[k].items():
                        total[k][l] = total[k].get(l, 0) + v
                total["box"] = res["box"] if total["box"] is None else (tuple(min(a, b) for a, b in zip(total["box"][0], res["box"][0])),
                                                                       tuple(max(a, b) for a, b in zip(total["box"][1], res["box"][1])))
                total["changed"] += res["changed"]
            if first + _lib.BRUSH_MAX_POINTS >= len(points):
                break
            first += _lib.BRUSH_MAX_POINTS - 1                          # the last point again: the capsule to the next one
        out["relabel"] = total
        return out

    def brush_at(self, ctx, x, y, name, radius, over=(0,), window=(0, 255), spacing=(1, 1, 1), alpha_min=0.5):
        """Click to paint: pick pixel (x, y) and paint a ball of `radius` (texels of the finest axis of `spacing`; round in the units
        of `spacing`) at the picked texel, as stroke paints: the texels of the segments `over` with a density byte in `window` join
        segment `name` (None erases to label 0).  One call of the brush, one undo step.  Returns the pick with a "relabel" entry (the
        result's dict; None when the pixel shows no sample)."""
        self._ready_to_edit(ctx)
        p = self.pick(ctx, x, y, alpha_min)
        p["relabel"] = None
        if p["status"] == "hit":
            weights, unit = scene.distance_weights(spacing)
            table = self._brush_table(ctx, name, over)
            p["relabel"] = self._brush(ctx, scene.Brush([p["texel"]], self._band(1.0, radius), None, 0, window, table, weights, dims=self.dims))
        return p

    def _lasso(self, ctx, lasso):
        result = ctx.lasso_labels(scene.check_lasso(lasso, self.dims))
        if int(result["changed"]) and not lasso.flags & _lib.LASSO_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def lasso_view(self, ctx, depth=None):
        """The integer view of the latest frame's camera (scene.lasso_view); depth: None, or (front, back) along the view axis in the
        unit cube's units (back None: no far end)."""
        view = scene.lasso_view(self._camera_uniforms, ctx.width, ctx.height, self.dims)
        if depth is not None:
            view = scene.lasso_view_depth(view, depth[0], float("inf") if depth[1] is None else depth[1])
        return view

    def lasso(self, ctx, pixels, name, over=(0,), window=(0, 255), depth=None, outside=False, uncut=False):
        """Scissors: the texels that the latest frame's view projects into the polygon `pixels` [(x, y), ...] (3 to 1024 vertices,
        closed implicitly, even-odd; they may lie off screen), through the whole volume or the range `depth` = (front, back) along the
        view axis, of the segments `over` (names, ids or label values; None: every label) and with a density byte in `window`, join
        segment `name` (as split_at takes it; None erases to label 0).  outside: the texels that do NOT project into the polygon
        instead -- "keep only what is under the lasso".  One call, one undo step.  Returns the result's dict."""
        self._ready_to_edit(ctx)
        flags = (_lib.LASSO_OUTSIDE if outside else 0) | (_lib.LASSO_UNCUT if uncut else 0)
        table = self._brush_table(ctx, name, over)
        return self._lasso(ctx, scene.Lasso(pixels, self.lasso_view(ctx, depth), None, flags, window, table, dims=self.dims))

    def lasso_erase(self, ctx, pixels, over=None, window=(0, 255), depth=None, outside=False, uncut=False):
        """lasso with target label 0: what is under the polygon (outside: what is not) becomes unlabelled; over None: every label."""
        return self.lasso(ctx, pixels, None, over, window, depth, outside, uncut)

    def lasso_to_pick(self, ctx, pixels, name, thickness, over=None, alpha_min=0.5):
        """Cut only a slab behind the surface the user sees: pick the polygon's first vertex, and lasso from the picked texel's depth
        to `thickness` texels (of the volume's longest axis) behind it.  Returns the pick with a "relabel" entry (the result's dict;
        None when the pixel shows no sample)."""
        self._ready_to_edit(ctx)
        pixels = [(int(x), int(y)) for x, y in pixels]
        p = self.pick(ctx, pixels[0][0], pixels[0][1], alpha_min)
        p["relabel"] = None
        if p["status"] == "hit":
            view = self.lasso_view(ctx)
            t = [2 * v + 1 for v in p["texel"]]
            front = float(sum(view.m[2][a] * t[a] for a in range(3)) + view.c[2]) * 2.0 ** -view.scale_log2      # the texel's own D, in world units
            view = scene.lasso_view_depth(view, front, front + float(thickness) / max(self.dims))
            p["relabel"] = self._lasso(ctx, scene.Lasso(pixels, view, None, 0, (0, 255), self._brush_table(ctx, name, over), dims=self.dims))
        return p

    def _smooth(self, ctx, smooth):
        result = ctx.smooth_labels(scene.check_smooth(smooth, self.dims))
        if int(result["changed"]) and not smooth.flags & _lib.SMOOTH_DRY_RUN:
            self._labels_edited = True
            self._records_for = None
        return scene.relabel_result_dict(result)

    def smooth(self, ctx, names=None, radius=1, iterations=1, box=None, window=(0, 255), uncut=False):
        """Smooth the segmentation: a majority filter over the neighbourhood of `radius` texels (an int, or (rx, ry, rz): (1, 1, 0)
        smooths inside slices).  names None: joint, every label gives and takes; a list (names, ids or label values): those
        segments and label 0 give and take -- a median filter of one segment against the background.  `iterations` passes, EACH AN
        UNDO STEP of its own; they stop early once a pass changes nothing.  Returns the list of the results' dicts."""
        self._ready_to_edit(ctx)
        table = None if names is None else scene.smooth_table(self._label_values(names) + [0])
        flags = _lib.SMOOTH_UNCUT if uncut else 0
        out = []
        for _ in range(int(iterations)):
            out.append(self._smooth(ctx, scene.Smooth(radius, box, flags, window, table, table, dims=self.dims)))
            if not out[-1]["changed"]:
                break
        return out

    def smooth_at(self, ctx, x, y, radius=1, iterations=1, alpha_min=0.5):
        """Click to smooth: pick pixel (x, y) and smooth the segment it shows against label 0.  Returns the pick with a "smooth"
        entry (the list smooth returns; None when the pixel shows no sample or no label)."""
        self._ready_to_edit(ctx)
        p = self.pick(ctx, x, y, alpha_min)
        p["smooth"] = None
        if p["status"] == "hit" and p["label"] is not None:
            p["smooth"] = self.smooth(ctx, [int(p["label"])], radius, iterations)
        return p

    def save_labels(self, ctx, path):
        """Write the labels as they stand on the device to `path`: raw bytes in the orientation prepare_volume read, so that the
        file loads again as labels_raw.  Returns the number of bytes."""
        if not self._labels_on_device:
            raw = self._labels_raw
        else:
            raw = self._labels_raw = self._labels_from_device(ctx)
            self._labels_edited = False
        with open(path, "wb") as f:
            f.write(raw.tobytes())
        return int(raw.size)
