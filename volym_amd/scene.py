"""Host scene model: thin Python faces over the C++ shim in libvolym_hip.so
(volym_amd/csrc/scene.cpp, include/volym_host.h).  Names follow the reference
(src/camera.rs, src/state.rs, src/transfer_function.rs); no math is done in Python.
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import CameraUniforms, ParameterUniforms  # noqa: F401  (re-export)


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class Camera:
    """src/camera.rs:5-73"""

    def __init__(self, c=None):
        self.c = c if c is not None else _lib.CCamera()

    @staticmethod
    def default_with_aspect_and_pos(aspect, position):
        cam = Camera()
        pos = (C.c_float * 3)(*position)
        _lib.lib().volym_camera_default_with_aspect_and_pos(C.byref(cam.c), float(aspect), pos)
        return cam

    def orbit(self, horizontal_delta, vertical_delta, zoom_delta):
        _lib.lib().volym_camera_orbit(C.byref(self.c), float(horizontal_delta), float(vertical_delta),
                                      float(zoom_delta))

    def view_matrix(self):
        m = np.zeros((4, 4), np.float32)
        _lib.lib().volym_camera_view_matrix(C.byref(self.c), _f32p(m))
        return m

    def projection_matrix(self):
        m = np.zeros((4, 4), np.float32)
        _lib.lib().volym_camera_projection_matrix(C.byref(self.c), _f32p(m))
        return m

    def uniforms(self):
        """CameraUniforms::try_from(&Camera) (src/gpu_resources/camera.rs:66-85)"""
        u = CameraUniforms()
        rc = _lib.lib().volym_camera_uniforms_from(C.byref(self.c), C.byref(u))
        if rc != _lib.OK:
            raise _lib.VolymError(rc, "inverse_view_proj inversion failed")
        return u

    @property
    def position(self):
        return tuple(self.c.position)


class StateParameters:
    """src/state.rs:28-55; `benchmark()` = src/main.rs:180-190"""

    def __init__(self, c=None):
        if c is None:
            c = _lib.CStateParameters()
            _lib.lib().volym_state_parameters_default(C.byref(c))
        self.c = c

    @staticmethod
    def benchmark():
        c = _lib.CStateParameters()
        _lib.lib().volym_state_parameters_benchmark(C.byref(c))
        return StateParameters(c)

    def replace(self, **kw):
        c = _lib.CStateParameters.from_buffer_copy(bytes(self.c))
        for k, v in kw.items():
            if k == "camera_position":
                c.camera_position = (C.c_float * 3)(*v)
            else:
                if not hasattr(c, k):
                    raise AttributeError(k)
                setattr(c, k, v)
        return StateParameters(c)


class State:
    """src/state.rs:11-76, :153-155 (parameter half; window input is out of scope)"""

    def __init__(self, c):
        self.c = c

    @staticmethod
    def with_parameters(aspect, parameters):
        c = _lib.CState()
        _lib.lib().volym_state_with_parameters(C.byref(c), float(aspect), C.byref(parameters.c))
        return State(c)

    def update(self):
        _lib.lib().volym_state_update(C.byref(self.c))

    def process_mouse(self, dx, dy):
        _lib.lib().volym_camera_controller_process_mouse(C.byref(self.c.camera_controller), float(dx), float(dy))

    def process_scroll(self, line_delta):
        _lib.lib().volym_camera_controller_process_scroll(C.byref(self.c.camera_controller), float(line_delta))

    @property
    def camera(self):
        return Camera(self.c.camera)

    def camera_uniforms(self):
        return self.camera.uniforms()

    def parameter_uniforms(self):
        """ParameterUniforms::try_from(&State) (src/gpu_resources/parameters.rs:68-83)"""
        u = ParameterUniforms()
        _lib.check(_lib.lib().volym_parameter_uniforms_from(C.byref(self.c), C.byref(u)))
        return u


class TransferFunction:
    """src/transfer_function.rs; baked as GPUTransferFunction::new_texture_1d_rgbt does."""

    def __init__(self, rgb_points=None, alpha_points=None):
        self.rgb_points = [] if rgb_points is None else list(rgb_points)      # (iso, r, g, b)
        self.alpha_points = [] if alpha_points is None else list(alpha_points)  # (iso, a)

    @staticmethod
    def default():
        """impl Default for TransferFunction (src/transfer_function.rs:19-56)"""
        return TransferFunction(
            [(0.0, 0, 1, 0), (0.2, 0, 1, 1), (0.4, 1, 1, 0), (0.6, 1, 0, 1), (1.0, 1, 0, 0)],
            [(0.0, 0.0), (1.0, 1.0)])

    def add_rgb_control_point(self, iso, r, g, b):
        self.rgb_points.append((iso, r, g, b))

    def add_alpha_control_point(self, iso, a):
        self.alpha_points.append((iso, a))

    def bake_rgba8(self):
        rgb = np.ascontiguousarray(self.rgb_points, np.float32).reshape(-1, 4)
        al = np.ascontiguousarray(self.alpha_points, np.float32).reshape(-1, 2)
        out = np.zeros(1024, np.uint8)
        _lib.check(_lib.lib().volym_transfer_function_bake(_f32p(rgb), rgb.shape[0], _f32p(al), al.shape[0],
                                                           _u8p(out)))
        return out


def default_lut():
    out = np.zeros(1024, np.uint8)
    _lib.lib().volym_transfer_function_default_lut(_u8p(out))
    return out


def prepare_volume(raw, dims, flip_y=True):
    """GpuVolume::init's byte path (src/gpu_resources/volume.rs:38-61): pad/truncate, FlipMode::Y."""
    nx, ny, nz = dims
    raw = np.ascontiguousarray(raw, np.uint8).ravel()
    out = np.empty(nx * ny * nz, np.uint8)
    _lib.check(_lib.lib().volym_prepare_volume(_u8p(raw), raw.size, nx, ny, nz, 1 if flip_y else 0, _u8p(out)))
    return out


def load_segments(path_or_list):
    """Vec<SegmentInfo> (src/demos/simple/importance.rs:13-20) from the JSON the reference ships."""
    if isinstance(path_or_list, (list, tuple)):
        segs = list(path_or_list)
    else:
        with open(path_or_list) as f:
            segs = json.load(f)
    for s in segs:
        for k in ("label_value", "importance"):
            if not (isinstance(s[k], int) and 0 <= s[k] <= 255):
                raise ValueError("segment field %s must be a u8" % k)
    return segs


def segment_table(segments):
    """The 256-byte label -> importance table of map_segments_to_importance (src/demos/simple/importance.rs:148-158): the
    first segment whose label_value matches wins, labels no segment names get 0."""
    table = np.zeros(256, np.uint8)
    for s in reversed(list(segments)):
        table[s["label_value"]] = s["importance"]
    return table


def check_segment_table(table):
    t = np.ascontiguousarray(table, np.uint8).ravel()
    if t.size != 256:
        raise ValueError("a segment table has 256 entries, not %d" % t.size)
    return t


def check_segment_visibility(visible):
    """A visibility mask: 256 flags, one per label value, nonzero = visible.  Returns np.uint8[256] of 0 / 1."""
    if isinstance(visible, (str, bytes, bytearray)) and len(visible) != 256:
        raise ValueError("a visibility mask has 256 entries, not %d" % len(visible))
    try:
        v = np.asarray(visible)
    except Exception:
        raise ValueError("a visibility mask is 256 flags, one per label value")
    if v.dtype == object or v.dtype.kind not in "buif":
        raise ValueError("a visibility mask is 256 flags (bool or numbers), not %s" % v.dtype)
    if v.ndim != 1 or v.size != 256:
        raise ValueError("a visibility mask has 256 entries, not %s" % (v.shape,))
    return (v != 0).astype(np.uint8)


def visibility_mask(hidden_label_values):
    """All visible except the given label values."""
    v = np.ones(256, np.uint8)
    for l in hidden_label_values:
        if not 0 <= int(l) <= 255:
            raise ValueError("a label value is a u8, got %r" % (l,))
        v[int(l)] = 0
    return v


def hide_segments(prepared, labels, visible):
    """The definition of segment visibility: a copy of the prepared bytes (density or importances) with every texel whose
    label is hidden set to 0.  `labels`: the prepared label bytes, as many as `prepared`.  Composes with crop_volume."""
    v = check_segment_visibility(visible)
    src = np.ascontiguousarray(prepared, np.uint8).ravel()
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != src.size:
        raise ValueError("labels have %d bytes, the volume %d" % (lab.size, src.size))
    hidden = np.flatnonzero(v == 0)
    if hidden.size <= 16:
        # a compare per hidden label: a gather through the table would widen every label to an index first
        gone = np.zeros(lab.shape, bool)
        for l in hidden:
            gone |= lab == l
    else:
        gone = (v == 0)[lab]
    out = src.copy()
    out[gone] = 0
    return out


def check_crop_box(lo, hi, dims):
    """A crop box in texels of the prepared volume (lo inclusive, hi exclusive, x first): lo <= hi <= n on every axis."""
    try:
        lo, hi, dims = [int(v) for v in lo], [int(v) for v in hi], [int(v) for v in dims]
    except TypeError:
        raise ValueError("a crop box is two triples of texel indices")
    if len(lo) != 3 or len(hi) != 3 or len(dims) != 3:
        raise ValueError("a crop box is two triples of texel indices, got %d and %d values" % (len(lo), len(hi)))
    for a in range(3):
        if not 0 <= lo[a] <= hi[a] <= dims[a]:
            raise ValueError("crop box axis %d: need 0 <= lo <= hi <= %d, got [%d, %d)" % (a, dims[a], lo[a], hi[a]))
    return tuple(lo), tuple(hi)


def crop_box_texels(lo01, hi01, dims):
    """Unit-cube coordinates in [0, 1] (the space the camera orbits, target (.5, .5, .5)) -> texels of the prepared volume:
    texel = floor(p * n + 0.5), clamped to [0, n].  A face at p cuts between the texels whose centres lie on either side."""
    if len(lo01) != 3 or len(hi01) != 3 or len(dims) != 3:
        raise ValueError("a crop box is two triples of unit-cube coordinates")

    def texel(p, n):
        return int(min(max(np.floor(float(p) * n + 0.5), 0), n))
    lo = [texel(p, n) for p, n in zip(lo01, dims)]
    hi = [texel(p, n) for p, n in zip(hi01, dims)]
    return check_crop_box(lo, hi, dims)


def crop_volume(prepared, dims, lo, hi):
    """The definition of the crop box: a copy of the prepared bytes (density or importances) with every texel outside
    [lo, hi) set to 0."""
    lo, hi = check_crop_box(lo, hi, dims)
    nx, ny, nz = dims
    src = np.ascontiguousarray(prepared, np.uint8).reshape(nz, ny, nx)
    out = np.zeros_like(src)
    out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = src[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    return out.ravel()


CLIP_PLANE_MAX = 4096              # VOLYM_CLIP_PLANE_MAX: largest |coefficient| of a clip plane's normal


def check_clip_plane(n, d):
    """A clip plane in texels of the prepared volume: texel (x, y, z) is kept iff n[0]*x + n[1]*y + n[2]*z <= d.  Integers with
    |n[a]| <= 4096 and d in int32; n == (0, 0, 0) only with d == 0 ("no plane").  Returns ((n0, n1, n2), d)."""
    try:
        given = list(n)
        n, offset = [int(v) for v in given], int(d)
        if len(n) != 3 or any(v != i for v, i in zip(given, n)) or offset != d:
            raise TypeError
        d = offset
    except (TypeError, ValueError):
        raise ValueError("a clip plane is a triple of integer coefficients and an integer offset")
    if any(abs(v) > CLIP_PLANE_MAX for v in n):
        raise ValueError("clip plane: need |n| <= %d on every axis, got %r" % (CLIP_PLANE_MAX, tuple(n)))
    if not -2 ** 31 <= d < 2 ** 31:
        raise ValueError("clip plane: d = %d is not a 32-bit integer" % d)
    if n == [0, 0, 0] and d != 0:
        raise ValueError("clip plane: the zero normal means no plane and goes with d == 0 only (to keep nothing: n = (1, 0, 0), d = -1)")
    return tuple(n), d


def clip_plane_texels(normal, point, dims):
    """A plane of the unit cube (the cube the camera orbits; y as the prepared, flipped volume has it) -> integers for
    check_clip_plane.  The kept side is normal . (centre - point) <= 0 with texel centres at (x + 0.5) / n.  In float64:
    g_i = normal_i / dims_i, k = 4096 / max|g_i|, n_i = floor(g_i * k + 0.5), d = floor(sum n_i * (point_i * dims_i - 0.5)).
    A zero normal raises ValueError."""
    if len(normal) != 3 or len(point) != 3 or len(dims) != 3:
        raise ValueError("a clip plane is a normal and a point of the unit cube, three coordinates each")
    g = np.array([float(v) for v in normal], np.float64) / np.array([float(v) for v in dims], np.float64)
    top = float(np.abs(g).max())
    if not np.isfinite(g).all() or top == 0.0:
        raise ValueError("clip plane: the normal must be finite and not zero")
    a = np.floor(g * (CLIP_PLANE_MAX / top) + 0.5)
    p = np.array([float(v) for v in point], np.float64) * np.array([float(v) for v in dims], np.float64) - 0.5
    return check_clip_plane([int(v) for v in a], int(np.floor(float((a * p).sum()))))


def clip_volume(prepared, dims, n, d):
    """The definition of the clip plane: a copy of the prepared bytes (density or importances) with every texel that is not
    kept (n . (x, y, z) > d) set to 0.  Composes with crop_volume and hide_segments."""
    n, d = check_clip_plane(n, d)
    nx, ny, nz = (int(v) for v in dims)
    out = np.array(prepared, np.uint8).reshape(nz, ny, nx)            # (a copy)
    xy = n[0] * np.arange(nx, dtype=np.int64)[None, :] + n[1] * np.arange(ny, dtype=np.int64)[:, None]
    kept = np.empty((ny, nx), bool)
    for z in range(nz):                                               # a slice at a time: the sums of a whole 1024^3 are 8 GiB
        np.less_equal(xy, d - n[2] * z, out=kept)
        np.multiply(out[z], kept, out=out[z])
    return out.ravel()


def check_selection(selected):
    """An outline selection: 256 flags, one per label value, nonzero = selected.  Returns np.uint8[256] of 0 / 1."""
    return check_segment_visibility(selected)


def selection_mask(label_values):
    """Nothing selected except the given label values."""
    return (1 - visibility_mask(label_values)).astype(np.uint8)


def _rgba(c, what):
    v = [int(x) for x in c]
    if len(v) != 4 or not all(0 <= x <= 255 for x in v):
        raise ValueError("%s is four bytes (r, g, b, a)" % what)
    return np.array(v, np.uint32)


def outline_blend(src, col):
    """The blend of the outline pass on uint8 arrays (..., 4): out[c] = (src[c] * (255 - A) + col[c] * A + 127) // 255 for r, g, b
    and the same with 255 for col in the alpha byte, A = col[3]."""
    col = _rgba(col, "a colour")
    a = col[3]
    v = np.array([col[0], col[1], col[2], 255], np.uint32)
    return ((np.asarray(src, np.uint8).astype(np.uint32) * (255 - a) + v * a + 127) // 255).astype(np.uint8)


def outline_frame(frame, picks, rect, selected, ring_rgba, fill_rgba=(0, 0, 0, 0), radius=2):
    """The definition of the outline pass (include/volym_hip.h volym_outline_pass), integers only: `frame` (H, W, 4) uint8, `picks`
    an (h, w) array of _lib.PICK_DTYPE covering rect = (x0, y0, w, h) of it.  A pixel is selected when it lies inside rect, its
    record has status 2 and selected[label] != 0; it is on the ring when it is not selected and a selected pixel of the frame lies
    within `radius` (1..8) of it in the Chebyshev metric.  Ring pixels are blended with ring_rgba, selected ones with fill_rgba
    (outline_blend), every other pixel is the frame's.  Returns a new (H, W, 4) uint8 image."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 4:
        raise ValueError("the frame is (H, W, 4) uint8")
    H, W = frame.shape[:2]
    r = int(radius)
    if not 1 <= r <= 8:
        raise ValueError("the radius is 1..8, got %r" % (radius,))
    if len(rect) != 4:
        raise ValueError("a rect is (x0, y0, w, h)")
    x0, y0, w, h = (int(v) for v in rect)
    if w <= 0 or h <= 0 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError("the rect must be non-empty and inside the frame")
    picks = np.asarray(picks)
    if picks.dtype != _lib.PICK_DTYPE or picks.shape != (h, w):
        raise ValueError("the records are an (h, w) = (%d, %d) array of PICK_DTYPE" % (h, w))
    sel = check_selection(selected)
    mask = np.zeros((H, W), bool)
    mask[y0:y0 + h, x0:x0 + w] = (picks["status"] == 2) & (sel[picks["label"]] != 0)
    # Chebyshev dilation: along x, then along y, on a plane padded with `r` unselected pixels (pixels beyond the frame do not exist)
    pad = np.zeros((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = mask
    rows = np.zeros((H + 2 * r, W), bool)
    for s in range(2 * r + 1):
        rows |= pad[:, s:s + W]
    near = np.zeros((H, W), bool)
    for s in range(2 * r + 1):
        near |= rows[s:s + H]
    ring = near & ~mask
    out = frame.copy()
    out[ring] = outline_blend(frame[ring], ring_rgba)
    out[mask] = outline_blend(frame[mask], fill_rgba)
    return out


def _replaced(obj, noun, names, kw):
    """A copy of request `obj` (a `noun` whose constructor takes `names`) with the fields of kw changed."""
    fields = {k: getattr(obj, k) for k in names}
    for k in kw:
        if k not in fields:
            raise TypeError("a %s has no field %r" % (noun, k))
    fields.update(kw)
    return type(obj)(**fields)


# The box of a request over the scene's bytes (Measure, Surface, Components, Distance, Relabel, Brush): (lo, hi) in texels.
def _box_or_whole(box, dims, missing):
    """`box` as two tuples of int; None: the whole volume, which needs dims -- ValueError(missing) without them."""
    if box is None:
        if dims is None:
            raise ValueError(missing)
        box = ((0, 0, 0), tuple(int(v) for v in dims))
    lo, hi = box
    return (tuple(int(v) for v in lo), tuple(int(v) for v in hi))


def _box_to_c(box, noun):
    """The six u32 of a request's box; ValueError in the name of `noun` where they are not."""
    v = list(box[0]) + list(box[1])
    if len(v) != 6 or not all(0 <= x < 2 ** 32 for x in v):
        raise ValueError("%s: the box is two triples of u32 texel indices" % noun)
    return (C.c_uint32 * 6)(*v)


def _box_in_dims(box, dims, noun):
    """(lo, hi, dims as a list of int) of a box with 0 <= lo <= hi <= dims on every axis; ValueError in the name of `noun`."""
    dims = [int(v) for v in dims]
    lo, hi = box
    if len(lo) != 3 or len(hi) != 3 or len(dims) != 3:
        raise ValueError("%s: the box is two triples of texel indices" % noun)
    for a in range(3):
        if not 0 <= lo[a] <= hi[a] <= dims[a]:
            raise ValueError("%s box axis %d: need 0 <= lo <= hi <= %d, got [%d, %d)" % (noun, a, dims[a], lo[a], hi[a]))
    return lo, hi, dims


SLICE_MAX = 8192                   # largest width and height of a slice
SLICE_LIMIT = 1 << 30              # every corner position of a slice lies in [-2^30, 2^30), 16.16
_SLICE_AXES = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}


class Slice:
    """volym_slice (include/volym_hip.h): an affine map from output pixels to 16.16 texel coordinates -- pixel (i, j) shows texel
    floor((origin + i * du + j * dv) / 65536) -- with what to show there.  mode: _lib.SLICE_DENSITY / SLICE_TF / SLICE_IMPORTANCE;
    flags: SLICE_UNCUT | SLICE_LABELS | SLICE_MARK_CUT; palette: (256, 4) uint8, colour per label value with alpha = strength."""

    def __init__(self, origin, du, dv, width, height, mode=_lib.SLICE_DENSITY, flags=0, background=(0, 0, 0, 255), cut_rgba=(255, 0, 0, 96),
                 palette=None):
        self.origin, self.du, self.dv = (tuple(int(v) for v in t) for t in (origin, du, dv))
        self.width, self.height, self.mode, self.flags = int(width), int(height), int(mode), int(flags)
        self.background, self.cut_rgba = tuple(int(v) for v in background), tuple(int(v) for v in cut_rgba)
        self.palette = np.zeros((256, 4), np.uint8) if palette is None else np.array(palette, np.uint8).reshape(256, 4)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "slice", ("origin", "du", "dv", "width", "height", "mode", "flags", "background", "cut_rgba", "palette"), kw)

    def to_c(self):
        """The _lib.Slice of this slice.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Slice()
        for name in ("origin", "du", "dv"):
            v = getattr(self, name)
            if len(v) != 3 or not all(-2 ** 31 <= x < 2 ** 31 for x in v):
                raise ValueError("slice: %s is three 32-bit integers (16.16)" % name)
            setattr(c, name, (C.c_int32 * 3)(*v))
        for name in ("width", "height", "mode", "flags"):
            v = getattr(self, name)
            if not 0 <= v < 2 ** 32:
                raise ValueError("slice: %s = %d is not a u32" % (name, v))
            setattr(c, name, v)
        c.background = (C.c_uint8 * 4)(*[int(v) for v in _rgba(self.background, "background")])
        c.cut_rgba = (C.c_uint8 * 4)(*[int(v) for v in _rgba(self.cut_rgba, "cut_rgba")])
        C.memmove(c.palette, _u8p(np.ascontiguousarray(self.palette, np.uint8)), 1024)
        return c

    @classmethod
    def from_c(cls, c):
        return cls(tuple(c.origin), tuple(c.du), tuple(c.dv), c.width, c.height, c.mode, c.flags, tuple(c.background), tuple(c.cut_rgba),
                   np.ctypeslib.as_array(c.palette).copy())


def _slice_pos(s, a, i, j):
    return s.origin[a] + i * s.du[a] + j * s.dv[a]          # Python integers: exact


def check_slice(s):
    """The validity rules of volym_slice_check: a known mode, known flag bits, no IMPORTANCE with UNCUT, width and height in
    1..8192, and the four corner positions in [-2^30, 2^30) on every axis.  Returns the slice; raises ValueError."""
    if s.mode not in (_lib.SLICE_DENSITY, _lib.SLICE_TF, _lib.SLICE_IMPORTANCE):
        raise ValueError("slice: unknown mode %r" % (s.mode,))
    if s.flags & ~(_lib.SLICE_UNCUT | _lib.SLICE_LABELS | _lib.SLICE_MARK_CUT) or s.flags < 0:
        raise ValueError("slice: unknown flag bits in %#x" % s.flags)
    if s.mode == _lib.SLICE_IMPORTANCE and s.flags & _lib.SLICE_UNCUT:
        raise ValueError("slice: IMPORTANCE with UNCUT (the importances' uncut source is not one buffer)")
    if not (1 <= s.width <= SLICE_MAX and 1 <= s.height <= SLICE_MAX):
        raise ValueError("slice: width and height are 1..%d, got %d x %d" % (SLICE_MAX, s.width, s.height))
    for a in range(3):
        for i in (0, s.width - 1):
            for j in (0, s.height - 1):
                if not -SLICE_LIMIT <= _slice_pos(s, a, i, j) < SLICE_LIMIT:
                    raise ValueError("slice: corner (%d, %d) is at %d on axis %d, outside [-2^30, 2^30)" % (i, j, _slice_pos(s, a, i, j), a))
    return s


def slice_axis(axis, index, dims, **kw):
    """The slice normal to `axis` ("x", "y", "z" or 0, 1, 2) through texel `index` (volym_slice_axis): one texel per pixel through
    texel centres.  z: u = +x, v = +y.  y: u = +x, v = +z.  x: u = +y, v = +z.  Keywords go to Slice (mode, flags, colours)."""
    if axis not in _SLICE_AXES:
        raise ValueError("a slice axis is x, y or z (0, 1, 2), got %r" % (axis,))
    a = _SLICE_AXES[axis]
    dims = [int(v) for v in dims]
    if len(dims) != 3 or not 0 <= int(index) < dims[a]:
        raise ValueError("slice index %r is not inside axis %d of %r" % (index, a, dims))
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    origin, du, dv = [0x8000] * 3, [0] * 3, [0] * 3
    origin[a] = (int(index) << 16) + 0x8000
    du[u] = dv[v] = 1 << 16
    return check_slice(Slice(origin, du, dv, dims[u], dims[v], **kw))


def slice_texel(s, i, j):
    """The texel (x, y, z) output pixel (i, j) of the slice shows (volym_slice_texel), inside the volume or not: floor, not
    truncation."""
    if not (0 <= int(i) < s.width and 0 <= int(j) < s.height):
        raise ValueError("pixel (%r, %r) is not inside the %d x %d slice" % (i, j, s.width, s.height))
    return tuple(_slice_pos(s, a, int(i), int(j)) >> 16 for a in range(3))


def slice_through(point_texel, normal, up_hint, size, texels_per_pixel=1.0, **kw):
    """An oblique slice: the plane through `point_texel` (texel coordinates, a texel's centre is at index + 0.5) with the given
    normal (texel space; scene.clip_plane_texels gives a clip plane's n, so the cut surface can be shown).  `point_texel` is the
    centre of the size = (width, height) output, rows run against the part of up_hint that lies in the plane, columns along
    up x normal, and a pixel is texels_per_pixel texels wide.  The steps are rounded to 16.16 (float64, round half up), so the
    plane shown is the one of the rounded steps.  Keywords go to Slice."""
    n = np.array([float(v) for v in normal], np.float64)
    up = np.array([float(v) for v in up_hint], np.float64)
    pt = np.array([float(v) for v in point_texel], np.float64)
    w, h = int(size[0]), int(size[1])
    if n.shape != (3,) or up.shape != (3,) or pt.shape != (3,) or not np.isfinite(np.concatenate([n, up, pt])).all() or not (n != 0).any():
        raise ValueError("an oblique slice is a point, a non-zero normal and an up hint, three finite coordinates each")
    n /= np.sqrt((n * n).sum())
    up = up - (up * n).sum() * n
    if np.sqrt((up * up).sum()) < 1e-9:
        raise ValueError("slice_through: the up hint is parallel to the normal")
    up /= np.sqrt((up * up).sum())
    right = np.cross(up, n)
    k = float(texels_per_pixel) * 65536.0
    if not np.isfinite(k) or k <= 0.0:
        raise ValueError("slice_through: texels_per_pixel must be positive")
    du = [int(v) for v in np.floor(right * k + 0.5)]
    dv = [int(v) for v in np.floor(-up * k + 0.5)]
    # twice the centre offset is an integer: origin = round(point * 65536) - ((w - 1) * du + (h - 1) * dv) / 2, floored
    origin = [int(np.floor(pt[a] * 65536.0 + 0.5)) - (((w - 1) * du[a] + (h - 1) * dv[a]) >> 1) for a in range(3)]
    return check_slice(Slice(origin, du, dv, w, h, **kw))


def cut_volume(prepared, dims, cut, labels=None):
    """Box, plane and mask of a cut state applied to prepared bytes (density or importances): crop_volume, clip_volume and
    hide_segments in one.  `cut`: a dict with any of "box": (lo, hi), "plane": (n, d), "visible": 256 flags; None cuts nothing."""
    out = np.ascontiguousarray(prepared, np.uint8).ravel()
    cut = cut or {}
    if cut.get("box") is not None:
        out = crop_volume(out, dims, *cut["box"])
    if cut.get("plane") is not None:
        out = clip_volume(out, dims, *cut["plane"])
    if cut.get("visible") is not None and labels is not None:
        out = hide_segments(out, labels, cut["visible"])
    return out


def slice_frame(prepared, dims, slice, lut=None, labels=None, importances=None, cut=None, uncut=None):
    """The definition of the slice pass (include/volym_hip.h volym_slice_pass), integers only; equal to the device in every byte.
    `prepared`: the density bytes of the scene as it stands (box, plane and mask applied: cut_volume); `uncut`: the density before
    any cut, shown under SLICE_UNCUT (None: the context never cut, `prepared` is shown); `lut`: the RGBA8 bytes
    set_transfer_function received (SLICE_TF); `labels`: prepared label bytes of the volume's dimensions (SLICE_LABELS, and the
    mask of SLICE_MARK_CUT); `importances`: the importance bytes as the march reads them (SLICE_IMPORTANCE); `cut`: the cut state
    SLICE_MARK_CUT marks, as cut_volume takes it.  Returns (height, width, 4) uint8."""
    s = check_slice(slice)
    nx, ny, nz = (int(v) for v in dims)
    n = (nx, ny, nz)
    i = np.arange(s.width, dtype=np.int64)[None, :]
    j = np.arange(s.height, dtype=np.int64)[:, None]
    t = [(s.origin[a] + i * s.du[a] + j * s.dv[a]) >> 16 for a in range(3)]         # floor: an arithmetic shift
    inside = np.ones((s.height, s.width), bool)
    for a in range(3):
        inside &= (t[a] >= 0) & (t[a] < n[a])
    x, y, z = (v[inside] for v in t)
    at = (z * ny + y) * nx + x

    def fetch(arr, what):
        if arr is None:
            raise ValueError("slice_frame: this slice needs %s" % what)
        arr = np.ascontiguousarray(arr, np.uint8).ravel()
        if arr.size != nx * ny * nz:
            raise ValueError("slice_frame: %s have %d bytes, the volume %d" % (what, arr.size, nx * ny * nz))
        return arr[at]

    if s.mode == _lib.SLICE_IMPORTANCE:
        b = fetch(importances, "importances")
    else:
        b = fetch(uncut if (s.flags & _lib.SLICE_UNCUT and uncut is not None) else prepared, "density bytes")
    base = np.empty((b.size, 4), np.uint8)
    if s.mode == _lib.SLICE_TF:
        if lut is None:
            raise ValueError("slice_frame: SLICE_TF needs the transfer function's RGBA8 bytes")
        table = np.ascontiguousarray(lut, np.uint8).reshape(-1, 4)
        base[:] = table[(b.astype(np.int64) * table.shape[0]) >> 8]
    else:
        base[:, 0] = base[:, 1] = base[:, 2] = b
    base[:, 3] = 255
    need_labels = s.flags & _lib.SLICE_LABELS or (s.flags & _lib.SLICE_MARK_CUT and labels is not None)
    lab = fetch(labels, "labels") if need_labels else None
    if s.flags & _lib.SLICE_LABELS:
        # outline_blend with a colour per pixel
        col = np.ascontiguousarray(s.palette, np.uint8).reshape(256, 4)[lab].astype(np.uint32)
        a8 = col[:, 3:4].copy()
        col[:, 3] = 255
        base = ((base.astype(np.uint32) * (255 - a8) + col * a8 + 127) // 255).astype(np.uint8)
    if s.flags & _lib.SLICE_MARK_CUT and cut:
        removed = np.zeros(b.size, bool)
        if cut.get("box") is not None:
            lo, hi = check_crop_box(cut["box"][0], cut["box"][1], dims)
            for a, v in enumerate((x, y, z)):
                removed |= (v < lo[a]) | (v >= hi[a])
        if cut.get("plane") is not None:
            pn, pd = check_clip_plane(*cut["plane"])
            removed |= pn[0] * x + pn[1] * y + pn[2] * z > pd
        if cut.get("visible") is not None and lab is not None:
            removed |= check_segment_visibility(cut["visible"])[lab] == 0
        base[removed] = outline_blend(base[removed], s.cut_rgba)
    out = np.empty((s.height, s.width, 4), np.uint8)
    out[:] = np.array(_rgba(s.background, "background"), np.uint8)
    out[inside] = base
    return out


class Measure:
    """volym_measure (include/volym_hip.h): what one measure pass counts.  box: (lo, hi) in texels of the prepared volume, lo
    inclusive, hi exclusive (None: the whole volume, which needs `dims`); flags: _lib.MEASURE_UNCUT; group: 256 entries, label value
    -> histogram group 0..7 or _lib.MEASURE_NO_GROUP (None: every label in group 0)."""

    def __init__(self, box=None, flags=0, group=None, dims=None):
        self.box = _box_or_whole(box, dims, "a measure without a box needs the volume's dims")
        self.flags = int(flags)
        self.group = np.zeros(256, np.int64) if group is None else np.array(group, np.int64).ravel()

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "measure", ("box", "flags", "group"), kw)

    def to_c(self):
        """The _lib.Measure of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Measure()
        c.box = _box_to_c(self.box, "measure")
        if not 0 <= self.flags < 2 ** 32:
            raise ValueError("measure: flags = %d is not a u32" % self.flags)
        c.flags = self.flags
        if self.group.size != 256 or not ((self.group >= 0) & (self.group <= 255)).all():
            raise ValueError("measure: the group table is 256 bytes")
        c.group = (C.c_uint8 * 256)(*[int(g) for g in self.group])
        return c


def measure_groups(*label_sets):
    """A group table: the label values of the k-th argument go to histogram group k, every other label to no group."""
    if len(label_sets) > _lib.MEASURE_GROUPS:
        raise ValueError("at most %d histogram groups" % _lib.MEASURE_GROUPS)
    g = np.full(256, _lib.MEASURE_NO_GROUP, np.int64)
    for k, values in enumerate(label_sets):
        for l in values:
            if not 0 <= int(l) <= 255:
                raise ValueError("a label value is a u8, got %r" % (l,))
            g[int(l)] = k
    return g


def check_measure(measure, dims):
    """The validity rules of volym_measure_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits, every
    group entry below 8 or 255.  Returns the measure; raises ValueError."""
    m = measure
    _box_in_dims(m.box, dims, "measure")
    if m.flags & ~_lib.MEASURE_UNCUT or m.flags < 0:
        raise ValueError("measure: unknown flag bits in %#x" % m.flags)
    g = np.asarray(m.group)
    if g.size != 256 or not (((g >= 0) & (g < _lib.MEASURE_GROUPS)) | (g == _lib.MEASURE_NO_GROUP)).all():
        raise ValueError("measure: every group entry is 0..%d or %d" % (_lib.MEASURE_GROUPS - 1, _lib.MEASURE_NO_GROUP))
    return m


def empty_measurement():
    """(records, hist) of a pass that counts nothing: 256 empty records (zeros, min 255, max 0, box INT32_MAX x 3, -1 x 3)."""
    rec = np.zeros(256, _lib.SEGMENT_STATS_DTYPE)
    rec["min"] = 255
    rec["box"][:, :3] = 2 ** 31 - 1
    rec["box"][:, 3:] = -1
    return rec, np.zeros((_lib.MEASURE_GROUPS, 256), np.uint64)


def measure_volume(prepared, dims, measure, labels=None, cut=None, uncut=None):
    """The definition of the measure pass (include/volym_hip.h volym_measure_pass), NumPy integers only; equal to the device in every
    byte.  `prepared`: the density bytes of the scene as it stands (box, plane and mask applied: cut_volume); `uncut`: the density
    before any cut, read under MEASURE_UNCUT (None: the context never cut, `prepared` is read); `labels`: prepared label bytes of the
    volume's dimensions (None: every texel has label 0 and the mask removes nothing); `cut`: the cut state, as cut_volume takes it.
    Returns (records, hist): 256 records of _lib.SEGMENT_STATS_DTYPE and uint64[8, 256]."""
    m = check_measure(measure, dims)
    nx, ny, nz = (int(v) for v in dims)
    n = (nx, ny, nz)
    whole = bool(m.flags & _lib.MEASURE_UNCUT)
    cut = {} if whole else (cut or {})
    lo, hi = list(m.box[0]), list(m.box[1])
    if cut.get("box") is not None:
        blo, bhi = check_crop_box(cut["box"][0], cut["box"][1], dims)
        lo = [max(a, b) for a, b in zip(lo, blo)]
        hi = [min(a, b) for a, b in zip(hi, bhi)]
    rec, hist = empty_measurement()
    if any(a >= b for a, b in zip(lo, hi)):
        return rec, hist
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("measure_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub].astype(np.int64)
    if labels is None:
        l = np.zeros_like(b)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("measure_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub].astype(np.int64)
    z, y, x = np.meshgrid(*[np.arange(lo[a], hi[a], dtype=np.int64) for a in (2, 1, 0)], indexing="ij")
    inside = np.ones(b.shape, bool)
    if cut.get("plane") is not None:
        pn, pd = check_clip_plane(*cut["plane"])
        inside &= pn[0] * x + pn[1] * y + pn[2] * z <= pd
    if cut.get("visible") is not None and labels is not None:
        inside &= check_segment_visibility(cut["visible"])[l] != 0
    b, l, pos = b[inside], l[inside], [v[inside] for v in (x, y, z)]
    if b.size == 0:
        return rec, hist
    # counts per (label, byte) and per (label, coordinate): everything else is an integer sum over those tables
    per_byte = np.bincount(l * 256 + b, minlength=65536).reshape(256, 256).astype(np.int64)
    values = np.arange(256, dtype=np.int64)
    count = per_byte.sum(axis=1)
    rec["count"] = count
    rec["sum"] = per_byte @ values
    rec["sum_sq"] = per_byte @ (values * values)
    present = np.flatnonzero(count)
    for k in present:
        nz_b = np.flatnonzero(per_byte[k])
        rec["min"][k], rec["max"][k] = nz_b[0], nz_b[-1]
    for a, name in enumerate(("sum_x", "sum_y", "sum_z")):
        per_pos = np.bincount(l * n[a] + pos[a], minlength=256 * n[a]).reshape(256, n[a]).astype(np.int64)
        rec[name] = per_pos @ np.arange(n[a], dtype=np.int64)
        for k in present:
            nz_p = np.flatnonzero(per_pos[k])
            rec["box"][k, a], rec["box"][k, 3 + a] = nz_p[0], nz_p[-1]
    group = np.asarray(m.group)
    for g in range(_lib.MEASURE_GROUPS):
        hist[g] = per_byte[group == g].sum(axis=0)
    return rec, hist


def segment_summary(stats, spacing=(1, 1, 1)):
    """What a user reads off one record of a measurement (np.void of _lib.SEGMENT_STATS_DTYPE, or a _lib.SegmentStats): count, mean
    and population standard deviation of the density byte, min, max, centroid (texel indices, x first: the mean coordinate),
    centre (the centroid's position in physical units: (centroid + 0.5) * spacing, a texel's centre being at index + 0.5), box
    ((x0, y0, z0), (x1, y1, z1), hi inclusive) and volume (count * the volume of a texel).  Python ints and floats, derived in
    double from exact integers.  None for an empty record."""
    import math
    get = (lambda k: stats[k]) if isinstance(stats, (np.void, dict)) else (lambda k: getattr(stats, k))
    count = int(get("count"))
    if count == 0:
        return None
    s, sq = int(get("sum")), int(get("sum_sq"))
    sums = [int(get(k)) for k in ("sum_x", "sum_y", "sum_z")]
    box = [int(v) for v in get("box")]
    sp = [float(v) for v in spacing]
    centroid = tuple(v / count for v in sums)
    return {"count": count, "mean": s / count, "std": math.sqrt(count * sq - s * s) / count, "min": int(get("min")), "max": int(get("max")),
            "centroid": centroid, "centre": tuple((c + 0.5) * h for c, h in zip(centroid, sp)),
            "box": (tuple(box[:3]), tuple(box[3:])), "volume": count * sp[0] * sp[1] * sp[2]}


class Surface:
    """volym_surface (include/volym_hip.h): what one surface pass takes the boundary of.  box: (lo, hi) in texels of the prepared
    volume, lo inclusive, hi exclusive (None: the whole volume, which needs `dims`); flags: _lib.SURFACE_UNCUT; min_byte: 1..255, a
    texel is solid only with a density byte of at least this; select: 256 entries, label value -> non-zero when its texels can be
    solid (None: every label)."""

    def __init__(self, box=None, flags=0, min_byte=1, select=None, dims=None):
        self.box = _box_or_whole(box, dims, "a surface without a box needs the volume's dims")
        self.flags = int(flags)
        self.min_byte = int(min_byte)
        self.select = np.ones(256, np.int64) if select is None else np.array(select, np.int64).ravel()

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "surface", ("box", "flags", "min_byte", "select"), kw)

    def to_c(self):
        """The _lib.Surface of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Surface()
        c.box = _box_to_c(self.box, "surface")
        if not 0 <= self.flags < 2 ** 32 or not 0 <= self.min_byte < 2 ** 32:
            raise ValueError("surface: flags = %d and min_byte = %d must be u32" % (self.flags, self.min_byte))
        c.flags, c.min_byte = self.flags, self.min_byte
        if self.select.size != 256 or not ((self.select >= 0) & (self.select <= 255)).all():
            raise ValueError("surface: the select table is 256 bytes")
        c.select = (C.c_uint8 * 256)(*[int(g) for g in self.select])
        return c


def surface_select(label_values):
    """A select table: 1 for the given label values, 0 for every other."""
    s = np.zeros(256, np.int64)
    for l in label_values:
        if not 0 <= int(l) <= 255:
            raise ValueError("a label value is a u8, got %r" % (l,))
        s[int(l)] = 1
    return s


def check_surface(surface, dims):
    """The validity rules of volym_surface_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits, min_byte
    in 1..255.  Returns the surface; raises ValueError."""
    s = surface
    _box_in_dims(s.box, dims, "surface")
    if s.flags & ~_lib.SURFACE_UNCUT or s.flags < 0:
        raise ValueError("surface: unknown flag bits in %#x" % s.flags)
    if not 1 <= s.min_byte <= 255:
        raise ValueError("surface: min_byte is 1..255, got %d" % s.min_byte)
    if np.asarray(s.select).size != 256:
        raise ValueError("surface: the select table has 256 entries")
    return s


def empty_surface():
    """(summary, faces) of a pass that finds nothing: a zero summary (np.void of _lib.SURFACE_SUMMARY_DTYPE) and no face records."""
    return np.zeros(1, _lib.SURFACE_SUMMARY_DTYPE)[0], np.zeros(0, _lib.SURFACE_FACE_DTYPE)


def surface_volume(prepared, dims, surface, labels=None, cut=None, uncut=None):
    """The definition of the surface passes (include/volym_hip.h volym_surface_pass / volym_surface_faces_pass), NumPy integers only;
    equal to the device in every byte.  `prepared`: the density bytes of the scene as it stands (box, plane and mask applied:
    cut_volume); `uncut`: the density before any cut, read under SURFACE_UNCUT (None: the context never cut, `prepared` is read);
    `labels`: prepared label bytes of the volume's dimensions (None: every texel has label 0).  `cut` is what measure_volume takes in
    this place and is not read: a cut texel has byte 0 in `prepared` and min_byte >= 1, so the cuts are in the bytes.
    Returns (summary, faces): an np.void of _lib.SURFACE_SUMMARY_DTYPE and the records (_lib.SURFACE_FACE_DTYPE) in ascending
    (z, y, x, dir)."""
    s = check_surface(surface, dims)
    nx, ny, nz = (int(v) for v in dims)
    n = (nx, ny, nz)
    lo, hi = s.box
    summary, none = empty_surface()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, none
    whole = bool(s.flags & _lib.SURFACE_UNCUT)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("surface_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("surface_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    solid = (b >= s.min_byte) & (np.asarray(s.select)[l] != 0)
    p = np.pad(solid, 1)                                    # a neighbour outside the request's box is not solid
    mask = np.empty(solid.shape + (6,), bool)               # [z, y, x, dir]
    mask[..., 0] = solid & ~p[1:-1, 1:-1, :-2]
    mask[..., 1] = solid & ~p[1:-1, 1:-1, 2:]
    mask[..., 2] = solid & ~p[1:-1, :-2, 1:-1]
    mask[..., 3] = solid & ~p[1:-1, 2:, 1:-1]
    mask[..., 4] = solid & ~p[:-2, 1:-1, 1:-1]
    mask[..., 5] = solid & ~p[2:, 1:-1, 1:-1]
    at = np.argwhere(mask)                                  # rows in ascending (z, y, x, dir): the canonical order
    faces = np.zeros(len(at), _lib.SURFACE_FACE_DTYPE)
    label = l[at[:, 0], at[:, 1], at[:, 2]].astype(np.int64)
    t = [at[:, 2] + lo[0], at[:, 1] + lo[1], at[:, 0] + lo[2]]
    d = at[:, 3]
    faces["x"], faces["y"], faces["z"], faces["dir"], faces["label"] = t[0], t[1], t[2], d, label
    summary["faces"][...] = np.bincount(label * 6 + d, minlength=256 * 6).reshape(256, 6)
    summary["total"] = len(at)
    for a in range(3):
        for name, side, add in (("neg", 2 * a, 0), ("pos", 2 * a + 1, 1)):
            sel = d == side
            per = np.bincount(label[sel] * (n[a] + 1) + t[a][sel] + add, minlength=256 * (n[a] + 1)).reshape(256, n[a] + 1).astype(np.int64)
            summary[name][:, a] = per @ np.arange(n[a] + 1, dtype=np.int64)
    return summary, faces


def surface_summary(summary, label=None, spacing=(1, 1, 1), stats=None):
    """What a user reads off the summary of a surface pass, for one label value or (label None) for all selected labels together:
    faces (per direction, -x +x -y +y -z +z), pairs (faces per axis: normal to x, y, z), area (sum over the axes of pairs[a] * the
    area of a texel's face normal to a), enclosed (the number of solid texels, from the divergence sums pos - neg), volume
    (enclosed * the volume of a texel) and sphericity (pi^(1/3) * (6 * volume)^(2/3) / area: 1 for a sphere, (pi / 6)^(1/3) ~ 0.81
    for a cube, and a sphere made of texels tends to 2 / 3 because its staircase has 1.5 times the area).  The sums of all labels
    together always close; those of one label do when it was selected alone (two solid texels of different labels have no face
    between them), and where the three axes disagree enclosed, volume and sphericity are None.  With `stats`, the record of the
    same label from a measure pass, "measured" is its count and sphericity takes the volume from it.  Python ints and floats.
    None without faces."""
    import math
    pick = (lambda k: summary[k].astype(np.int64).sum(axis=0)) if label is None else (lambda k: summary[k][label])
    faces = [int(v) for v in pick("faces")]
    if not sum(faces):
        return None
    sp = [float(v) for v in spacing]
    texel = sp[0] * sp[1] * sp[2]
    pairs = [faces[2 * a] + faces[2 * a + 1] for a in range(3)]
    enclosed = {int(p) - int(n) for p, n in zip(pick("pos"), pick("neg"))}
    enclosed = enclosed.pop() if len(enclosed) == 1 else None
    area = pairs[0] * sp[1] * sp[2] + pairs[1] * sp[0] * sp[2] + pairs[2] * sp[0] * sp[1]
    out = {"label": None if label is None else int(label), "faces": faces, "pairs": pairs, "area": area, "enclosed": enclosed,
           "volume": None if enclosed is None else enclosed * texel}
    volume = out["volume"]
    if stats is not None:
        get = (lambda k: stats[k]) if isinstance(stats, (np.void, dict)) else (lambda k: getattr(stats, k))
        out["measured"] = int(get("count"))
        volume = out["measured"] * texel
    out["sphericity"] = None if volume is None else math.pi ** (1.0 / 3.0) * (6.0 * volume) ** (2.0 / 3.0) / area
    return out


# corners of the face on side dir of the unit texel, counter-clockwise seen from outside: (v1 - v0) x (v2 - v0) points along dir
SURFACE_FACE_CORNERS = np.array([
    [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],      # -x
    [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)],      # +x
    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],      # -y
    [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],      # +y
    [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],      # -z
    [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)],      # +z
], np.int64)
SURFACE_FACE_NORMALS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.float32)


def surface_mesh(faces, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """The quad mesh of a face list (records of _lib.SURFACE_FACE_DTYPE): (vertices, quads).  A texel covers [t, t + 1) on every
    axis, so its corners are integer points; corners that several faces share become one vertex (sorted by z, y, x), at origin +
    corner * spacing, float64 [n, 3].  quads: int64 [faces, 4], one per record in the records' order, wound counter-clockwise seen
    from outside the solid."""
    f = np.asarray(faces)
    t = np.stack([f["x"], f["y"], f["z"]], axis=1).astype(np.int64)
    corners = (t[:, None, :] + SURFACE_FACE_CORNERS[f["dir"].astype(np.int64)]).reshape(-1, 3)          # coordinates 0..4096
    key = (corners[:, 2] * 4097 + corners[:, 1]) * 4097 + corners[:, 0]
    unique, inverse = np.unique(key, return_inverse=True)
    points = np.stack([unique % 4097, (unique // 4097) % 4097, unique // (4097 * 4097)], axis=1)
    vertices = np.asarray(origin, np.float64) + points * np.asarray(spacing, np.float64)
    return vertices, inverse.reshape(-1, 4).astype(np.int64)


class Components:
    """volym_components (include/volym_hip.h): what one components pass splits into its pieces.  box, flags, min_byte and select as
    Surface takes them (flags: _lib.COMPONENTS_UNCUT | _lib.COMPONENTS_SPLIT_LABELS); max_components: the table records to keep
    (0: _lib.COMPONENTS_DEFAULT_MAX)."""

    def __init__(self, box=None, flags=0, min_byte=1, select=None, max_components=0, dims=None):
        self.box = _box_or_whole(box, dims, "components without a box need the volume's dims")
        self.flags = int(flags)
        self.min_byte = int(min_byte)
        self.select = np.ones(256, np.int64) if select is None else np.array(select, np.int64).ravel()
        self.max_components = int(max_components)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "components", ("box", "flags", "min_byte", "select", "max_components"), kw)

    def to_c(self):
        """The _lib.Components of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Components()
        c.box = _box_to_c(self.box, "components")
        if not 0 <= self.flags < 2 ** 32 or not 0 <= self.min_byte < 2 ** 32 or not 0 <= self.max_components < 2 ** 32:
            raise ValueError("components: flags = %d, min_byte = %d and max_components = %d must be u32" % (self.flags, self.min_byte, self.max_components))
        c.flags, c.min_byte, c.max_components = self.flags, self.min_byte, self.max_components
        if self.select.size != 256 or not ((self.select >= 0) & (self.select <= 255)).all():
            raise ValueError("components: the select table is 256 bytes")
        c.select = (C.c_uint8 * 256)(*[int(g) for g in self.select])
        return c


def check_components(components, dims):
    """The validity rules of volym_components_check: lo <= hi <= dims on every axis (an empty box is valid), at most
    _lib.COMPONENTS_BOX_MAX texels in the box, known flag bits, min_byte in 1..255, max_components at most
    _lib.COMPONENTS_TABLE_MAX.  Returns the request; raises ValueError."""
    c = components
    lo, hi, dims = _box_in_dims(c.box, dims, "components")
    texels = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    if texels > _lib.COMPONENTS_BOX_MAX:
        raise ValueError("components: the box has %d texels, more than 2^31 - 2" % texels)
    if c.flags & ~(_lib.COMPONENTS_UNCUT | _lib.COMPONENTS_SPLIT_LABELS) or c.flags < 0:
        raise ValueError("components: unknown flag bits in %#x" % c.flags)
    if not 1 <= c.min_byte <= 255:
        raise ValueError("components: min_byte is 1..255, got %d" % c.min_byte)
    if not 0 <= c.max_components <= _lib.COMPONENTS_TABLE_MAX:
        raise ValueError("components: max_components is 0..2^24, got %d" % c.max_components)
    if np.asarray(c.select).size != 256:
        raise ValueError("components: the select table has 256 entries")
    return c


def empty_components():
    """(summary, table, ids) of a pass over an empty box: a zero summary (np.void of _lib.COMPONENTS_SUMMARY_DTYPE), no records
    (_lib.COMPONENT_DTYPE) and no ids."""
    return np.zeros(1, _lib.COMPONENTS_SUMMARY_DTYPE)[0], np.zeros(0, _lib.COMPONENT_DTYPE), np.zeros((0, 0, 0), np.uint32)


def components_volume(prepared, dims, c, labels=None, cut=None, uncut=None):
    """The definition of the components pass (include/volym_hip.h volym_components_pass), NumPy and plain Python integers only; equal
    to the device in every byte.  `prepared`, `uncut`, `labels` and `cut` are what surface_volume takes, and solid is its predicate.
    A union-find over the x-runs of solid texels (with SPLIT_LABELS: of solid texels of one label), with one union for every pair of
    runs of adjacent rows that overlap in x; runs are numbered in ascending (z, y, x) of their first texels and the smaller run
    always becomes the parent, so a component's root run is the one that starts at its root texel.
    Returns (summary, table, ids): an np.void of _lib.COMPONENTS_SUMMARY_DTYPE, the records (_lib.COMPONENT_DTYPE) of the
    components numbered below max_components, and the ids as a uint32 array [z, y, x] over the request's box (its bytes are the
    box-linear id volume), _lib.COMPONENT_NONE where the texel is not solid."""
    c = check_components(c, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = c.box
    summary, table, ids = empty_components()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, table, ids
    whole = bool(c.flags & _lib.COMPONENTS_UNCUT)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("components_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("components_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    split = bool(c.flags & _lib.COMPONENTS_SPLIT_LABELS) and labels is not None
    solid = (b >= c.min_byte) & (np.asarray(c.select)[l] != 0)
    d, h, w = solid.shape
    none = np.uint32(_lib.COMPONENT_NONE)
    ids = np.full((d, h, w), none, np.uint32)
    summary["n_solid"] = int(solid.sum())
    if not solid.any():
        return summary, table, ids

    def linked(here, there):
        """texels of `here` linked to their neighbour in `there` (two views of the box, shifted by one texel)"""
        both = solid[here] & solid[there]
        return both & (l[here] == l[there]) if split else both

    # the x-runs: a solid texel not linked to its left neighbour starts one
    start = solid.copy()
    start[:, :, 1:] &= ~linked((slice(None), slice(None), slice(1, None)), (slice(None), slice(None), slice(0, -1)))
    run_of = np.cumsum(start.ravel(), dtype=np.int64).reshape(d, h, w) - 1           # of every solid texel: its run, in ascending (z, y, x)
    first = np.flatnonzero(start.ravel())                                             # of every run: its first texel, box-linear
    n_runs = first.size
    # one union per pair of overlapping runs of adjacent rows
    pairs = []
    for here, there in (((slice(None), slice(1, None)), (slice(None), slice(0, -1))), ((slice(1, None),), (slice(0, -1),))):
        at = linked(here, there)
        pairs.append(np.unique(run_of[here][at] * n_runs + run_of[there][at]))
    pairs = np.unique(np.concatenate(pairs))
    parent = list(range(n_runs))
    for a, r in zip((pairs // n_runs).tolist(), (pairs % n_runs).tolist()):
        while parent[a] != a:
            parent[a] = a = parent[parent[a]]
        while parent[r] != r:
            parent[r] = r = parent[parent[r]]
        if a < r:
            parent[r] = a
        elif r < a:
            parent[a] = r
    parent = np.array(parent, np.int64)
    while True:                                                                       # every run to its root
        up = parent[parent]
        if np.array_equal(up, parent):
            break
        parent = up
    roots = np.flatnonzero(parent == np.arange(n_runs))                               # ascending: the canonical order
    number = np.zeros(n_runs, np.int64)
    number[roots] = np.arange(roots.size)
    of_run = number[parent]                                                           # of every run: its component
    ids[solid] = of_run[run_of[solid]].astype(np.uint32)

    # the records, from the runs
    n = roots.size
    length = np.bincount(run_of[solid], minlength=n_runs)
    rx, ry, rz = first % w, (first // w) % h, first // (w * h)                         # box coordinates of every run's first texel
    count = np.zeros(n, np.int64)
    np.add.at(count, of_run, length)
    mins = [np.full(n, 1 << 20, np.int64) for _ in range(3)]
    maxs = [np.full(n, -1, np.int64) for _ in range(3)]
    for a, (t0, t1) in enumerate(((rx, rx + length - 1), (ry, ry), (rz, rz))):
        np.minimum.at(mins[a], of_run, t0)
        np.maximum.at(maxs[a], of_run, t1)
    edge = (rx == 0) | (rx + length == w) | (ry == 0) | (ry == h - 1) | (rz == 0) | (rz == d - 1)
    flags = np.zeros(n, np.int64)
    np.maximum.at(flags, of_run, edge.astype(np.int64))
    root_label = l.ravel()[first[roots]].astype(np.int64)
    full = np.zeros(n, _lib.COMPONENT_DTYPE)
    full["x"], full["y"], full["z"] = rx[roots] + lo[0], ry[roots] + lo[1], rz[roots] + lo[2]
    full["label"], full["flags"], full["count"] = root_label, flags, count
    for a in range(3):
        full["box"][:, a] = mins[a] + lo[a]
        full["box"][:, 3 + a] = maxs[a] + lo[a]
    recorded = min(n, c.max_components or _lib.COMPONENTS_DEFAULT_MAX)
    summary["n_components"], summary["recorded"] = n, recorded
    summary["per_label"][...] = np.bincount(root_label, minlength=256)
    return summary, full[:recorded].copy(), ids


def components_summary(summary, table, spacing=(1, 1, 1), below=8):
    """What a user reads off a components pass, per label value that is the root label of some piece: {label: {"pieces": how many
    pieces have a root of that label (the summary's count, whatever the table kept), "recorded": how many of them the table holds,
    "largest": the largest recorded piece as a dict (number, root, count, volume = count * the volume of a texel, box with hi
    inclusive, open: it touches the request's box), "share": the share of ALL solid texels of the request that the largest piece
    holds (of the segment's own texels when the segment was selected alone), "small": the recorded pieces of fewer than `below`
    texels as {"pieces", "texels", "numbers"}}}.  Python ints and floats; labels in ascending order."""
    t = np.asarray(table)
    n_solid = int(summary["n_solid"])
    out = {}
    for label in np.flatnonzero(np.asarray(summary["per_label"])).tolist():
        mine = np.flatnonzero(t["label"] == label)
        one = {"pieces": int(summary["per_label"][label]), "recorded": int(mine.size), "largest": None, "share": None,
               "small": {"pieces": 0, "texels": 0, "numbers": []}}
        if mine.size:
            k = int(mine[np.argmax(t["count"][mine])])             # (the first of equals: the lowest number)
            r = t[k]
            one["largest"] = component_dict(r, k, spacing)
            one["share"] = int(r["count"]) / n_solid
            small = mine[t["count"][mine] < below]
            one["small"] = {"pieces": int(small.size), "texels": int(t["count"][small].sum()), "numbers": small.tolist()}
        out[label] = one
    return out


def component_dict(record, number, spacing=(1, 1, 1)):
    """One record of a components table as a dict of Python values: number, root (x, y, z), label, count, volume, box ((lo), (hi))
    with hi inclusive, open (the piece touches the request's box and may continue outside)."""
    sp = [float(v) for v in spacing]
    box = [int(v) for v in record["box"]]
    return {"number": int(number), "root": (int(record["x"]), int(record["y"]), int(record["z"])), "label": int(record["label"]),
            "count": int(record["count"]), "volume": int(record["count"]) * sp[0] * sp[1] * sp[2],
            "box": (tuple(box[:3]), tuple(box[3:])), "open": bool(int(record["flags"]) & 1)}


class Distance:
    """volym_distance (include/volym_hip.h): what one distance pass maps.  box, flags, min_byte and select as Surface takes them
    (flags: _lib.DISTANCE_UNCUT | _lib.DISTANCE_INSIDE); weight: the three integer weights of the squared distance, 1..64 each."""

    def __init__(self, box=None, flags=0, min_byte=1, select=None, weight=(1, 1, 1), dims=None):
        self.box = _box_or_whole(box, dims, "a distance request without a box needs the volume's dims")
        self.flags = int(flags)
        self.min_byte = int(min_byte)
        self.select = np.ones(256, np.int64) if select is None else np.array(select, np.int64).ravel()
        self.weight = tuple(int(v) for v in weight)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "distance", ("box", "flags", "min_byte", "select", "weight"), kw)

    def to_c(self):
        """The _lib.Distance of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Distance()
        c.box = _box_to_c(self.box, "distance")
        if not 0 <= self.flags < 2 ** 32 or not 0 <= self.min_byte < 2 ** 32:
            raise ValueError("distance: flags = %d and min_byte = %d must be u32" % (self.flags, self.min_byte))
        c.flags, c.min_byte = self.flags, self.min_byte
        if self.select.size != 256 or not ((self.select >= 0) & (self.select <= 255)).all():
            raise ValueError("distance: the select table is 256 bytes")
        c.select = (C.c_uint8 * 256)(*[int(g) for g in self.select])
        if len(self.weight) != 3 or not all(0 <= x < 2 ** 32 for x in self.weight):
            raise ValueError("distance: the weights are three u32")
        c.weight = (C.c_uint32 * 3)(*self.weight)
        return c


def check_distance(distance, dims):
    """The validity rules of volym_distance_check: lo <= hi <= dims on every axis (an empty box is valid), at most
    _lib.DISTANCE_BOX_MAX texels in the box, known flag bits, min_byte in 1..255, every weight in 1.._lib.DISTANCE_WEIGHT_MAX.
    Returns the request; raises ValueError."""
    d = distance
    lo, hi, dims = _box_in_dims(d.box, dims, "distance")
    texels = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    if texels > _lib.DISTANCE_BOX_MAX:
        raise ValueError("distance: the box has %d texels, more than 2^31 - 2" % texels)
    if d.flags & ~(_lib.DISTANCE_UNCUT | _lib.DISTANCE_INSIDE) or d.flags < 0:
        raise ValueError("distance: unknown flag bits in %#x" % d.flags)
    if not 1 <= d.min_byte <= 255:
        raise ValueError("distance: min_byte is 1..255, got %d" % d.min_byte)
    if len(d.weight) != 3 or not all(1 <= v <= _lib.DISTANCE_WEIGHT_MAX for v in d.weight):
        raise ValueError("distance: the weights are three integers in 1..%d, got %r" % (_lib.DISTANCE_WEIGHT_MAX, (d.weight,)))
    if np.asarray(d.select).size != 256:
        raise ValueError("distance: the select table has 256 entries")
    return d


def empty_distance():
    """(summary, map) of a pass over an empty box: no texel is finite (an np.void of _lib.DISTANCE_SUMMARY_DTYPE) and no map."""
    summary = np.zeros(1, _lib.DISTANCE_SUMMARY_DTYPE)[0]
    summary["max_d2"] = _lib.DISTANCE_NONE
    summary["near_d2"][...] = _lib.DISTANCE_NONE
    return summary, np.zeros((0, 0, 0), np.uint32)


def distance_ceil_sqrt(v):
    """The smallest integer c with c * c >= v, elementwise and exact (the float root proposes, integers settle)."""
    v = np.asarray(v, np.int64)
    c = np.sqrt(v.astype(np.float64)).astype(np.int64)
    c += c * c < v
    c -= (c > 0) & ((c - 1) * (c - 1) >= v)
    return c


def distance_volume(prepared, dims, d, labels=None, cut=None, uncut=None):
    """The definition of the distance pass (include/volym_hip.h volym_distance_pass), NumPy integers only; equal to the device in
    every byte.  `prepared`, `uncut`, `labels` and `cut` are what surface_volume takes, and solid is its predicate.  The transform is
    separable: per axis one broadcast minimum, f[i] = min_j g[j] + weight * (i - j)^2, taken one j at a time over the whole box.
    Returns (summary, map): an np.void of _lib.DISTANCE_SUMMARY_DTYPE and D as a uint32 array [z, y, x] over the request's box (its
    bytes are the box-linear map), _lib.DISTANCE_NONE where the box holds no seed."""
    d = check_distance(d, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = d.box
    summary, none = empty_distance()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, none
    whole = bool(d.flags & _lib.DISTANCE_UNCUT)
    inside = bool(d.flags & _lib.DISTANCE_INSIDE)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("distance_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("distance_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    present = b >= d.min_byte
    solid = present & (np.asarray(d.select)[l] != 0)
    seeds = ~solid if inside else solid
    far = np.int64(1) << 40                                         # no seed: above every distance, and three of them do not overflow
    g = np.where(seeds, np.int64(0), far)
    for axis, weight in ((2, d.weight[0]), (1, d.weight[1]), (0, d.weight[2])):
        n = g.shape[axis]
        shape = [1, 1, 1]
        shape[axis] = n
        i = np.arange(n, dtype=np.int64).reshape(shape)
        f = np.full(g.shape, far, np.int64)
        for j in range(n):
            at = [slice(None)] * 3
            at[axis] = slice(j, j + 1)
            np.minimum(f, g[tuple(at)] + weight * (i - j) ** 2, out=f)
        g = np.minimum(f, far)
    if inside:
        # every texel outside the box is a seed, and the nearest of them is the axis-aligned one
        for axis, weight in ((2, d.weight[0]), (1, d.weight[1]), (0, d.weight[2])):
            n = g.shape[axis]
            shape = [1, 1, 1]
            shape[axis] = n
            i = np.arange(n, dtype=np.int64).reshape(shape)
            g = np.minimum(g, weight * np.minimum(i + 1, n - i) ** 2)
    finite = g < far
    out = np.where(finite, g, np.int64(_lib.DISTANCE_NONE)).astype(np.uint32)
    return distance_map_summary(out, b, l, d), out


def distance_map_summary(dmap, density, label, d):
    """The summary of a distance map, from the map (uint32 [z, y, x] over the request's box) and the density and label bytes of the
    same box: what the finish of the pass accumulates, by its definition."""
    summary, _ = empty_distance()
    lo, _hi = d.box
    depth, h, w = dmap.shape
    present = density >= d.min_byte
    solid = present & (np.asarray(d.select)[label] != 0)
    finite = dmap != np.uint32(_lib.DISTANCE_NONE)
    summary["n_solid"], summary["n_present"], summary["n_finite"] = int(solid.sum()), int(present.sum()), int(finite.sum())

    def texel(i):
        return (lo[0] + i % w, lo[1] + (i // w) % h, lo[2] + i // (w * h))

    flat = dmap.ravel().astype(np.int64)
    if finite.any():
        top = int(flat[finite.ravel()].max())
        summary["max_d2"] = top
        summary["max_at"][...] = texel(int(np.flatnonzero(finite.ravel() & (flat == top))[0]))
        bins = np.minimum(distance_ceil_sqrt(flat[finite.ravel()]), 255)
        summary["hist"][...] = np.bincount(bins, minlength=256)
    ok = (present & finite).ravel()
    lab = label.ravel()
    for v in np.unique(lab[ok]).tolist():
        mine = ok & (lab == v)
        best = int(flat[mine].min())
        summary["near_d2"][v] = best
        summary["near_at"][v][...] = texel(int(np.flatnonzero(mine & (flat == best))[0]))
    return summary


def distance_weights(spacing):
    """(weights, unit) for a texel spacing (sx, sy, sz): the squared integer multiples of the smallest spacing, and that smallest
    spacing -- sqrt(D) * unit is a physical distance.  Raises ValueError where a spacing is no integer multiple (1..8) of the
    smallest: the device takes integer weights of at most 64 only."""
    sp = [float(v) for v in spacing]
    if len(sp) != 3 or not all(v > 0.0 and np.isfinite(v) for v in sp):
        raise ValueError("distance_weights: three positive spacings, got %r" % (spacing,))
    unit = min(sp)
    weights = []
    for v in sp:
        m = int(round(v / unit))
        if not 1 <= m <= 8 or abs(v / unit - m) > 1e-6 * m:
            raise ValueError("distance_weights: spacing %g is no integer multiple (1..8) of the smallest, %g" % (v, unit))
        weights.append(m * m)
    return tuple(weights), unit


def distance_summary(summary, unit=1.0):
    """What a user reads off a distance pass, as Python ints and floats: {"n_solid", "n_present", "n_finite", "max_d2", "max_at",
    "max" (sqrt(max_d2) * unit; None without a finite texel), "clearance": {label: {"d2", "distance", "at"}} for every label with a
    present texel at a finite distance, "within": the cumulative histogram -- within[r] texels have a distance of at most r units,
    for r < 255}."""
    none = _lib.DISTANCE_NONE
    top = int(summary["max_d2"])
    out = {"n_solid": int(summary["n_solid"]), "n_present": int(summary["n_present"]), "n_finite": int(summary["n_finite"]),
           "max_d2": None if top == none else top, "max_at": tuple(int(v) for v in summary["max_at"]),
           "max": None if top == none else float(np.sqrt(float(top))) * float(unit), "clearance": {},
           "within": np.cumsum(np.asarray(summary["hist"], np.uint64)[:255]).tolist()}
    for l in np.flatnonzero(np.asarray(summary["near_d2"]) != none).tolist():
        v = int(summary["near_d2"][l])
        out["clearance"][l] = {"d2": v, "distance": float(np.sqrt(float(v))) * float(unit), "at": tuple(int(x) for x in summary["near_at"][l])}
    return out


def relabel_table(mapping=None):
    """The `to` table of a relabel request from {old label: new label}: the identity everywhere else."""
    to = np.arange(256, dtype=np.int64)
    for old, new in (mapping or {}).items():
        if not (0 <= int(old) <= 255 and 0 <= int(new) <= 255):
            raise ValueError("relabel_table: labels are bytes, got %r -> %r" % (old, new))
        to[int(old)] = int(new)
    return to


# What the three edits of the labels share (Relabel, Brush, Lasso; `noun` names the request in every ValueError): the fields box, flags,
# window and to, and the tail of their host twins.
def _edit_fields(r, noun, box, dims, flags, window, to):
    r.box = _box_or_whole(box, dims, "a %s request without a box needs the volume's dims" % noun)
    r.flags = int(flags)
    r.window = tuple(int(v) for v in window)
    r.to = relabel_table() if to is None else (relabel_table(to) if isinstance(to, dict) else np.array(to, np.int64).ravel())


def _edit_fields_to_c(r, c, noun, others_fit, others):
    """box, flags, window and to of request r into its C struct c.  `others_fit`: the request's other u32 fields fit too; `others`:
    how the ValueError names them all."""
    c.box = _box_to_c(r.box, noun)
    if not 0 <= r.flags < 2 ** 32 or len(r.window) != 2 or not all(0 <= x < 2 ** 32 for x in r.window) or not others_fit:
        raise ValueError("%s: %s" % (noun, others))
    c.flags = r.flags
    c.min_byte, c.max_byte = r.window
    if r.to.size != 256 or not ((r.to >= 0) & (r.to <= 255)).all():
        raise ValueError("%s: the table is 256 bytes" % noun)
    c.to = (C.c_uint8 * 256)(*[int(g) for g in r.to])
    return c


def _check_edit_fields(r, dims, noun, known):
    """The rules every edit shares: lo <= hi <= dims on every axis (an empty box is valid), no flag bit outside `known`,
    min_byte <= max_byte <= 255, a table of 256 entries.  Returns dims as a list of int."""
    dims = _box_in_dims(r.box, dims, noun)[2]
    if r.flags & ~known or r.flags < 0:
        raise ValueError("%s: unknown flag bits in %#x" % (noun, r.flags))
    if len(r.window) != 2 or not 0 <= r.window[0] <= r.window[1] <= 255:
        raise ValueError("%s: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (noun, r.window,))
    if np.asarray(r.to).size != 256:
        raise ValueError("%s: the table has 256 entries" % noun)
    return dims


def _edit_volume(noun, prepared, dims, r, labels, uncut, uncut_flag, dry_flag, select):
    """What relabel_volume, brush_volume and lasso_volume share.  `select(lo, hi)`: the request's own condition as a bool array over
    its box [z, y, x], or None for none; it is called only for a box that is not empty.  UNCUT and DRY_RUN are the caller's flag
    values.  Returns (new_labels, result)."""
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = r.box
    result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != nx * ny * nz:
        raise ValueError("%s: labels have %d bytes, the volume %d" % (noun, lab.size, nx * ny * nz))
    new = lab.reshape(nz, ny, nx).copy()
    src = np.ascontiguousarray(uncut if (r.flags & uncut_flag and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != lab.size:
        raise ValueError("%s: the density has %d bytes, the volume %d" % (noun, src.size, lab.size))
    if any(a >= b for a, b in zip(lo, hi)):
        return new, result
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    old = new[sub]
    to = np.asarray(r.to, np.int64).astype(np.uint8)
    d = src.reshape(nz, ny, nx)[sub]
    hit = (to[old] != old) & (d >= r.window[0]) & (d <= r.window[1])
    selected = select(lo, hi)
    if selected is not None:
        hit &= selected
    n = int(hit.sum())
    if n == 0:
        return new, result
    result["changed"] = n
    result["left"][...] = np.bincount(old[hit], minlength=256)
    result["arrived"][...] = np.bincount(to[old[hit]], minlength=256)
    z, y, x = np.nonzero(hit)
    result["box"][...] = (lo[0] + x.min(), lo[1] + y.min(), lo[2] + z.min(), lo[0] + x.max() + 1, lo[1] + y.max() + 1, lo[2] + z.max() + 1)
    if not r.flags & dry_flag:
        new[sub] = np.where(hit, to[old], old)
    return new, result


class Relabel:
    """volym_relabel (include/volym_hip.h): one edit of the labels.  box as Surface takes it; flags: _lib.RELABEL_UNCUT | RELABEL_IDS |
    RELABEL_IDS_EXCEPT | RELABEL_DISTANCE | RELABEL_DRY_RUN; window: (min_byte, max_byte) of the density; to: 256 labels (relabel_table);
    ids: (id_lo, id_hi) in the latest components pass; d2: (d2_lo, d2_hi) in the latest distance map."""

    def __init__(self, box=None, flags=0, window=(0, 255), to=None, ids=(0, 0), d2=(0, 0), dims=None):
        _edit_fields(self, "relabel", box, dims, flags, window, to)
        self.ids = tuple(int(v) for v in ids)
        self.d2 = tuple(int(v) for v in d2)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "relabel", ("box", "flags", "window", "to", "ids", "d2"), kw)

    def to_c(self):
        """The _lib.Relabel of this request.  Fields that do not fit their C types raise ValueError."""
        pairs_fit = all(len(p) == 2 and all(0 <= x < 2 ** 32 for x in p) for p in (self.ids, self.d2))
        c = _edit_fields_to_c(self, _lib.Relabel(), "relabel", pairs_fit, "flags, window, ids and d2 must be u32 (pairs)")
        c.id_lo, c.id_hi = self.ids
        c.d2_lo, c.d2_hi = self.d2
        return c


def check_relabel(relabel, dims):
    """The validity rules of volym_relabel_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits, IDS_EXCEPT
    only with IDS, min_byte <= max_byte <= 255, id_lo <= id_hi with IDS, d2_lo <= d2_hi with DISTANCE.  Returns the request; raises
    ValueError."""
    r = relabel
    _check_edit_fields(r, dims, "relabel", _lib.RELABEL_UNCUT | _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT | _lib.RELABEL_DISTANCE | _lib.RELABEL_DRY_RUN)
    if r.flags & _lib.RELABEL_IDS_EXCEPT and not r.flags & _lib.RELABEL_IDS:
        raise ValueError("relabel: IDS_EXCEPT is valid only together with IDS")
    if r.flags & _lib.RELABEL_IDS and not (len(r.ids) == 2 and 0 <= r.ids[0] <= r.ids[1]):
        raise ValueError("relabel: IDS needs id_lo <= id_hi, got %r" % (r.ids,))
    if r.flags & _lib.RELABEL_DISTANCE and not (len(r.d2) == 2 and 0 <= r.d2[0] <= r.d2[1]):
        raise ValueError("relabel: DISTANCE needs d2_lo <= d2_hi, got %r" % (r.d2,))
    return r


def _snapshot_in_box(name, snap, snap_box, lo, hi):
    """The part of a box-linear snapshot (ids, distance map: uint32 [z, y, x] over snap_box) that covers the request's box."""
    if snap is None or snap_box is None:
        raise ValueError("relabel_volume: %s and its box are needed" % name)
    slo, shi = (tuple(int(v) for v in snap_box[0]), tuple(int(v) for v in snap_box[1]))
    if any(lo[a] < slo[a] or hi[a] > shi[a] for a in range(3)):
        raise ValueError("relabel_volume: the request's box reaches outside the box of %s" % name)
    full = np.asarray(snap, np.uint32).reshape(shi[2] - slo[2], shi[1] - slo[1], shi[0] - slo[0])
    return full[lo[2] - slo[2]:hi[2] - slo[2], lo[1] - slo[1]:hi[1] - slo[1], lo[0] - slo[0]:hi[0] - slo[0]]


def relabel_volume(prepared, dims, r, labels, ids=None, ids_box=None, dmap=None, dmap_box=None, uncut=None):
    """The definition of the label edit (include/volym_hip.h volym_edit_labels), NumPy integers only; equal to the device in every
    byte.  `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None: prepared),
    `labels`: the labels before the edit; ids / dmap: the snapshots of the latest components / distance pass as uint32 [z, y, x] over
    ids_box / dmap_box = ((lo), (hi)).  Returns (new_labels, result): the labels as a uint8 array [z, y, x] of the volume (the input
    untouched; with DRY_RUN a copy of it) and an np.void of _lib.RELABEL_RESULT_DTYPE."""
    r = check_relabel(r, dims)
    lo, hi = r.box
    picked_ids = _snapshot_in_box("the component ids", ids, ids_box, lo, hi) if r.flags & _lib.RELABEL_IDS else None
    picked_map = _snapshot_in_box("the distance map", dmap, dmap_box, lo, hi) if r.flags & _lib.RELABEL_DISTANCE else None

    def select(lo, hi):
        hit = None
        if picked_ids is not None:
            ranged = (picked_ids >= r.ids[0]) & (picked_ids <= r.ids[1])
            hit = (picked_ids != np.uint32(_lib.COMPONENT_NONE)) & (~ranged if r.flags & _lib.RELABEL_IDS_EXCEPT else ranged)
        if picked_map is not None:
            banded = (picked_map != np.uint32(_lib.DISTANCE_NONE)) & (picked_map >= r.d2[0]) & (picked_map <= r.d2[1])
            hit = banded if hit is None else hit & banded
        return hit

    return _edit_volume("relabel_volume", prepared, dims, r, labels, uncut, _lib.RELABEL_UNCUT, _lib.RELABEL_DRY_RUN, select)


class Brush:
    """volym_brush (include/volym_hip.h): one stroke of the brush.  box, window and to as Relabel takes them; flags: _lib.BRUSH_UNCUT |
    BRUSH_DRY_RUN; weight: the distance pass's axis weights (distance_weights); r2: the squared radius in that metric; points: up to
    _lib.BRUSH_MAX_POINTS texels (x, y, z) or (x, y, z, flags), flags = _lib.BRUSH_LIFT: no capsule from the point before."""

    def __init__(self, points, r2, box=None, flags=0, window=(0, 255), to=None, weight=(1, 1, 1), dims=None):
        _edit_fields(self, "brush", box, dims, flags, window, to)
        self.weight = tuple(int(v) for v in weight)
        self.r2 = int(r2)
        self.points = [tuple(int(v) for v in p) + ((0,) if len(p) == 3 else ()) for p in points]

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "brush", ("points", "r2", "box", "flags", "window", "to", "weight"), kw)

    def to_c(self):
        """The _lib.Brush of this request.  Fields that do not fit their C types raise ValueError."""
        c = _edit_fields_to_c(self, _lib.Brush(), "brush", 0 <= self.r2 < 2 ** 32, "flags, r2 and the window's ends must be u32")
        if len(self.weight) != 3 or not all(0 <= x < 2 ** 32 for x in self.weight):
            raise ValueError("brush: three u32 weights")
        c.r2 = self.r2
        c.weight = (C.c_uint32 * 3)(*self.weight)
        if len(self.points) > _lib.BRUSH_MAX_POINTS:
            raise ValueError("brush: at most %d points, got %d" % (_lib.BRUSH_MAX_POINTS, len(self.points)))
        c.n_points = len(self.points)
        for i, p in enumerate(self.points):
            if len(p) != 4 or not all(0 <= x < 2 ** 16 for x in p):
                raise ValueError("brush: a point is (x, y, z[, flags]) of u16, got %r" % (p,))
            c.points[i].x, c.points[i].y, c.points[i].z, c.points[i].flags = p
        return c


def check_brush(brush, dims):
    """The validity rules of volym_brush_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, weights in 1.._lib.DISTANCE_WEIGHT_MAX, 1.._lib.BRUSH_MAX_POINTS points inside the volume, no point
    flag but LIFT; r2 is any u32.  Returns the request; raises ValueError."""
    b = brush
    dims = _check_edit_fields(b, dims, "brush", _lib.BRUSH_UNCUT | _lib.BRUSH_DRY_RUN)
    if len(b.weight) != 3 or not all(1 <= w <= _lib.DISTANCE_WEIGHT_MAX for w in b.weight):
        raise ValueError("brush: three weights in 1..%d, got %r" % (_lib.DISTANCE_WEIGHT_MAX, b.weight))
    if not 0 <= b.r2 < 2 ** 32:
        raise ValueError("brush: r2 is a u32, got %r" % (b.r2,))
    if not 1 <= len(b.points) <= _lib.BRUSH_MAX_POINTS:
        raise ValueError("brush: 1..%d points, got %d" % (_lib.BRUSH_MAX_POINTS, len(b.points)))
    for p in b.points:
        if len(p) != 4 or not all(0 <= p[a] < dims[a] for a in range(3)):
            raise ValueError("brush: point %r lies outside the volume %r" % (p, tuple(dims)))
        if p[3] & ~_lib.BRUSH_LIFT or p[3] < 0:
            raise ValueError("brush: unknown point flag bits in %#x" % p[3])
    return b


def brush_reach(r2, weight):
    """How far a brush of squared radius r2 reaches along an axis of this weight, in texels: the largest m with weight * m * m <= r2."""
    import math
    return math.isqrt(int(r2) // int(weight))


def brush_segments(brush):
    """The segments of the stroke as ((ax, ay, az), (bx, by, bz)): point i gives (p_i, p_i) when i == 0 or it carries LIFT, else
    (p_{i-1}, p_i)."""
    out = []
    for i, p in enumerate(brush.points):
        q = p if i == 0 or p[3] & _lib.BRUSH_LIFT else brush.points[i - 1]
        out.append((tuple(q[:3]), tuple(p[:3])))
    return out


def _brush_span(least, most, brush, dims):
    reach = [brush_reach(brush.r2, w) for w in brush.weight]
    return (tuple(max(least[a] - reach[a], 0) for a in range(3)), tuple(min(most[a] + reach[a] + 1, int(dims[a])) for a in range(3)))


def brush_box(brush, dims):
    """volym_brush_box: the box the brush kernel walks, ((lo), (hi)) -- the request's box cut to the stroke's hull (the points' box
    grown per axis by the brush's reach, clipped to the volume); ((0, 0, 0), (0, 0, 0)) when the two do not meet."""
    b = check_brush(brush, dims)
    pts = np.array([p[:3] for p in b.points], np.int64)
    lo, hi = _brush_span(pts.min(axis=0).tolist(), pts.max(axis=0).tolist(), b, dims)
    lo = tuple(max(lo[a], b.box[0][a]) for a in range(3))
    hi = tuple(min(hi[a], b.box[1][a]) for a in range(3))
    if any(lo[a] >= hi[a] for a in range(3)):
        return ((0, 0, 0), (0, 0, 0))
    return (lo, hi)


def brush_within(t, a, b, weight, r2):
    """Does texel t lie within segment (a, b)?  The integer rule of include/volym_hip.h, on Python integers."""
    dot = lambda u, v: sum(int(weight[k]) * int(u[k]) * int(v[k]) for k in range(3))
    d = [int(b[k]) - int(a[k]) for k in range(3)]
    w = [int(t[k]) - int(a[k]) for k in range(3)]
    dd, wd, ww = dot(d, d), dot(w, d), dot(w, w)
    if dd == 0 or wd <= 0:
        return ww <= r2
    if wd >= dd:
        u = [int(t[k]) - int(b[k]) for k in range(3)]
        return dot(u, u) <= r2
    return ww * dd - wd * wd <= r2 * dd


def brush_mask(brush, dims):
    """The texels within at least one segment of the stroke, as a bool array [z, y, x] of the volume: the rule above in NumPy's 64-bit
    integers (every inner product is below 2^32 and every product below 2^64), segment by segment over the segment's own box."""
    nx, ny, nz = (int(v) for v in dims)
    hit = np.zeros((nz, ny, nx), bool)
    wt = [int(w) for w in brush.weight]
    r2 = int(brush.r2)
    for a, b in brush_segments(brush):
        lo, hi = _brush_span([min(a[k], b[k]) for k in range(3)], [max(a[k], b[k]) for k in range(3)], brush, dims)
        z, y, x = np.meshgrid(*[np.arange(lo[k], hi[k], dtype=np.int64) for k in (2, 1, 0)], indexing="ij")
        t = (x, y, z)
        w = [t[k] - a[k] for k in range(3)]
        d = [b[k] - a[k] for k in range(3)]
        ww = sum(wt[k] * w[k] * w[k] for k in range(3))
        dd = sum(wt[k] * d[k] * d[k] for k in range(3))
        if dd == 0:
            inside = ww <= r2
        else:
            wd = sum(wt[k] * d[k] * w[k] for k in range(3))
            u = [t[k] - b[k] for k in range(3)]
            uu = sum(wt[k] * u[k] * u[k] for k in range(3))
            mid = (wd > 0) & (wd < dd)
            p = np.where(mid, wd, 0).astype(np.uint64)
            perp = ww.astype(np.uint64) * np.uint64(dd) - p * p          # (>= 0 where mid, by Cauchy-Schwarz; unused elsewhere)
            inside = np.where(wd <= 0, ww <= r2, np.where(wd >= dd, uu <= r2, perp <= np.uint64(r2 * dd)))
        hit[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] |= inside
    return hit


def brush_volume(prepared, dims, b, labels, uncut=None):
    """The definition of the brush (include/volym_hip.h volym_brush_labels), integers only; equal to the device in every byte.
    `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None: prepared), `labels`:
    the labels before the stroke.  A texel with label l becomes to[l] iff it lies in the box, to[l] != l, its density byte lies in
    the window and it lies within at least one segment; every texel is decided once, from the bytes before the edit.  Returns
    (new_labels, result) as relabel_volume does."""
    b = check_brush(b, dims)
    select = lambda lo, hi: brush_mask(b, dims)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    return _edit_volume("brush_volume", prepared, dims, b, labels, uncut, _lib.BRUSH_UNCUT, _lib.BRUSH_DRY_RUN, select)


class LassoView:
    """volym_lasso_view (include/volym_hip.h): the integer view texel -> (X, Y, D).  m: three rows of three ints, c: three ints,
    depth: (lo, hi), width x height: the frame, scale_log2: what lasso_view scaled by (lasso_view_depth reads it)."""

    def __init__(self, m, c, depth, width, height, scale_log2=0):
        self.m = tuple(tuple(int(v) for v in row) for row in m)
        self.c = tuple(int(v) for v in c)
        self.depth = tuple(int(v) for v in depth)
        self.width, self.height, self.scale_log2 = int(width), int(height), int(scale_log2)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "lasso view", ("m", "c", "depth", "width", "height", "scale_log2"), kw)

    @classmethod
    def from_c(cls, v):
        return cls([[int(v.m[r][a]) for a in range(3)] for r in range(3)], [int(x) for x in v.c], [int(x) for x in v.depth], v.width, v.height, v.scale_log2)

    def to_c(self):
        """The _lib.LassoView of this view.  Fields that do not fit their C types raise ValueError."""
        v = _lib.LassoView()
        if len(self.m) != 3 or any(len(row) != 3 for row in self.m) or len(self.c) != 3 or len(self.depth) != 2:
            raise ValueError("lasso view: m is 3 x 3, c has three entries, depth two")
        if not all(-2 ** 31 <= x < 2 ** 31 for row in self.m for x in row) or not all(-2 ** 63 <= x < 2 ** 63 for x in self.c + self.depth):
            raise ValueError("lasso view: m is int32, c and depth are int64")
        if not (0 <= self.width < 2 ** 32 and 0 <= self.height < 2 ** 32 and -2 ** 31 <= self.scale_log2 < 2 ** 31):
            raise ValueError("lasso view: width and height are u32, scale_log2 is int32")
        for r in range(3):
            for a in range(3):
                v.m[r][a] = self.m[r][a]
            v.c[r] = self.c[r]
        v.depth[0], v.depth[1] = self.depth
        v.width, v.height, v.scale_log2 = self.width, self.height, self.scale_log2
        return v


class Lasso:
    """volym_lasso (include/volym_hip.h): one cut of the scissors.  points: 3.._lib.LASSO_MAX_POINTS vertices (x, y) in pixels, closed
    implicitly; view: a LassoView; box, window and to as Relabel takes them; flags: _lib.LASSO_UNCUT | LASSO_DRY_RUN | LASSO_OUTSIDE."""

    def __init__(self, points, view, box=None, flags=0, window=(0, 255), to=None, dims=None):
        _edit_fields(self, "lasso", box, dims, flags, window, to)
        self.view = view
        self.points = [tuple(int(v) for v in p) for p in points]

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "lasso", ("points", "view", "box", "flags", "window", "to"), kw)

    def to_c(self):
        """The _lib.Lasso of this request.  Fields that do not fit their C types raise ValueError."""
        c = _edit_fields_to_c(self, _lib.Lasso(), "lasso", True, "flags and the window's ends must be u32")
        c.view = self.view.to_c()
        if len(self.points) > _lib.LASSO_MAX_POINTS:
            raise ValueError("lasso: at most %d vertices, got %d" % (_lib.LASSO_MAX_POINTS, len(self.points)))
        c.n_points = len(self.points)
        for i, p in enumerate(self.points):
            if len(p) != 2 or not all(-2 ** 31 <= x < 2 ** 31 for x in p):
                raise ValueError("lasso: a vertex is (x, y) of int32, got %r" % (p,))
            c.points[i].x, c.points[i].y = p
        return c


def check_lasso(lasso, dims):
    """The validity rules of volym_lasso_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, 3.._lib.LASSO_MAX_POINTS vertices within _lib.LASSO_VERTEX_MAX of the origin, |m| < 2^31, |c| < 2^46,
    1 <= depth[0] <= depth[1], a frame of 1.._lib.LASSO_MAX_FRAME pixels a side.  Returns the request; raises ValueError."""
    l = lasso
    _check_edit_fields(l, dims, "lasso", _lib.LASSO_UNCUT | _lib.LASSO_DRY_RUN | _lib.LASSO_OUTSIDE)
    _check_lasso_polygon(l.points, l.view.width, l.view.height)
    v = l.view
    if len(v.m) != 3 or any(len(row) != 3 for row in v.m) or len(v.c) != 3 or len(v.depth) != 2:
        raise ValueError("lasso view: m is 3 x 3, c has three entries, depth two")
    if not all(abs(x) < 2 ** 31 for row in v.m for x in row):
        raise ValueError("lasso view: |m| < 2^31")
    if not all(abs(x) < 2 ** 46 for x in v.c):
        raise ValueError("lasso view: |c| < 2^46")
    if not 1 <= v.depth[0] <= v.depth[1] < 2 ** 63:
        raise ValueError("lasso view: 1 <= depth[0] <= depth[1], got %r" % (v.depth,))
    return l


def _check_lasso_polygon(points, width, height):
    if not 3 <= len(points) <= _lib.LASSO_MAX_POINTS:
        raise ValueError("lasso: 3..%d vertices, got %d" % (_lib.LASSO_MAX_POINTS, len(points)))
    if not (1 <= width <= _lib.LASSO_MAX_FRAME and 1 <= height <= _lib.LASSO_MAX_FRAME):
        raise ValueError("lasso: a frame of 1..%d pixels a side, got %r x %r" % (_lib.LASSO_MAX_FRAME, width, height))
    for p in points:
        if len(p) != 2 or not all(abs(x) <= _lib.LASSO_VERTEX_MAX for x in p):
            raise ValueError("lasso: vertex %r lies further than 2^20 from the origin" % (p,))


def lasso_view(camera_uniforms, width, height, dims, near=0.0):
    """volym_lasso_view_from_camera: the integer view of a frame -- the ONE quantisation of its camera; the device rule and its twin
    both start from these integers, and nothing restates it here.  camera_uniforms: a CameraUniforms; near: the near distance along
    the view axis (<= 0: none).  Returns a LassoView with depth = (max(1, near), INT64_MAX)."""
    out = _lib.LassoView()
    d = (C.c_uint32 * 3)(*[int(v) for v in dims])
    rc = _lib.lib().volym_lasso_view_from_camera(C.byref(camera_uniforms), int(width), int(height), d, float(near), C.byref(out))
    if rc != _lib.OK:
        raise ValueError("lasso_view: no integer view of this camera, frame and volume (%d)" % rc)
    return LassoView.from_c(out)


def lasso_view_depth(view, front, back=float("inf")):
    """volym_lasso_view_depth: a copy of `view` whose depth range is [front, back], two distances along the view axis in world units."""
    c = view.to_c()
    rc = _lib.lib().volym_lasso_view_depth(C.byref(c), float(front), float(back))
    if rc != _lib.OK:
        raise ValueError("lasso_view_depth: no depth range [%r, %r] (%d)" % (front, back, rc))
    return LassoView.from_c(c)


def lasso_rect(lasso):
    """volym_lasso_rect: the mask's rect (x0, y0, x1, y1), hi exclusive -- the polygon's bounding box cut to the frame; all 0 when the
    two do not meet."""
    _check_lasso_polygon(lasso.points, lasso.view.width, lasso.view.height)
    return _lasso_rect(lasso.points, lasso.view.width, lasso.view.height)


def _lasso_rect(points, width, height):
    xs, ys = [p[0] for p in points], [p[1] for p in points]
    x0, y0, x1, y1 = max(min(xs), 0), max(min(ys), 0), min(max(xs), int(width)), min(max(ys), int(height))
    return (0, 0, 0, 0) if x0 >= x1 or y0 >= y1 else (x0, y0, x1, y1)


def lasso_mask(points, width, height):
    """The polygon's mask over the whole frame, bool [height, width]: pixel (px, py) is in it iff an odd number of edges
    (x0, y0) -> (x1, y1) satisfy (y0 <= py) != (y1 <= py) and (px - x0) (y1 - y0) < (x1 - x0) (py - y0) when y1 > y0, > when y1 < y0
    (include/volym_hip.h), in NumPy's 64-bit integers: every factor is below 2^22."""
    width, height = int(width), int(height)
    _check_lasso_polygon(points, width, height)
    mask = np.zeros((height, width), bool)
    px = np.arange(width, dtype=np.int64)
    n = len(points)
    for i in range(n):
        (x0, y0), (x1, y1) = points[i], points[(i + 1) % n]
        lo, hi = max(min(y0, y1), 0), min(max(y0, y1), height)     # the rows with (y0 <= py) != (y1 <= py): min <= py < max
        if lo >= hi:
            continue
        py = np.arange(lo, hi, dtype=np.int64)
        lhs = (px - x0) * (y1 - y0)
        rhs = (x1 - x0) * (py - y0)
        mask[lo:hi] ^= (lhs[None, :] < rhs[:, None]) if y1 > y0 else (lhs[None, :] > rhs[:, None])
    return mask


def lasso_mask_words(points, width, height):
    """(rect, words): the mask as volym_read_lasso_mask returns it -- the rect of lasso_rect and the bit plane over it, uint32
    [rect_h * ceil(rect_w / 32)]: pixel (px, py) is bit (px - x0) & 31 of word (py - y0) * stride + (px - x0) // 32."""
    rect = _lasso_rect(points, width, height)
    x0, y0, x1, y1 = rect
    if x0 == x1:
        return rect, np.zeros(0, np.uint32)
    sub = lasso_mask(points, width, height)[y0:y1, x0:x1]
    stride = (x1 - x0 + 31) // 32
    bits = np.zeros((y1 - y0, stride * 32), np.uint8)
    bits[:, :x1 - x0] = sub
    return rect, np.packbits(bits, axis=1, bitorder="little").view("<u4").ravel().copy()


def _lasso_below(X, r, D):
    """X < r * D for int64 arrays X, D below 2^62 in size and an int 0 <= r <= 2^14, exact although r * D may not fit 64 bits (the device's
    lasso_below): D = dh * 2^32 + dl, r * D = hi * 2^32 + lo, compared high word first."""
    r = int(r)
    low = r * (D & 0xffffffff)
    hi = r * (D >> 32) + (low >> 32)
    xh = X >> 32
    return (xh < hi) | ((xh == hi) & ((X & 0xffffffff) < (low & 0xffffffff)))


def lasso_texels(view, dims):
    """Which pixel each texel lands on (include/volym_hip.h): (lands, px, py), arrays [z, y, x] of the volume; px and py are 0 where
    the texel does not land.  X, Y and D in NumPy's 64-bit integers, which hold them (below 2^51)."""
    nx, ny, nz = (int(v) for v in dims)
    hx = 2 * np.arange(nx, dtype=np.int64)[None, None, :] + 1
    hy = 2 * np.arange(ny, dtype=np.int64)[None, :, None] + 1
    hz = 2 * np.arange(nz, dtype=np.int64)[:, None, None] + 1
    X, Y, D = (view.m[r][0] * hx + view.m[r][1] * hy + view.m[r][2] * hz + view.c[r] for r in range(3))
    lands = (D >= view.depth[0]) & (D <= view.depth[1]) & (X >= 0) & (Y >= 0) & _lasso_below(X, view.width, D) & _lasso_below(Y, view.height, D)
    safe = np.where(lands, D, 1)
    return lands, np.where(lands, X // safe, 0), np.where(lands, Y // safe, 0)


def lasso_volume(prepared, dims, lasso, labels, uncut=None):
    """The definition of the lasso (include/volym_hip.h volym_lasso_labels), integers only and without any cull; equal to the device
    in every byte.  `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None:
    prepared), `labels`: the labels before the cut.  A texel is inside iff it lands on a pixel of the polygon's mask and selected iff
    inside != OUTSIDE; a selected texel with label l becomes to[l] iff it lies in the box, to[l] != l and its density byte lies in
    the window; every texel is decided once, from the bytes before the edit.  Returns (new_labels, result) as relabel_volume does."""
    l = check_lasso(lasso, dims)

    def select(lo, hi):
        lands, px, py = lasso_texels(l.view, dims)
        inside = lands & lasso_mask(l.points, l.view.width, l.view.height)[py, px]
        return (inside != bool(l.flags & _lib.LASSO_OUTSIDE))[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]

    return _edit_volume("lasso_volume", prepared, dims, l, labels, uncut, _lib.LASSO_UNCUT, _lib.LASSO_DRY_RUN, select)


def smooth_table(labels=None):
    """A give or take table of a smoothing request: 256 bytes, 1 for every label of `labels` (None: for all of them)."""
    if labels is None:
        return np.ones(256, np.uint8)
    t = np.zeros(256, np.uint8)
    for l in labels:
        if not 0 <= int(l) <= 255:
            raise ValueError("smooth_table: labels are bytes, got %r" % (l,))
        t[int(l)] = 1
    return t


class Smooth:
    """volym_smooth (include/volym_hip.h): one pass of the majority filter.  box and window as Relabel takes them; flags:
    _lib.SMOOTH_UNCUT | SMOOTH_DRY_RUN; radius: (rx, ry, rz), each 0.._lib.SMOOTH_MAX_RADIUS and not all 0 (an int: all three);
    give, take: tables of 256 bytes (smooth_table; None: every label) -- the labels whose texels may change and the labels that may
    receive texels."""

    def __init__(self, radius=1, box=None, flags=0, window=(0, 255), give=None, take=None, dims=None):
        self.box = _box_or_whole(box, dims, "a smooth request without a box needs the volume's dims")
        self.flags = int(flags)
        self.window = tuple(int(v) for v in window)
        self.radius = (int(radius),) * 3 if np.isscalar(radius) else tuple(int(v) for v in radius)
        self.give = smooth_table() if give is None else np.array(give, np.int64).ravel()
        self.take = smooth_table() if take is None else np.array(take, np.int64).ravel()

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "smooth", ("radius", "box", "flags", "window", "give", "take"), kw)

    def to_c(self):
        """The _lib.Smooth of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Smooth()
        c.box = _box_to_c(self.box, "smooth")
        if not 0 <= self.flags < 2 ** 32 or len(self.window) != 2 or not all(0 <= x < 2 ** 32 for x in self.window):
            raise ValueError("smooth: flags and the window's ends must be u32")
        if len(self.radius) != 3 or not all(0 <= x < 2 ** 32 for x in self.radius):
            raise ValueError("smooth: three u32 radii")
        c.flags = self.flags
        c.min_byte, c.max_byte = self.window
        c.radius = (C.c_uint32 * 3)(*self.radius)
        for name, t in (("give", self.give), ("take", self.take)):
            if t.size != 256 or not ((t >= 0) & (t <= 255)).all():
                raise ValueError("smooth: %s is a table of 256 bytes" % name)
            setattr(c, name, (C.c_uint8 * 256)(*[int(g) for g in t]))
        return c


def check_smooth(smooth, dims):
    """The validity rules of volym_smooth_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, radii in 0.._lib.SMOOTH_MAX_RADIUS and not all 0, tables of 256 entries.  Returns the request;
    raises ValueError."""
    r = smooth
    _box_in_dims(r.box, dims, "smooth")
    if r.flags & ~(_lib.SMOOTH_UNCUT | _lib.SMOOTH_DRY_RUN) or r.flags < 0:
        raise ValueError("smooth: unknown flag bits in %#x" % r.flags)
    if len(r.window) != 2 or not 0 <= r.window[0] <= r.window[1] <= 255:
        raise ValueError("smooth: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (r.window,))
    if len(r.radius) != 3 or not all(0 <= v <= _lib.SMOOTH_MAX_RADIUS for v in r.radius):
        raise ValueError("smooth: three radii in 0..%d, got %r" % (_lib.SMOOTH_MAX_RADIUS, r.radius))
    if not any(r.radius):
        raise ValueError("smooth: at least one radius above 0")
    if np.asarray(r.give).size != 256 or np.asarray(r.take).size != 256:
        raise ValueError("smooth: give and take have 256 entries")
    return r


def _window_sums(a, r, axis):
    """Sums of int array `a` over [i - r, i + r] along `axis`, cut to the array: differences of one cumulative sum."""
    if r == 0:
        return a
    n = a.shape[axis]
    shape = list(a.shape)
    shape[axis] = 1
    c = np.concatenate([np.zeros(shape, np.int64), np.cumsum(a, axis=axis, dtype=np.int64)], axis=axis)
    i = np.arange(n)
    return np.take(c, np.minimum(i + r, n - 1) + 1, axis=axis) - np.take(c, np.maximum(i - r, 0), axis=axis)


def smooth_volume(prepared, dims, smooth, labels, uncut=None):
    """The definition of the smoothing (include/volym_hip.h volym_smooth_labels), integers only and without any cull; equal to the
    device in every byte.  `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None:
    prepared), `labels`: the labels before the pass.  Per label of the volume, the votes of every texel are box sums of the label's
    indicator over the WHOLE volume (x, then y, then z, from cumulative sums); the winner among the own label and the labels that
    take is the largest count, the own label first and else the smallest label; a texel of the box whose label gives and whose
    density byte lies in the window becomes the winner.  Returns (new_labels, result) as relabel_volume does."""
    r = check_smooth(smooth, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = r.box
    result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != nx * ny * nz:
        raise ValueError("smooth_volume: labels have %d bytes, the volume %d" % (lab.size, nx * ny * nz))
    old = lab.reshape(nz, ny, nx)
    new = old.copy()
    src = np.ascontiguousarray(uncut if (r.flags & _lib.SMOOTH_UNCUT and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != lab.size:
        raise ValueError("smooth_volume: the density has %d bytes, the volume %d" % (src.size, lab.size))
    if any(a >= b for a, b in zip(lo, hi)):
        return new, result
    give, take = np.asarray(r.give) != 0, np.asarray(r.take) != 0
    own = np.zeros(old.shape, np.int64)
    best = np.zeros(old.shape, np.int64)
    best_label = np.zeros(old.shape, np.uint8)
    for m in np.unique(old).tolist():                               # ascending: a later label must beat the count, not equal it
        if not (give[m] or take[m]):
            continue                                                # no candidate of any texel that may change
        is_m = old == m
        votes = _window_sums(_window_sums(_window_sums(is_m.astype(np.int64), r.radius[0], 2), r.radius[1], 1), r.radius[2], 0)
        own[is_m] = votes[is_m]
        if take[m]:
            better = ~is_m & (votes > best)
            best[better] = votes[better]
            best_label[better] = m
    d = src.reshape(nz, ny, nx)
    hit = np.zeros(old.shape, bool)
    hit[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    hit &= give[old] & (best > own) & (d >= r.window[0]) & (d <= r.window[1])
    n = int(hit.sum())
    if n == 0:
        return new, result
    result["changed"] = n
    result["left"][...] = np.bincount(old[hit], minlength=256)
    result["arrived"][...] = np.bincount(best_label[hit], minlength=256)
    z, y, x = np.nonzero(hit)
    result["box"][...] = (x.min(), y.min(), z.min(), x.max() + 1, y.max() + 1, z.max() + 1)
    if not r.flags & _lib.SMOOTH_DRY_RUN:
        new[hit] = best_label[hit]
    return new, result


def check_nearest(distance, dims):
    """The validity rules of volym_nearest_check: those of check_distance, and no INSIDE (the nearest texel that is not solid may lie
    outside the box and has no label).  Returns the request; raises ValueError."""
    d = check_distance(distance, dims)
    if d.flags & _lib.DISTANCE_INSIDE:
        raise ValueError("nearest: INSIDE is not valid for a nearest pass")
    return d


def empty_nearest():
    """(summary, sites, near_labels) of a pass over an empty box: all counters 0 (an np.void of _lib.NEAREST_SUMMARY_DTYPE), no maps."""
    return np.zeros(1, _lib.NEAREST_SUMMARY_DTYPE)[0], np.zeros((0, 0, 0), np.uint32), np.zeros((0, 0, 0), np.uint8)


def nearest_volume(prepared, dims, d, labels=None, cut=None, uncut=None):
    """The definition of the nearest pass (include/volym_hip.h volym_nearest_pass), NumPy integers only; equal to the device in every
    byte.  The arguments are distance_volume's.  Every texel carries the 64-bit key d2 << 31 | site, site being the box-linear index
    of a solid texel (below 2^31, ascending in (z, y, x)); per axis one broadcast minimum of key[j] + (weight * (i - j)^2 << 31), one j
    at a time over the whole box.  Adding to a key is monotone, so the three minima are the minimum over all solid texels of
    (d2, site): the nearest one, the first in (z, y, x) among equals.  Returns (summary, sites, near_labels): an np.void of
    _lib.NEAREST_SUMMARY_DTYPE, the sites as a uint32 array [z, y, x] over the request's box (_lib.NEAREST_NONE: the box holds no solid
    texel) and the label byte of each site as a uint8 array of the same shape."""
    d = check_nearest(d, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = d.box
    summary, no_sites, no_labels = empty_nearest()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, no_sites, no_labels
    whole = bool(d.flags & _lib.DISTANCE_UNCUT)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("nearest_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("nearest_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    present = b >= d.min_byte
    solid = present & (np.asarray(d.select)[l] != 0)
    # d2 < 2^32 and site < 2^31: a key is below 2^63; `far` is above every key, and far + (64 * 4095^2 << 31) is below 2^64
    far = np.uint64(1) << np.uint64(63)
    index = np.arange(b.size, dtype=np.uint64).reshape(b.shape)
    key = np.where(solid, index, far)
    for axis, weight in ((2, d.weight[0]), (1, d.weight[1]), (0, d.weight[2])):
        n = key.shape[axis]
        shape = [1, 1, 1]
        shape[axis] = n
        i = np.arange(n, dtype=np.int64).reshape(shape)
        f = np.full(key.shape, far, np.uint64)
        for j in range(n):
            at = [slice(None)] * 3
            at[axis] = slice(j, j + 1)
            np.minimum(f, key[tuple(at)] + ((weight * (i - j) ** 2).astype(np.uint64) << np.uint64(31)), out=f)
        key = np.minimum(f, far)
    finite = key < far
    sites = np.where(finite, key & np.uint64(0x7FFFFFFF), np.uint64(_lib.NEAREST_NONE)).astype(np.uint32)
    near = np.where(finite, l.ravel()[np.where(finite, sites, 0)], 0).astype(np.uint8)
    summary["n_solid"], summary["n_present"], summary["n_finite"] = int(solid.sum()), int(present.sum()), int(finite.sum())
    summary["cell"][...] = np.bincount(near[finite], minlength=256)
    summary["cell_present"][...] = np.bincount(near[finite & present & ~solid], minlength=256)
    return summary, sites, near


def nearest_d2(sites, box, weight):
    """d2(t, site(t)) of a site map (uint32 [z, y, x] over `box` = ((lo), (hi))) under `weight`, as int64; _lib.NEAREST_NONE where the
    site is."""
    sites = np.asarray(sites, np.uint32)
    depth, h, w = sites.shape
    s = sites.astype(np.int64)
    z, y, x = np.meshgrid(np.arange(depth), np.arange(h), np.arange(w), indexing="ij")
    d2 = weight[0] * (x - s % w) ** 2 + weight[1] * (y - (s // w) % h) ** 2 + weight[2] * (z - s // (w * h)) ** 2
    return np.where(sites == np.uint32(_lib.NEAREST_NONE), np.int64(_lib.NEAREST_NONE), d2)


def nearest_summary(summary, names=None):
    """What a user reads off a nearest pass, as Python ints: {"n_solid", "n_present", "n_finite", "cells": {label or name: {"texels",
    "fill"}}} for every label with a cell -- `texels` of the box are nearest to it, `fill` of them are present and not solid.  names:
    {label: name}."""
    out = {"n_solid": int(summary["n_solid"]), "n_present": int(summary["n_present"]), "n_finite": int(summary["n_finite"]), "cells": {}}
    for l in np.flatnonzero(np.asarray(summary["cell"])).tolist():
        out["cells"][(names or {}).get(l, l)] = {"label": l, "texels": int(summary["cell"][l]), "fill": int(summary["cell_present"][l])}
    return out


class Fill:
    """volym_fill (include/volym_hip.h): one fill by the latest nearest pass.  box and window as Relabel takes them; flags:
    _lib.FILL_UNCUT | FILL_DRY_RUN; give, take: tables of 256 bytes (smooth_table; None: every label) -- the labels whose texels may
    change and the labels that may receive texels; d2: (d2_lo, d2_hi), the band of the squared distance to the site."""

    def __init__(self, box=None, flags=0, window=(0, 255), give=None, take=None, d2=(0, 0xFFFFFFFF), dims=None):
        self.box = _box_or_whole(box, dims, "a fill request without a box needs the volume's dims")
        self.flags = int(flags)
        self.window = tuple(int(v) for v in window)
        self.give = smooth_table() if give is None else np.array(give, np.int64).ravel()
        self.take = smooth_table() if take is None else np.array(take, np.int64).ravel()
        self.d2 = tuple(int(v) for v in d2)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "fill", ("box", "flags", "window", "give", "take", "d2"), kw)

    def to_c(self):
        """The _lib.Fill of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Fill()
        c.box = _box_to_c(self.box, "fill")
        if not 0 <= self.flags < 2 ** 32 or len(self.window) != 2 or not all(0 <= x < 2 ** 32 for x in self.window):
            raise ValueError("fill: flags and the window's ends must be u32")
        if len(self.d2) != 2 or not all(0 <= x < 2 ** 32 for x in self.d2):
            raise ValueError("fill: d2 is a pair of u32")
        c.flags = self.flags
        c.min_byte, c.max_byte = self.window
        c.d2_lo, c.d2_hi = self.d2
        for name, t in (("give", self.give), ("take", self.take)):
            if t.size != 256 or not ((t >= 0) & (t <= 255)).all():
                raise ValueError("fill: %s is a table of 256 bytes" % name)
            setattr(c, name, (C.c_uint8 * 256)(*[int(g) for g in t]))
        return c


def check_fill(fill, dims):
    """The validity rules of volym_fill_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, d2_lo <= d2_hi, tables of 256 entries.  Returns the request; raises ValueError."""
    r = fill
    _box_in_dims(r.box, dims, "fill")
    if r.flags & ~(_lib.FILL_UNCUT | _lib.FILL_DRY_RUN) or r.flags < 0:
        raise ValueError("fill: unknown flag bits in %#x" % r.flags)
    if len(r.window) != 2 or not 0 <= r.window[0] <= r.window[1] <= 255:
        raise ValueError("fill: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (r.window,))
    if len(r.d2) != 2 or not 0 <= r.d2[0] <= r.d2[1]:
        raise ValueError("fill: the band needs d2_lo <= d2_hi, got %r" % (r.d2,))
    if np.asarray(r.give).size != 256 or np.asarray(r.take).size != 256:
        raise ValueError("fill: give and take have 256 entries")
    return r


def fill_volume(prepared, dims, fill, labels, sites, near_labels, pass_box, weight=(1, 1, 1), uncut=None):
    """The definition of the fill (include/volym_hip.h volym_fill_labels), NumPy integers only; equal to the device in every byte.
    `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None: prepared), `labels`: the
    labels before the edit; sites, near_labels: the snapshot of the latest nearest pass (nearest_volume's maps) over pass_box =
    ((lo), (hi)), and `weight` that pass's weights.  A texel of the box whose label gives becomes its near label n iff it has a site,
    n takes, n is not its label, its density byte lies in the window and d2(t, site) lies in the band.  Returns (new_labels, result)
    as relabel_volume does."""
    r = check_fill(fill, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = r.box
    result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != nx * ny * nz:
        raise ValueError("fill_volume: labels have %d bytes, the volume %d" % (lab.size, nx * ny * nz))
    new = lab.reshape(nz, ny, nx).copy()
    src = np.ascontiguousarray(uncut if (r.flags & _lib.FILL_UNCUT and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != lab.size:
        raise ValueError("fill_volume: the density has %d bytes, the volume %d" % (src.size, lab.size))
    slo, shi = (tuple(int(v) for v in pass_box[0]), tuple(int(v) for v in pass_box[1]))
    if any(lo[a] < slo[a] or hi[a] > shi[a] for a in range(3)):
        raise ValueError("fill_volume: the request's box reaches outside the box of the nearest pass")
    if any(a >= b for a, b in zip(lo, hi)):
        return new, result
    shape = (shi[2] - slo[2], shi[1] - slo[1], shi[0] - slo[0])
    inner = (slice(lo[2] - slo[2], hi[2] - slo[2]), slice(lo[1] - slo[1], hi[1] - slo[1]), slice(lo[0] - slo[0], hi[0] - slo[0]))
    site = np.asarray(sites, np.uint32).reshape(shape)
    d2 = nearest_d2(site, (slo, shi), weight)[inner]
    site = site[inner]
    n = np.asarray(near_labels, np.uint8).reshape(shape)[inner]
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    old = new[sub]
    d = src.reshape(nz, ny, nx)[sub]
    give, take = np.asarray(r.give) != 0, np.asarray(r.take) != 0
    hit = give[old] & (site != np.uint32(_lib.NEAREST_NONE)) & take[n] & (n != old) & (d >= r.window[0]) & (d <= r.window[1]) & (d2 >= r.d2[0]) & (d2 <= r.d2[1])
    count = int(hit.sum())
    if count == 0:
        return new, result
    result["changed"] = count
    result["left"][...] = np.bincount(old[hit], minlength=256)
    result["arrived"][...] = np.bincount(n[hit], minlength=256)
    z, y, x = np.nonzero(hit)
    result["box"][...] = (lo[0] + x.min(), lo[1] + y.min(), lo[2] + z.min(), lo[0] + x.max() + 1, lo[1] + y.max() + 1, lo[2] + z.max() + 1)
    if not r.flags & _lib.FILL_DRY_RUN:
        new[sub] = np.where(hit, n, old)
    return new, result


class Geodesic:
    """volym_geodesic (include/volym_hip.h): what one geodesic pass maps.  box as Distance takes it; flags: _lib.GEODESIC_UNCUT;
    window: (min_byte, max_byte) of the medium and of the labelled seeds; seed, through: tables of 256 bytes (smooth_table; None:
    every label but 0 seeds, label 0 the medium); max_steps: 0 for no limit; points: seed texels (x, y, z) in volume coordinates."""

    def __init__(self, box=None, flags=0, window=(1, 255), seed=None, through=None, max_steps=0, points=(), dims=None):
        self.box = _box_or_whole(box, dims, "a geodesic request without a box needs the volume's dims")
        self.flags = int(flags)
        self.window = tuple(int(v) for v in window)
        self.seed = smooth_table(range(1, 256)) if seed is None else np.array(seed, np.int64).ravel()
        self.through = smooth_table([0]) if through is None else np.array(through, np.int64).ravel()
        self.max_steps = int(max_steps)
        self.points = tuple(tuple(int(v) for v in p) for p in points)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "geodesic", ("box", "flags", "window", "seed", "through", "max_steps", "points"), kw)

    def to_c(self):
        """The _lib.Geodesic of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Geodesic()
        c.box = _box_to_c(self.box, "geodesic")
        if not 0 <= self.flags < 2 ** 32 or len(self.window) != 2 or not all(0 <= x < 2 ** 32 for x in self.window) or not 0 <= self.max_steps < 2 ** 32:
            raise ValueError("geodesic: flags, the window's ends and max_steps must be u32")
        c.flags, c.max_steps = self.flags, self.max_steps
        c.min_byte, c.max_byte = self.window
        for name, t in (("seed", self.seed), ("through", self.through)):
            if t.size != 256 or not ((t >= 0) & (t <= 255)).all():
                raise ValueError("geodesic: %s is a table of 256 bytes" % name)
            setattr(c, name, (C.c_uint8 * 256)(*[int(g) for g in t]))
        if not all(len(p) == 3 and all(0 <= x < 2 ** 32 for x in p) for p in self.points):
            raise ValueError("geodesic: a point is three u32")
        c.n_points = len(self.points)                      # (the check refuses more than the struct holds; only those are copied)
        for i, p in enumerate(self.points[:_lib.GEODESIC_POINTS_MAX]):
            c.points[i] = (C.c_uint32 * 3)(*p)
        return c


def check_geodesic(geodesic, dims):
    """The validity rules of volym_geodesic_check: lo <= hi <= dims on every axis (an empty box is valid), at most
    _lib.GEODESIC_BOX_MAX texels, no flag but UNCUT, min_byte <= max_byte <= 255, max_steps <= _lib.GEODESIC_STEPS_MAX, at most
    _lib.GEODESIC_POINTS_MAX points, every point inside the box.  Returns the request; raises ValueError."""
    g = geodesic
    lo, hi, dims = _box_in_dims(g.box, dims, "geodesic")
    texels = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    if texels > _lib.GEODESIC_BOX_MAX:
        raise ValueError("geodesic: the box has %d texels, more than 2^31 - 2" % texels)
    if g.flags & ~_lib.GEODESIC_UNCUT or g.flags < 0:
        raise ValueError("geodesic: unknown flag bits in %#x" % g.flags)
    if len(g.window) != 2 or not 0 <= g.window[0] <= g.window[1] <= 255:
        raise ValueError("geodesic: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (g.window,))
    if not 0 <= g.max_steps <= _lib.GEODESIC_STEPS_MAX:
        raise ValueError("geodesic: max_steps is 0 (no limit) or 1..%d, got %d" % (_lib.GEODESIC_STEPS_MAX, g.max_steps))
    if len(g.points) > _lib.GEODESIC_POINTS_MAX:
        raise ValueError("geodesic: %d points, more than %d" % (len(g.points), _lib.GEODESIC_POINTS_MAX))
    for p in g.points:
        if len(p) != 3 or not all(lo[a] <= p[a] < hi[a] for a in range(3)):
            raise ValueError("geodesic: the point %r lies outside the box" % (p,))
    if np.asarray(g.seed).size != 256 or np.asarray(g.through).size != 256:
        raise ValueError("geodesic: seed and through have 256 entries")
    return g


def empty_geodesic():
    """(summary, keys) of a pass over an empty box: nothing reached (an np.void of _lib.GEODESIC_SUMMARY_DTYPE) and no map."""
    summary = np.zeros(1, _lib.GEODESIC_SUMMARY_DTYPE)[0]
    summary["max_steps"] = _lib.GEODESIC_NONE
    return summary, np.zeros((0, 0, 0), np.uint32)


def geodesic_volume(prepared, dims, g, labels=None, cut=None, uncut=None):
    """The definition of the geodesic pass (include/volym_hip.h volym_geodesic_pass), NumPy integers only; equal to the device in
    every byte.  The arguments are distance_volume's.  Layer by layer: the seeds carry their label as layer 0; layer k is every
    medium texel not reached yet that has a neighbour (one step along one axis, inside the box) in layer k - 1, and it takes the
    smallest label among those neighbours; it ends with an empty layer or at max_steps.  Returns (summary, keys): an np.void of
    _lib.GEODESIC_SUMMARY_DTYPE and the keys steps << 8 | geo_label (_lib.GEODESIC_NONE: not reached) as a uint32 array [z, y, x] over
    the request's box."""
    g = check_geodesic(g, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = g.box
    summary, no_keys = empty_geodesic()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, no_keys
    whole = bool(g.flags & _lib.GEODESIC_UNCUT)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("geodesic_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("geodesic_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    window = (b >= g.window[0]) & (b <= g.window[1])
    seed = window & (np.asarray(g.seed)[l] != 0)
    for p in g.points:
        seed[p[2] - lo[2], p[1] - lo[1], p[0] - lo[0]] = True
    medium = window & (np.asarray(g.through)[l] != 0)
    far = np.int64(1) << np.int64(40)                          # above every key
    key = np.where(seed, l.astype(np.int64), far)
    layer = key.copy()                                         # the keys of the latest layer, `far` elsewhere
    waiting = medium & ~seed
    limit = g.max_steps or _lib.GEODESIC_STEPS_MAX
    for _k in range(1, limit + 1):
        if not waiting.any():
            break
        m = np.full(key.shape, far, np.int64)
        for axis in range(3):
            n = key.shape[axis]
            if n < 2:
                continue
            a, c = [slice(None)] * 3, [slice(None)] * 3
            a[axis], c[axis] = slice(1, n), slice(0, n - 1)
            a, c = tuple(a), tuple(c)
            np.minimum(m[a], layer[c], out=m[a])
            np.minimum(m[c], layer[a], out=m[c])
        new = waiting & (m < far)
        if not new.any():
            break
        key[new] = m[new] + 256
        waiting &= ~new
        layer = np.where(new, key, far)
    reached = key < far
    keys = np.where(reached, key, np.int64(_lib.GEODESIC_NONE)).astype(np.uint32)
    summary["n_seed"], summary["n_medium"], summary["n_reached"] = int(seed.sum()), int((medium & ~seed).sum()), int(reached.sum())
    if reached.any():
        steps = np.where(reached, key >> 8, -1)
        at = int(np.argmax(steps))                              # (the first of the largest, in (z, y, x))
        d, h, w = key.shape
        summary["max_steps"] = int(steps.ravel()[at])
        summary["max_at"][...] = (lo[0] + at % w, lo[1] + (at // w) % h, lo[2] + at // (w * h))
        summary["cell"][...] = np.bincount((key[reached] & 0xFF), minlength=256)
        summary["cell_medium"][...] = np.bincount((key[reached & ~seed] & 0xFF), minlength=256)
        summary["hist"][...] = np.bincount(np.minimum(key[reached] >> 8, 255), minlength=256)
    return summary, keys


def geodesic_summary(summary, names=None):
    """What a user reads off a geodesic pass, as Python ints: {"n_seed", "n_medium", "n_reached", "max_steps" (None: nothing
    reached), "max_at", "cells": {label or name: {"label", "texels", "grown"}}} for every label with a cell -- `texels` of the box
    were reached from it, `grown` of them are no seeds.  names: {label: name}."""
    none = int(summary["n_reached"]) == 0
    out = {"n_seed": int(summary["n_seed"]), "n_medium": int(summary["n_medium"]), "n_reached": int(summary["n_reached"]),
           "max_steps": None if none else int(summary["max_steps"]), "max_at": None if none else tuple(int(v) for v in summary["max_at"]), "cells": {}}
    for l in np.flatnonzero(np.asarray(summary["cell"])).tolist():
        out["cells"][(names or {}).get(l, l)] = {"label": l, "texels": int(summary["cell"][l]), "grown": int(summary["cell_medium"][l])}
    return out


class Flood:
    """volym_flood (include/volym_hip.h): one flood by the latest geodesic pass.  box and window as Relabel takes them; flags:
    _lib.FLOOD_UNCUT | FLOOD_DRY_RUN; give, take: tables of 256 bytes (smooth_table; None: every label) -- the labels whose texels
    may change and the geo labels whose texels may change; to: the label a texel of geo label g becomes (None: g itself; a dict
    {g: label} changes the identity there); steps: (steps_lo, steps_hi), the band of the steps."""

    def __init__(self, box=None, flags=0, window=(0, 255), give=None, take=None, to=None, steps=(0, 0xFFFFFFFF), dims=None):
        self.box = _box_or_whole(box, dims, "a flood request without a box needs the volume's dims")
        self.flags = int(flags)
        self.window = tuple(int(v) for v in window)
        self.give = smooth_table() if give is None else np.array(give, np.int64).ravel()
        self.take = smooth_table() if take is None else np.array(take, np.int64).ravel()
        if to is None or isinstance(to, dict):
            table = np.arange(256, dtype=np.int64)
            for k, v in (to or {}).items():
                table[int(k)] = int(v)
            to = table
        self.to = np.array(to, np.int64).ravel()
        self.steps = tuple(int(v) for v in steps)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "flood", ("box", "flags", "window", "give", "take", "to", "steps"), kw)

    def to_c(self):
        """The _lib.Flood of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Flood()
        c.box = _box_to_c(self.box, "flood")
        if not 0 <= self.flags < 2 ** 32 or len(self.window) != 2 or not all(0 <= x < 2 ** 32 for x in self.window):
            raise ValueError("flood: flags and the window's ends must be u32")
        if len(self.steps) != 2 or not all(0 <= x < 2 ** 32 for x in self.steps):
            raise ValueError("flood: steps is a pair of u32")
        c.flags = self.flags
        c.min_byte, c.max_byte = self.window
        c.steps_lo, c.steps_hi = self.steps
        for name, t in (("give", self.give), ("take", self.take), ("to", self.to)):
            if t.size != 256 or not ((t >= 0) & (t <= 255)).all():
                raise ValueError("flood: %s is a table of 256 bytes" % name)
            setattr(c, name, (C.c_uint8 * 256)(*[int(g) for g in t]))
        return c


def check_flood(flood, dims):
    """The validity rules of volym_flood_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, steps_lo <= steps_hi, tables of 256 entries.  Returns the request; raises ValueError."""
    r = flood
    _box_in_dims(r.box, dims, "flood")
    if r.flags & ~(_lib.FLOOD_UNCUT | _lib.FLOOD_DRY_RUN) or r.flags < 0:
        raise ValueError("flood: unknown flag bits in %#x" % r.flags)
    if len(r.window) != 2 or not 0 <= r.window[0] <= r.window[1] <= 255:
        raise ValueError("flood: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (r.window,))
    if len(r.steps) != 2 or not 0 <= r.steps[0] <= r.steps[1]:
        raise ValueError("flood: the band needs steps_lo <= steps_hi, got %r" % (r.steps,))
    if np.asarray(r.give).size != 256 or np.asarray(r.take).size != 256 or np.asarray(r.to).size != 256:
        raise ValueError("flood: give, take and to have 256 entries")
    return r


def flood_volume(prepared, dims, flood, labels, keys, pass_box, uncut=None):
    """The definition of the flood (include/volym_hip.h volym_flood_labels), NumPy integers only; equal to the device in every byte.
    `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None: prepared), `labels`: the
    labels before the edit; keys: the snapshot of the latest geodesic pass (geodesic_volume's map) over pass_box = ((lo), (hi)).  A
    texel of the box whose label gives becomes to[g], g its geo label, iff its key is not NONE, g takes, to[g] is not its label, its
    density byte lies in the window and its steps lie in the band.  Returns (new_labels, result) as relabel_volume does."""
    r = check_flood(flood, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = r.box
    result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != nx * ny * nz:
        raise ValueError("flood_volume: labels have %d bytes, the volume %d" % (lab.size, nx * ny * nz))
    new = lab.reshape(nz, ny, nx).copy()
    src = np.ascontiguousarray(uncut if (r.flags & _lib.FLOOD_UNCUT and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != lab.size:
        raise ValueError("flood_volume: the density has %d bytes, the volume %d" % (src.size, lab.size))
    slo, shi = (tuple(int(v) for v in pass_box[0]), tuple(int(v) for v in pass_box[1]))
    if any(lo[a] < slo[a] or hi[a] > shi[a] for a in range(3)):
        raise ValueError("flood_volume: the request's box reaches outside the box of the geodesic pass")
    if any(a >= b for a, b in zip(lo, hi)):
        return new, result
    shape = (shi[2] - slo[2], shi[1] - slo[1], shi[0] - slo[0])
    inner = (slice(lo[2] - slo[2], hi[2] - slo[2]), slice(lo[1] - slo[1], hi[1] - slo[1]), slice(lo[0] - slo[0], hi[0] - slo[0]))
    key = np.asarray(keys, np.uint32).reshape(shape)[inner]
    g, steps = (key & np.uint32(0xFF)).astype(np.int64), (key >> np.uint32(8)).astype(np.int64)
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    old = new[sub]
    d = src.reshape(nz, ny, nx)[sub]
    give, take = np.asarray(r.give) != 0, np.asarray(r.take) != 0
    n = np.asarray(r.to).astype(np.uint8)[g]
    hit = give[old] & (key != np.uint32(_lib.GEODESIC_NONE)) & take[g] & (n != old) & (d >= r.window[0]) & (d <= r.window[1]) & (steps >= r.steps[0]) & (steps <= r.steps[1])
    count = int(hit.sum())
    if count == 0:
        return new, result
    result["changed"] = count
    result["left"][...] = np.bincount(old[hit], minlength=256)
    result["arrived"][...] = np.bincount(n[hit], minlength=256)
    z, y, x = np.nonzero(hit)
    result["box"][...] = (lo[0] + x.min(), lo[1] + y.min(), lo[2] + z.min(), lo[0] + x.max() + 1, lo[1] + y.max() + 1, lo[2] + z.max() + 1)
    if not r.flags & _lib.FLOOD_DRY_RUN:
        new[sub] = np.where(hit, n, old)
    return new, result


class Cost:
    """volym_cost (include/volym_hip.h): what one cost pass maps.  box, flags (_lib.COST_UNCUT), window, seed, through and points as
    Geodesic takes them; step: what every step costs, 1..255; contrast: what every unit of density change across a step adds, 0..255;
    max_cost: 0 for no limit; hist_shift: the summary's histogram bins by min(cost >> hist_shift, 255)."""

    def __init__(self, box=None, flags=0, window=(1, 255), seed=None, through=None, step=1, contrast=16, max_cost=0, points=(), hist_shift=0, dims=None):
        self.box = _box_or_whole(box, dims, "a cost request without a box needs the volume's dims")
        self.flags = int(flags)
        self.window = tuple(int(v) for v in window)
        self.seed = smooth_table(range(1, 256)) if seed is None else np.array(seed, np.int64).ravel()
        self.through = smooth_table([0]) if through is None else np.array(through, np.int64).ravel()
        self.step, self.contrast, self.max_cost, self.hist_shift = int(step), int(contrast), int(max_cost), int(hist_shift)
        self.points = tuple(tuple(int(v) for v in p) for p in points)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "cost", ("box", "flags", "window", "seed", "through", "step", "contrast", "max_cost", "points", "hist_shift"), kw)

    def to_c(self):
        """The _lib.Cost of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Cost()
        c.box = _box_to_c(self.box, "cost")
        scalars = (self.flags, self.step, self.contrast, self.max_cost, self.hist_shift)
        if not all(0 <= x < 2 ** 32 for x in scalars) or len(self.window) != 2 or not all(0 <= x < 2 ** 32 for x in self.window):
            raise ValueError("cost: flags, the window's ends, step, contrast, max_cost and hist_shift must be u32")
        c.flags, c.step_cost, c.contrast_cost, c.max_cost, c.hist_shift = scalars
        c.min_byte, c.max_byte = self.window
        for name, t in (("seed", self.seed), ("through", self.through)):
            if t.size != 256 or not ((t >= 0) & (t <= 255)).all():
                raise ValueError("cost: %s is a table of 256 bytes" % name)
            setattr(c, name, (C.c_uint8 * 256)(*[int(g) for g in t]))
        if not all(len(p) == 3 and all(0 <= x < 2 ** 32 for x in p) for p in self.points):
            raise ValueError("cost: a point is three u32")
        c.n_points = len(self.points)                      # (the check refuses more than the struct holds; only those are copied)
        for i, p in enumerate(self.points[:_lib.COST_POINTS_MAX]):
            c.points[i] = (C.c_uint32 * 3)(*p)
        return c


def check_cost(cost, dims):
    """The validity rules of volym_cost_check: lo <= hi <= dims on every axis (an empty box is valid), at most _lib.COST_BOX_MAX
    texels, no flag but UNCUT, min_byte <= max_byte <= 255, step in 1..255, contrast in 0..255, max_cost <= _lib.COST_MAX,
    hist_shift <= 16, at most _lib.COST_POINTS_MAX points, every point inside the box.  Returns the request; raises ValueError."""
    q = cost
    lo, hi, dims = _box_in_dims(q.box, dims, "cost")
    texels = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    if texels > _lib.COST_BOX_MAX:
        raise ValueError("cost: the box has %d texels, more than 2^31 - 2" % texels)
    if q.flags & ~_lib.COST_UNCUT or q.flags < 0:
        raise ValueError("cost: unknown flag bits in %#x" % q.flags)
    if len(q.window) != 2 or not 0 <= q.window[0] <= q.window[1] <= 255:
        raise ValueError("cost: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (q.window,))
    if not 1 <= q.step <= 255:
        raise ValueError("cost: step is 1..255, got %d" % q.step)
    if not 0 <= q.contrast <= 255:
        raise ValueError("cost: contrast is 0..255, got %d" % q.contrast)
    if not 0 <= q.max_cost <= _lib.COST_MAX:
        raise ValueError("cost: max_cost is 0 (no limit) or 1..%d, got %d" % (_lib.COST_MAX, q.max_cost))
    if not 0 <= q.hist_shift <= _lib.COST_HIST_SHIFT_MAX:
        raise ValueError("cost: hist_shift is 0..%d, got %d" % (_lib.COST_HIST_SHIFT_MAX, q.hist_shift))
    if len(q.points) > _lib.COST_POINTS_MAX:
        raise ValueError("cost: %d points, more than %d" % (len(q.points), _lib.COST_POINTS_MAX))
    for p in q.points:
        if len(p) != 3 or not all(lo[a] <= p[a] < hi[a] for a in range(3)):
            raise ValueError("cost: the point %r lies outside the box" % (p,))
    if np.asarray(q.seed).size != 256 or np.asarray(q.through).size != 256:
        raise ValueError("cost: seed and through have 256 entries")
    return q


def empty_cost():
    """(summary, keys) of a pass over an empty box: nothing reached (an np.void of _lib.COST_SUMMARY_DTYPE) and no map."""
    summary = np.zeros(1, _lib.COST_SUMMARY_DTYPE)[0]
    summary["max_cost"] = _lib.COST_NONE
    return summary, np.zeros((0, 0, 0), np.uint32)


def cost_volume(prepared, dims, c, labels=None, cut=None, uncut=None):
    """The definition of the cost pass (include/volym_hip.h volym_cost_pass), NumPy integers only; equal to the device in every byte.
    The arguments are geodesic_volume's.  The seeds carry their label as key; then whole-array sweeps: every medium texel that is no
    seed takes the smallest key(u) + (step(u, t) << 8) over its six neighbours u in the box, where that is below its own and its cost
    within the limit, until a sweep lowers nothing -- the one fixed point, since every step costs at least 1.  Returns
    (summary, keys): an np.void of _lib.COST_SUMMARY_DTYPE and the keys cost << 8 | cost_label (_lib.COST_NONE: not reached) as a
    uint32 array [z, y, x] over the request's box."""
    q = check_cost(c, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = q.box
    summary, no_keys = empty_cost()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, no_keys
    whole = bool(q.flags & _lib.COST_UNCUT)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("cost_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("cost_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    window = (b >= q.window[0]) & (b <= q.window[1])
    seed = window & (np.asarray(q.seed)[l] != 0)
    for p in q.points:
        seed[p[2] - lo[2], p[1] - lo[1], p[0] - lo[0]] = True
    medium = window & (np.asarray(q.through)[l] != 0)
    far = np.int64(1) << np.int64(40)                          # above every key and every key + step
    limit = np.int64(((q.max_cost or _lib.COST_MAX) << 8) | 0xFF)  # the largest key the limit admits
    key = np.where(seed, l.astype(np.int64), far)
    open_ = medium & ~seed
    bi = b.astype(np.int64)
    pairs = []                                                 # per axis with two texels or more: the two slices and step << 8 between them
    for axis in range(3):
        n = key.shape[axis]
        if n < 2:
            continue
        a, d = [slice(None)] * 3, [slice(None)] * 3
        a[axis], d[axis] = slice(1, n), slice(0, n - 1)
        a, d = tuple(a), tuple(d)
        pairs.append((a, d, (q.step + q.contrast * np.abs(bi[a] - bi[d])) << 8))
    while open_.any():
        m = np.full(key.shape, far, np.int64)
        for a, d, step8 in pairs:
            np.minimum(m[a], key[d] + step8, out=m[a])
            np.minimum(m[d], key[a] + step8, out=m[d])
        lower = open_ & (m <= limit) & (m < key)
        if not lower.any():
            break
        key[lower] = m[lower]
    reached = key < far
    keys = np.where(reached, key, np.int64(_lib.COST_NONE)).astype(np.uint32)
    summary["n_seed"], summary["n_medium"], summary["n_reached"] = int(seed.sum()), int(open_.sum()), int(reached.sum())
    if reached.any():
        cost = np.where(reached, key >> 8, -1)
        at = int(np.argmax(cost))                               # (the first of the largest, in (z, y, x))
        d, h, w = key.shape
        summary["max_cost"] = int(cost.ravel()[at])
        summary["max_at"][...] = (lo[0] + at % w, lo[1] + (at // w) % h, lo[2] + at // (w * h))
        summary["cell"][...] = np.bincount((key[reached] & 0xFF), minlength=256)
        summary["cell_medium"][...] = np.bincount((key[reached & ~seed] & 0xFF), minlength=256)
        summary["hist"][...] = np.bincount(np.minimum((key[reached] >> 8) >> q.hist_shift, 255), minlength=256)
    return summary, keys


def cost_summary(summary, names=None):
    """What a user reads off a cost pass, as Python ints: {"n_seed", "n_medium", "n_reached", "max_cost" (None: nothing reached),
    "max_at", "cells": {label or name: {"label", "texels", "grown"}}} for every label with a cell -- `texels` of the box are reached
    most cheaply from it, `grown` of them are no seeds.  names: {label: name}."""
    none = int(summary["n_reached"]) == 0
    out = {"n_seed": int(summary["n_seed"]), "n_medium": int(summary["n_medium"]), "n_reached": int(summary["n_reached"]),
           "max_cost": None if none else int(summary["max_cost"]), "max_at": None if none else tuple(int(v) for v in summary["max_at"]), "cells": {}}
    for l in np.flatnonzero(np.asarray(summary["cell"])).tolist():
        out["cells"][(names or {}).get(l, l)] = {"label": l, "texels": int(summary["cell"][l]), "grown": int(summary["cell_medium"][l])}
    return out


class Spread:
    """volym_spread (include/volym_hip.h): one spread by the latest cost pass.  Everything as Flood takes it -- box, window, flags
    (_lib.SPREAD_UNCUT | SPREAD_DRY_RUN), give, take, to -- with cost: (cost_lo, cost_hi), the band of the cost."""

    def __init__(self, box=None, flags=0, window=(0, 255), give=None, take=None, to=None, cost=(0, 0xFFFFFFFF), dims=None):
        f = Flood(box, flags, window, give, take, to, cost, dims=dims)
        self.box, self.flags, self.window, self.give, self.take, self.to, self.cost = f.box, f.flags, f.window, f.give, f.take, f.to, f.steps

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "spread", ("box", "flags", "window", "give", "take", "to", "cost"), kw)

    def as_flood(self):
        """The Flood with the same fields, its band of steps this band of cost: flood_volume by a cost map is spread_volume."""
        return Flood(self.box, self.flags, self.window, self.give, self.take, self.to, self.cost)

    def to_c(self):
        """The _lib.Spread of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Spread()
        c.box = _box_to_c(self.box, "spread")
        if not 0 <= self.flags < 2 ** 32 or len(self.window) != 2 or not all(0 <= x < 2 ** 32 for x in self.window):
            raise ValueError("spread: flags and the window's ends must be u32")
        if len(self.cost) != 2 or not all(0 <= x < 2 ** 32 for x in self.cost):
            raise ValueError("spread: cost is a pair of u32")
        c.flags = self.flags
        c.min_byte, c.max_byte = self.window
        c.cost_lo, c.cost_hi = self.cost
        for name, t in (("give", self.give), ("take", self.take), ("to", self.to)):
            if t.size != 256 or not ((t >= 0) & (t <= 255)).all():
                raise ValueError("spread: %s is a table of 256 bytes" % name)
            setattr(c, name, (C.c_uint8 * 256)(*[int(g) for g in t]))
        return c


def check_spread(spread, dims):
    """The validity rules of volym_spread_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, cost_lo <= cost_hi, tables of 256 entries.  Returns the request; raises ValueError."""
    r = spread
    _box_in_dims(r.box, dims, "spread")
    if r.flags & ~(_lib.SPREAD_UNCUT | _lib.SPREAD_DRY_RUN) or r.flags < 0:
        raise ValueError("spread: unknown flag bits in %#x" % r.flags)
    if len(r.window) != 2 or not 0 <= r.window[0] <= r.window[1] <= 255:
        raise ValueError("spread: the window is 0 <= min_byte <= max_byte <= 255, got %r" % (r.window,))
    if len(r.cost) != 2 or not 0 <= r.cost[0] <= r.cost[1]:
        raise ValueError("spread: the band needs cost_lo <= cost_hi, got %r" % (r.cost,))
    if np.asarray(r.give).size != 256 or np.asarray(r.take).size != 256 or np.asarray(r.to).size != 256:
        raise ValueError("spread: give, take and to have 256 entries")
    return r


def spread_volume(prepared, dims, spread, labels, keys, pass_box, uncut=None):
    """The definition of the spread (include/volym_hip.h volym_spread_labels), NumPy integers only; equal to the device in every byte.
    The arguments are flood_volume's, keys the snapshot of the latest cost pass (cost_volume's map) over pass_box.  A texel of the
    box whose label gives becomes to[g], g its cost label, iff its key is not NONE, g takes, to[g] is not its label, its density byte
    lies in the window and its cost lies in the band.  Returns (new_labels, result) as relabel_volume does."""
    r = check_spread(spread, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = r.box
    result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != nx * ny * nz:
        raise ValueError("spread_volume: labels have %d bytes, the volume %d" % (lab.size, nx * ny * nz))
    new = lab.reshape(nz, ny, nx).copy()
    src = np.ascontiguousarray(uncut if (r.flags & _lib.SPREAD_UNCUT and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != lab.size:
        raise ValueError("spread_volume: the density has %d bytes, the volume %d" % (src.size, lab.size))
    slo, shi = (tuple(int(v) for v in pass_box[0]), tuple(int(v) for v in pass_box[1]))
    if any(lo[a] < slo[a] or hi[a] > shi[a] for a in range(3)):
        raise ValueError("spread_volume: the request's box reaches outside the box of the cost pass")
    if any(a >= b for a, b in zip(lo, hi)):
        return new, result
    shape = (shi[2] - slo[2], shi[1] - slo[1], shi[0] - slo[0])
    inner = (slice(lo[2] - slo[2], hi[2] - slo[2]), slice(lo[1] - slo[1], hi[1] - slo[1]), slice(lo[0] - slo[0], hi[0] - slo[0]))
    key = np.asarray(keys, np.uint32).reshape(shape)[inner]
    g, cost = (key & np.uint32(0xFF)).astype(np.int64), (key >> np.uint32(8)).astype(np.int64)
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    old = new[sub]
    d = src.reshape(nz, ny, nx)[sub]
    give, take = np.asarray(r.give) != 0, np.asarray(r.take) != 0
    n = np.asarray(r.to).astype(np.uint8)[g]
    hit = give[old] & (key != np.uint32(_lib.COST_NONE)) & take[g] & (n != old) & (d >= r.window[0]) & (d <= r.window[1]) & (cost >= r.cost[0]) & (cost <= r.cost[1])
    count = int(hit.sum())
    if count == 0:
        return new, result
    result["changed"] = count
    result["left"][...] = np.bincount(old[hit], minlength=256)
    result["arrived"][...] = np.bincount(n[hit], minlength=256)
    z, y, x = np.nonzero(hit)
    result["box"][...] = (lo[0] + x.min(), lo[1] + y.min(), lo[2] + z.min(), lo[0] + x.max() + 1, lo[1] + y.max() + 1, lo[2] + z.max() + 1)
    if not r.flags & _lib.SPREAD_DRY_RUN:
        new[sub] = np.where(hit, n, old)
    return new, result


class Interpolate:
    """volym_interpolate (include/volym_hip.h): what one interpolate pass (fill between slices) maps.  box, min_byte, select and weight
    as Distance takes them, but min_byte may be 0 (labels alone decide); flags: _lib.INTERPOLATE_UNCUT | INTERPOLATE_KEYS; axis: 0, 1 or
    2 (or "x", "y", "z"), the slices are the planes perpendicular to it; max_gap: 0 for no limit, else a gap of more slices is not
    filled; keys: the volume coordinates along axis of the key slices, read with KEYS only."""

    def __init__(self, box=None, flags=0, min_byte=1, select=None, weight=(1, 1, 1), axis=2, max_gap=0, keys=(), dims=None):
        self.box = _box_or_whole(box, dims, "an interpolate request without a box needs the volume's dims")
        self.flags = int(flags)
        self.min_byte = int(min_byte)
        self.select = np.ones(256, np.int64) if select is None else np.array(select, np.int64).ravel()
        self.weight = tuple(int(v) for v in weight)
        self.axis = "xyz".index(axis) if isinstance(axis, str) and axis in ("x", "y", "z") else int(axis)
        self.max_gap = int(max_gap)
        self.keys = tuple(sorted(set(int(k) for k in keys)))

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "interpolate", ("box", "flags", "min_byte", "select", "weight", "axis", "max_gap", "keys"), kw)

    def key_words(self):
        """The 128 words of the request's key bits; ValueError for a key outside 0..4095."""
        words = [0] * (_lib.INTERPOLATE_SLICES // 32)
        for k in self.keys:
            if not 0 <= k < _lib.INTERPOLATE_SLICES:
                raise ValueError("interpolate: a key slice is 0..%d, got %d" % (_lib.INTERPOLATE_SLICES - 1, k))
            words[k >> 5] |= 1 << (k & 31)
        return words

    def to_c(self):
        """The _lib.Interpolate of this request.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Interpolate()
        c.box = _box_to_c(self.box, "interpolate")
        if not all(0 <= v < 2 ** 32 for v in (self.flags, self.min_byte, self.axis, self.max_gap)):
            raise ValueError("interpolate: flags, min_byte, axis and max_gap must be u32")
        c.flags, c.min_byte, c.axis, c.max_gap = self.flags, self.min_byte, self.axis, self.max_gap
        if self.select.size != 256 or not ((self.select >= 0) & (self.select <= 255)).all():
            raise ValueError("interpolate: the select table is 256 bytes")
        c.select = (C.c_uint8 * 256)(*[int(g) for g in self.select])
        if len(self.weight) != 3 or not all(0 <= x < 2 ** 32 for x in self.weight):
            raise ValueError("interpolate: the weights are three u32")
        c.weight = (C.c_uint32 * 3)(*self.weight)
        c.keys = (C.c_uint32 * (_lib.INTERPOLATE_SLICES // 32))(*self.key_words())
        return c


def check_interpolate(interpolate, dims):
    """The validity rules of volym_interpolate_check: lo <= hi <= dims on every axis (an empty box is valid), at most
    _lib.DISTANCE_BOX_MAX texels in the box and _lib.INTERPOLATE_SLICES along an axis, known flag bits, min_byte in 0..255, every
    weight in 1.._lib.DISTANCE_WEIGHT_MAX, an axis in 0..2.  Returns the request; raises ValueError."""
    q = interpolate
    lo, hi, dims = _box_in_dims(q.box, dims, "interpolate")
    texels = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    if texels > _lib.DISTANCE_BOX_MAX or any(hi[a] - lo[a] > _lib.INTERPOLATE_SLICES for a in range(3)):
        raise ValueError("interpolate: the box has %d texels, more than 2^31 - 2, or more than %d along an axis" % (texels, _lib.INTERPOLATE_SLICES))
    if q.flags & ~(_lib.INTERPOLATE_UNCUT | _lib.INTERPOLATE_KEYS) or q.flags < 0:
        raise ValueError("interpolate: unknown flag bits in %#x" % q.flags)
    if not 0 <= q.min_byte <= 255:
        raise ValueError("interpolate: min_byte is 0..255, got %d" % q.min_byte)
    if len(q.weight) != 3 or not all(1 <= v <= _lib.DISTANCE_WEIGHT_MAX for v in q.weight):
        raise ValueError("interpolate: the weights are three integers in 1..%d, got %r" % (_lib.DISTANCE_WEIGHT_MAX, (q.weight,)))
    if q.axis not in (0, 1, 2):
        raise ValueError("interpolate: the axis is 0, 1 or 2, got %r" % (q.axis,))
    if q.max_gap < 0:
        raise ValueError("interpolate: max_gap is 0 (no limit) or a number of slices, got %d" % q.max_gap)
    if np.asarray(q.select).size != 256:
        raise ValueError("interpolate: the select table has 256 entries")
    q.key_words()
    return q


def empty_interpolate():
    """(summary, map, state) of a pass over an empty box: no slice (an np.void of _lib.INTERPOLATE_SUMMARY_DTYPE) and no maps."""
    return np.zeros(1, _lib.INTERPOLATE_SUMMARY_DTYPE)[0], np.zeros((0, 0, 0), np.uint32), np.zeros((0, 0, 0), np.uint8)


def _planar_d2(seeds, weights):
    """Per plane seeds[k] (bool [k, u, v]): the smallest weights[0] * du^2 + weights[1] * dv^2 to a seed of the plane, int64; `far`
    (2^40) in a plane without seeds.  One broadcast minimum per axis, as distance_volume takes it."""
    far = np.int64(1) << 40
    g = np.where(seeds, np.int64(0), far)
    for axis, weight in ((2, weights[1]), (1, weights[0])):
        n = g.shape[axis]
        shape = [1, 1, 1]
        shape[axis] = n
        i = np.arange(n, dtype=np.int64).reshape(shape)
        f = np.full(g.shape, far, np.int64)
        for j in range(n):
            at = [slice(None)] * 3
            at[axis] = slice(j, j + 1)
            np.minimum(f, g[tuple(at)] + weight * (i - j) ** 2, out=f)
        g = np.minimum(f, far)
    return g


def interpolate_volume(prepared, dims, q, labels=None, cut=None, uncut=None):
    """The definition of the interpolate pass (include/volym_hip.h volym_interpolate_pass), NumPy integers only; equal to the device in
    every byte.  `prepared`, `uncut`, `labels` and `cut` are what distance_volume takes.  Returns (summary, map, state): an np.void of
    _lib.INTERPOLATE_SUMMARY_DTYPE, the signed planar map as a uint32 array [z, y, x] over the request's box and the state bytes as a
    uint8 array of the same shape (their bytes are the box-linear maps)."""
    q = check_interpolate(q, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = q.box
    summary, no_map, no_state = empty_interpolate()
    if any(a >= b for a, b in zip(lo, hi)):
        return summary, no_map, no_state
    whole = bool(q.flags & _lib.INTERPOLATE_UNCUT)
    src = np.ascontiguousarray(uncut if (whole and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != nx * ny * nz:
        raise ValueError("interpolate_volume: the density has %d bytes, the volume %d" % (src.size, nx * ny * nz))
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = src.reshape(nz, ny, nx)[sub]
    if labels is None:
        l = np.zeros(b.shape, np.uint8)
    else:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != src.size:
            raise ValueError("interpolate_volume: labels have %d bytes, the volume %d" % (lab.size, src.size))
        l = lab.reshape(nz, ny, nx)[sub]
    none = np.int64(_lib.INTERPOLATE_NONE)
    # slices first: [k, u, v] with (u, v) the two in-plane axes in the order (z, y, x) keeps them
    np_axis = 2 - q.axis
    shape = np.moveaxis((b >= q.min_byte) & (np.asarray(q.select)[l] != 0), np_axis, 0)
    weights = [q.weight[a] for a in (2, 1, 0) if a != q.axis]
    n = shape.shape[0]
    counts = shape.reshape(n, -1).sum(axis=1)
    first = lo[q.axis]
    if q.flags & _lib.INTERPOLATE_KEYS:
        is_key = np.array([(first + k) in set(q.keys) for k in range(n)], bool)
    else:
        is_key = counts > 0
    keys = np.flatnonzero(is_key).tolist()
    word = np.full(shape.shape, none, np.int64)
    state = np.where(shape, _lib.INTERPOLATE_SHAPE, 0).astype(np.uint8)
    if keys:
        s = shape[keys]
        far = np.int64(1) << 40
        d_out, d_in = _planar_d2(s, weights), _planar_d2(~s, weights)
        for axis, weight in ((1, weights[0]), (2, weights[1])):        # texels outside the box are not SHAPE
            m = s.shape[axis]
            at = [1, 1, 1]
            at[axis] = m
            i = np.arange(m, dtype=np.int64).reshape(at)
            d_in = np.minimum(d_in, weight * np.minimum(i + 1, m - i) ** 2)
        word[keys] = np.where(s, d_in << 1 | 1, np.where(d_out < far, d_out << 1, none))
        state[keys] |= np.where(s, _lib.INTERPOLATE_INSIDE, 0).astype(np.uint8)
    rec = summary["slice"]
    rec["key_lo"][:n] = rec["key_hi"][:n] = _lib.INTERPOLATE_NONE
    for k in keys:
        rec[k] = (_lib.INTERPOLATE_SLICE_KEY, first + k, first + k, counts[k])
    n_gaps = n_gap_slices = n_refused = n_inside = n_new = n_stale = 0
    for z0, z1 in zip(keys, keys[1:]):
        if z1 - z0 < 2:
            continue
        if q.max_gap and z1 - z0 - 1 > q.max_gap:
            n_refused += 1
            for z in range(z0 + 1, z1):
                rec[z] = (_lib.INTERPOLATE_SLICE_REFUSED, first + z0, first + z1, 0)
            continue
        n_gaps += 1
        m0, m1 = word[z0], word[z1]
        sh0, sh1 = (m0 != none) & ((m0 & 1) == 1), (m1 != none) & ((m1 & 1) == 1)
        out0, out1 = (m0 != none) & ~sh0, (m1 != none) & ~sh1
        d0, d1 = m0 >> 1, m1 >> 1
        for z in range(z0 + 1, z1):
            a2, b2 = np.int64((z1 - z) ** 2), np.int64((z - z0) ** 2)
            inside = (sh0 & sh1) | (sh0 & out1 & (a2 * d0 > b2 * d1)) | (sh1 & out0 & (b2 * d1 > a2 * d0))
            was = shape[z]
            state[z] |= np.where(inside, _lib.INTERPOLATE_GAP | _lib.INTERPOLATE_INSIDE, _lib.INTERPOLATE_GAP).astype(np.uint8)
            count = int(inside.sum())
            rec[z] = (_lib.INTERPOLATE_SLICE_GAP, first + z0, first + z1, count)
            n_gap_slices += 1
            n_inside += count
            n_new += int((inside & ~was).sum())
            n_stale += int((was & ~inside).sum())
    summary["n_slices"], summary["n_keys"], summary["n_gaps"], summary["n_gap_slices"], summary["n_refused"] = n, len(keys), n_gaps, n_gap_slices, n_refused
    summary["n_shape"], summary["n_inside"], summary["n_new"], summary["n_stale"] = int(counts.sum()), n_inside, n_new, n_stale
    return (summary, np.ascontiguousarray(np.moveaxis(word, 0, np_axis)).astype(np.uint32), np.ascontiguousarray(np.moveaxis(state, 0, np_axis)))


def interpolate_summary(summary):
    """What a user reads off an interpolate pass, as Python ints: the counters of the summary, "keys": the volume coordinates of the
    key slices, "gaps": [(key_lo, key_hi)] of the fillable gaps and "refused": the same of those max_gap refused."""
    n = int(summary["n_slices"])
    rec = summary["slice"][:n]
    out = {k: int(summary[k]) for k in ("n_slices", "n_keys", "n_gaps", "n_gap_slices", "n_refused", "n_shape", "n_inside", "n_new", "n_stale")}
    out["keys"] = [int(r["key_lo"]) for r in rec if int(r["kind"]) == _lib.INTERPOLATE_SLICE_KEY]
    for name, kind in (("gaps", _lib.INTERPOLATE_SLICE_GAP), ("refused", _lib.INTERPOLATE_SLICE_REFUSED)):
        out[name] = sorted(set((int(r["key_lo"]), int(r["key_hi"])) for r in rec if int(r["kind"]) == kind))
    return out


class InterpolateEdit:
    """volym_interpolate_edit (include/volym_hip.h): one edit by the latest interpolate pass.  box and window as Relabel takes them;
    flags: _lib.INTERPOLATE_EDIT_UNCUT | INTERPOLATE_EDIT_DRY_RUN; to: the label an INSIDE texel of a gap slice becomes, out: the label
    every other texel of a gap slice becomes (relabel_table's dicts or 256 labels; None: the identity)."""

    def __init__(self, box=None, flags=0, window=(0, 255), to=None, out=None, dims=None):
        _edit_fields(self, "interpolate edit", box, dims, flags, window, to)
        self.out = relabel_table() if out is None else (relabel_table(out) if isinstance(out, dict) else np.array(out, np.int64).ravel())

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "interpolate edit", ("box", "flags", "window", "to", "out"), kw)

    def to_c(self):
        """The _lib.InterpolateEdit of this request.  Fields that do not fit their C types raise ValueError."""
        c = _edit_fields_to_c(self, _lib.InterpolateEdit(), "interpolate edit", True, "flags and the window's ends must be u32")
        if self.out.size != 256 or not ((self.out >= 0) & (self.out <= 255)).all():
            raise ValueError("interpolate edit: the out table is 256 bytes")
        c.out = (C.c_uint8 * 256)(*[int(g) for g in self.out])
        return c


def check_interpolate_edit(edit, dims):
    """The validity rules of volym_interpolate_labels_check: lo <= hi <= dims on every axis (an empty box is valid), known flag bits,
    min_byte <= max_byte <= 255, tables of 256 entries.  Returns the request; raises ValueError."""
    _check_edit_fields(edit, dims, "interpolate edit", _lib.INTERPOLATE_EDIT_UNCUT | _lib.INTERPOLATE_EDIT_DRY_RUN)
    if np.asarray(edit.out).size != 256:
        raise ValueError("interpolate edit: the out table has 256 entries")
    return edit


def interpolate_labels_volume(prepared, dims, edit, labels, state, pass_box, uncut=None):
    """The definition of the edit (include/volym_hip.h volym_interpolate_labels), NumPy integers only; equal to the device in every
    byte.  `prepared`: the scene bytes as they stand (cuts applied), `uncut`: the uncut copy (read with UNCUT; None: prepared),
    `labels`: the labels before the edit; state: the state map of the latest interpolate pass (interpolate_volume's) over pass_box =
    ((lo), (hi)).  A texel of the box whose state has GAP and whose density byte lies in the window becomes to[l] where its state has
    INSIDE and out[l] where it has not.  Returns (new_labels, result) as relabel_volume does."""
    r = check_interpolate_edit(edit, dims)
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = r.box
    result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
    lab = np.ascontiguousarray(labels, np.uint8).ravel()
    if lab.size != nx * ny * nz:
        raise ValueError("interpolate_labels_volume: labels have %d bytes, the volume %d" % (lab.size, nx * ny * nz))
    new = lab.reshape(nz, ny, nx).copy()
    src = np.ascontiguousarray(uncut if (r.flags & _lib.INTERPOLATE_EDIT_UNCUT and uncut is not None) else prepared, np.uint8).ravel()
    if src.size != lab.size:
        raise ValueError("interpolate_labels_volume: the density has %d bytes, the volume %d" % (src.size, lab.size))
    slo, shi = (tuple(int(v) for v in pass_box[0]), tuple(int(v) for v in pass_box[1]))
    if any(lo[a] < slo[a] or hi[a] > shi[a] for a in range(3)):
        raise ValueError("interpolate_labels_volume: the request's box reaches outside the box of the interpolate pass")
    if any(a >= b for a, b in zip(lo, hi)):
        return new, result
    shape = (shi[2] - slo[2], shi[1] - slo[1], shi[0] - slo[0])
    inner = (slice(lo[2] - slo[2], hi[2] - slo[2]), slice(lo[1] - slo[1], hi[1] - slo[1]), slice(lo[0] - slo[0], hi[0] - slo[0]))
    st = np.asarray(state, np.uint8).reshape(shape)[inner]
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    old = new[sub]
    d = src.reshape(nz, ny, nx)[sub]
    to, out = np.asarray(r.to, np.int64).astype(np.uint8), np.asarray(r.out, np.int64).astype(np.uint8)
    becomes = np.where((st & _lib.INTERPOLATE_INSIDE) != 0, to[old], out[old])
    hit = ((st & _lib.INTERPOLATE_GAP) != 0) & (d >= r.window[0]) & (d <= r.window[1]) & (becomes != old)
    count = int(hit.sum())
    if count == 0:
        return new, result
    result["changed"] = count
    result["left"][...] = np.bincount(old[hit], minlength=256)
    result["arrived"][...] = np.bincount(becomes[hit], minlength=256)
    z, y, x = np.nonzero(hit)
    result["box"][...] = (lo[0] + x.min(), lo[1] + y.min(), lo[2] + z.min(), lo[0] + x.max() + 1, lo[1] + y.max() + 1, lo[2] + z.max() + 1)
    if not r.flags & _lib.INTERPOLATE_EDIT_DRY_RUN:
        new[sub] = np.where(hit, becomes, old)
    return new, result


def relabel_result_dict(result):
    """A relabel result as Python values: {"changed", "left": {label: n}, "arrived": {label: n}, "box": ((lo), (hi)) or None}."""
    box = [int(v) for v in result["box"]]
    return {"changed": int(result["changed"]),
            "left": {int(l): int(result["left"][l]) for l in np.flatnonzero(result["left"])},
            "arrived": {int(l): int(result["arrived"][l]) for l in np.flatnonzero(result["arrived"])},
            "box": (tuple(box[:3]), tuple(box[3:])) if int(result["changed"]) else None}


def label_chunks_changed(dims, old, new, bricked):
    """The number of 16-byte chunks of the device layout in which the label volumes `old` and `new` differ: what one step of the
    label history journals.  Linear: 16 consecutive texels of the x-fastest order (a chunk may wrap rows and slices).  Bricked: the
    4 x 4 patch (x // 4, y // 4) of one z."""
    nx, ny, nz = (int(v) for v in dims)
    at = np.flatnonzero(np.asarray(old, np.uint8).ravel() != np.asarray(new, np.uint8).ravel())
    if not bricked:
        return int(np.unique(at >> 4).size)
    x, y, z = at % nx, (at // nx) % ny, at // (nx * ny)
    bx, by = (nx + 3) // 4, (ny + 3) // 4
    return int(np.unique((z * by + y // 4) * bx + x // 4).size)


def relabel_slab_items(dims, box, bricked):
    """The items the relabel kernel walks for a request over `box` = ((lo), (hi)) (None: the whole volume): the worst case of the
    chunks it can store, which sizes the staging area of the label history.  Bricked: four chunks per brick the box touches.
    Linear: the runs of consecutive bytes the box is made of (rows; whole rows merge into one run per z, whole slices into one
    run), each covered by the aligned chunks it may touch."""
    nx, ny, nz = (int(v) for v in dims)
    lo, hi = ((0, 0, 0), (nx, ny, nz)) if box is None else (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
    if bricked:
        n = [((hi[a] + 3) >> 2) - (lo[a] >> 2) for a in range(3)]
        return 4 * n[0] * n[1] * n[2]
    rows = lo[0] == 0 and hi[0] == nx
    slices = rows and lo[1] == 0 and hi[1] == ny
    run, runs_y, runs_z = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    if rows:
        run, runs_y = run * runs_y, 1
    if slices:
        run, runs_z = run * runs_z, 1
    return ((run + 15) // 16 + 1) * runs_y * runs_z


class LabelHistory:
    """The definition of the label history's rule (include/volym_hip.h volym_label_history), NumPy only: which steps are kept,
    evicted and given up, and what undo and redo restore and report.  info() equals the device's volym_label_history_info field for
    field.  A step keeps the texels that changed with their labels on both sides; what it costs is the device's figure, 20 bytes per
    16-byte chunk of the layout (`bricked`) in which a byte changed."""

    def __init__(self, budget_bytes, dims, bricked):
        self.dims, self.bricked = tuple(int(v) for v in dims), bool(bricked)
        self.budget = 0
        self.steps, self.cursor = [], 0           # oldest first: [0, cursor) can be undone, the rest redone (the nearest first)
        self.dropped = self.lost = 0
        self.set_budget(budget_bytes)

    def set_budget(self, budget_bytes):
        """volym_label_history: 0 drops everything, counters included; another budget keeps the steps that still fit."""
        budget_bytes = int(budget_bytes)
        if budget_bytes == 0:
            self.budget, self.steps, self.cursor, self.dropped, self.lost = 0, [], 0, 0, 0
            return
        if self.budget == 0:
            self.dropped = self.lost = 0
        self.budget = budget_bytes
        self._fit()

    def used(self):
        return _lib.JOURNAL_RECORD_BYTES * sum(s["records"] for s in self.steps)

    def _fit(self):
        # the oldest undoable steps go first; when none is left, the redo steps that would be redone last
        while self.used() > self.budget and self.steps:
            if self.cursor > 0:
                self.steps.pop(0)
                self.cursor -= 1
            else:
                self.steps.pop()
            self.dropped += 1

    def clear(self):
        """What volym_set_labels, volym_set_volume and volym_set_importances do to the history: the steps go, the rest stays."""
        self.steps, self.cursor = [], 0

    def record(self, old, new, slab_items=None, box=None):
        """An edit took the labels from `old` to `new`.  slab_items: the items of the request's slab (relabel_slab_items; default:
        those of `box`, or of the whole volume).  Returns True when a step was kept."""
        if self.budget == 0:
            return False
        old, new = np.asarray(old, np.uint8).ravel(), np.asarray(new, np.uint8).ravel()
        at = np.flatnonzero(old != new)
        if at.size == 0:
            return False
        del self.steps[self.cursor:]                                  # a recorded edit drops all redo steps
        records = label_chunks_changed(self.dims, old, new, self.bricked)
        items = relabel_slab_items(self.dims, box, self.bricked) if slab_items is None else int(slab_items)
        if records > min(items, self.budget // _lib.JOURNAL_RECORD_BYTES):
            self.steps, self.cursor = [], 0                           # the whole history is given up: no undo across a gap
            self.lost += 1
            return False
        self.steps.append({"at": at, "before": old[at].copy(), "after": new[at].copy(), "records": records})
        self.cursor = len(self.steps)
        self._fit()
        return True

    def _swap(self, labels, step, a, b):
        nx, ny, nz = self.dims
        out = np.array(labels, np.uint8).ravel()
        at = step["at"]
        if not np.array_equal(out[at], step[a]):
            raise ValueError("LabelHistory: the labels are not those the step left")
        out[at] = step[b]
        result = np.zeros(1, _lib.RELABEL_RESULT_DTYPE)[0]
        result["changed"] = at.size
        result["left"][...] = np.bincount(step[a], minlength=256)
        result["arrived"][...] = np.bincount(step[b], minlength=256)
        x, y, z = at % nx, (at // nx) % ny, at // (nx * ny)
        result["box"][...] = (x.min(), y.min(), z.min(), x.max() + 1, y.max() + 1, z.max() + 1)
        return out, result

    def undo(self, labels):
        """(labels with the newest undoable step taken back [flat], result); ValueError when there is none (the device: E_STATE)."""
        if self.budget == 0 or self.cursor == 0:
            raise ValueError("LabelHistory: nothing to undo")
        self.cursor -= 1
        return self._swap(labels, self.steps[self.cursor], "after", "before")

    def redo(self, labels):
        """(labels with the newest undone step carried out again [flat], result); ValueError when there is none."""
        if self.budget == 0 or self.cursor == len(self.steps):
            raise ValueError("LabelHistory: nothing to redo")
        self.cursor += 1
        return self._swap(labels, self.steps[self.cursor - 1], "before", "after")

    def info(self):
        """volym_label_history_info as GpuContext.label_history_info returns it."""
        undo, redo = self.cursor, len(self.steps) - self.cursor
        return {"budget_bytes": self.budget, "used_bytes": self.used(), "undo_steps": undo, "redo_steps": redo,
                "next_undo_records": self.steps[self.cursor - 1]["records"] if undo else 0,
                "next_redo_records": self.steps[self.cursor]["records"] if redo else 0,
                "dropped_steps": self.dropped, "lost": self.lost}


PROJECT_STEP_MIN, PROJECT_STEP_MAX = 1.0e-4, 1.0     # volym_update's range for the march step


class Projection:
    """volym_project (include/volym_hip.h): what one projection pass computes and shows.  step: the distance between the samples
    of a ray; mode: _lib.PROJECT_MAX / PROJECT_MEAN (what the image shows; a record holds both); flags: PROJECT_TF | PROJECT_LABELS
    | PROJECT_NO_SKIP; background: the image's colour where a ray misses the cube; palette: (256, 4) uint8, colour per label
    value with alpha = strength (PROJECT_LABELS)."""

    def __init__(self, step, mode=_lib.PROJECT_MAX, flags=0, background=(0, 0, 0, 255), palette=None):
        self.step, self.mode, self.flags = float(step), int(mode), int(flags)
        self.background = tuple(int(v) for v in background)
        self.palette = np.zeros((256, 4), np.uint8) if palette is None else np.array(palette, np.uint8).reshape(256, 4)

    def replace(self, **kw):
        """A copy with the given fields changed."""
        return _replaced(self, "projection", ("step", "mode", "flags", "background", "palette"), kw)

    def to_c(self):
        """The _lib.Project of this projection.  Fields that do not fit their C types raise ValueError."""
        c = _lib.Project()
        c.step = self.step
        for name in ("mode", "flags"):
            v = getattr(self, name)
            if not 0 <= v < 2 ** 32:
                raise ValueError("projection: %s = %d is not a u32" % (name, v))
            setattr(c, name, v)
        c.background = (C.c_uint8 * 4)(*[int(v) for v in _rgba(self.background, "background")])
        C.memmove(c.palette, _u8p(np.ascontiguousarray(self.palette, np.uint8)), 1024)
        return c

    @classmethod
    def from_c(cls, c):
        return cls(c.step, c.mode, c.flags, tuple(c.background), np.ctypeslib.as_array(c.palette).copy())


def check_projection(p):
    """The validity rules of volym_project_check: a finite step in [1e-4, 1] (as float32), a known mode, known flag bits, no
    LABELS with MEAN.  Returns the projection; raises ValueError."""
    step = np.float32(p.step)
    if not (np.isfinite(step) and np.float32(PROJECT_STEP_MIN) <= step <= np.float32(PROJECT_STEP_MAX)):
        raise ValueError("projection: the step must be in [1e-4, 1], got %r" % (p.step,))
    if p.mode not in (_lib.PROJECT_MAX, _lib.PROJECT_MEAN):
        raise ValueError("projection: unknown mode %r" % (p.mode,))
    if p.flags & ~(_lib.PROJECT_TF | _lib.PROJECT_LABELS | _lib.PROJECT_NO_SKIP) or p.flags < 0:
        raise ValueError("projection: unknown flag bits in %#x" % p.flags)
    if p.mode == _lib.PROJECT_MEAN and p.flags & _lib.PROJECT_LABELS:
        raise ValueError("projection: LABELS with MEAN (a mean has no texel to take a label from)")
    return p


def project_samples(t_entry, t_exit, step):
    """The count rule of the projection (volym_project_samples), as the loop it is defined by: the number of k = 0, 1, 2, ... with
    t_entry + float32(k) * step < t_exit in float32.  Arrays or scalars (broadcast); returns int64 of their common shape."""
    F = np.float32
    te, tx, st = np.broadcast_arrays(np.asarray(t_entry, F), np.asarray(t_exit, F), np.asarray(step, F))
    shape = te.shape
    te, tx, st = te.ravel(), tx.ravel(), st.ravel()
    n = np.zeros(te.size, np.int64)
    idx = np.arange(te.size)
    k = 0
    while idx.size:
        idx = idx[te[idx] + F(k) * st[idx] < tx[idx]]
        n[idx] += 1
        k += 1
    return n.reshape(shape)


def project_rays(camera_uniforms, W, H, gx, gy):
    """The rays of the pixels (gx[i], gy[i]) of the W x H frame (wgsl:221-241), restated in float32 operation for operation.
    -> (o[3], d[n, 3], t_entry[n], t_exit[n], hit[n])"""
    F = np.float32
    zero, one = F(0.0), F(1.0)
    ivp = np.array(camera_uniforms.inverse_view_proj, F)          # [col][row]
    o = np.array(list(camera_uniforms.camera_position), F)
    gx = np.asarray(gx).ravel().astype(F)
    gy = np.asarray(gy).ravel().astype(F)
    ndx = (gx / F(W)) * F(2.0) - one
    ndy = one - (gy / F(H)) * F(2.0)
    wp = [((ivp[0][r] * ndx + ivp[1][r] * ndy) + ivp[2][r] * zero) + ivp[3][r] * one for r in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = [wp[a] / wp[3] - o[a] for a in range(3)]
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        d = [c / ln for c in v]
        t1 = [(zero - o[a]) / d[a] for a in range(3)]
        t2 = [(one - o[a]) / d[a] for a in range(3)]
    lo = [np.fmin(a, b) for a, b in zip(t1, t2)]
    hi = [np.fmax(a, b) for a, b in zip(t1, t2)]
    t_entry = np.fmax(np.fmax(np.fmax(lo[0], lo[1]), lo[2]), zero).astype(F)
    t_exit = np.fmax(np.fmin(np.fmin(hi[0], hi[1]), hi[2]), zero).astype(F)
    with np.errstate(invalid="ignore"):
        hit = ~(t_exit <= t_entry)
    return o, np.stack(d, 1).astype(F), t_entry, t_exit, hit


def _project_texels(o, d, t, dims):
    """clamp(floor(pos * n), 0, n - 1) of pos = o + d * t, per axis (the march's nearest fetch)"""
    F = np.float32
    out = []
    for a in range(3):
        f = np.floor((o[a] + d[:, a] * t) * F(dims[a]))
        f = np.where(f >= F(0.0), f, F(0.0))                       # also NaN -> 0
        out.append(np.minimum(f, F(dims[a] - 1)).astype(np.int64))
    return out


def project_frame(prepared, dims, camera_uniforms, W, H, projection, rect=None, lut=None, labels=None):
    """The definition of the projection pass (include/volym_hip.h volym_project_pass); equal to the device in every byte.
    `prepared`: the density bytes of the scene as it stands (box, plane and mask applied: cut_volume); camera_uniforms: those of
    the last update; rect = (x0, y0, w, h), None: the whole frame; `lut`: the RGBA8 bytes set_transfer_function received
    (PROJECT_TF); `labels`: prepared label bytes of the volume's dimensions, None: none on the device (PROJECT_LABELS needs them).
    Every sample of every ray is read: PROJECT_NO_SKIP changes nothing here.  Returns (records, image): (h, w) of
    _lib.PROJECTION_DTYPE and (h, w, 4) uint8."""
    F = np.float32
    p = check_projection(projection)
    nx, ny, nz = (int(v) for v in dims)
    x0, y0, w, h = (0, 0, int(W), int(H)) if rect is None else (int(v) for v in rect)
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError("project_frame: the rect must be non-empty and inside the frame")
    vol = np.ascontiguousarray(prepared, np.uint8).ravel()
    if vol.size != nx * ny * nz:
        raise ValueError("project_frame: the density has %d bytes, the volume %d" % (vol.size, nx * ny * nz))
    gy, gx = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    o, d, t_entry, t_exit, hit = project_rays(camera_uniforms, W, H, gx.ravel(), gy.ravel())
    n = hit.size
    step = F(p.step)
    best = np.zeros(n, np.int64)
    best_k = np.zeros(n, np.int64)
    total = np.zeros(n, np.int64)
    count = np.zeros(n, np.int64)
    idx = np.flatnonzero(hit)
    k = 0
    while idx.size:
        t = t_entry[idx] + F(k) * step
        keep = t < t_exit[idx]
        idx, t = idx[keep], t[keep]
        ix, iy, iz = _project_texels(o, d[idx], t, (nx, ny, nz))
        b = vol[ix + nx * (iy + ny * iz)].astype(np.int64)
        total[idx] += b
        count[idx] += 1
        up = b > best[idx]                                          # strictly greater: the smallest k keeps the maximum
        best[idx[up]] = b[up]
        best_k[idx[up]] = k
        k += 1

    rec = np.zeros(n, _lib.PROJECTION_DTYPE)
    found = hit & (best > 0)
    rec["status"] = np.where(found, 2, np.where(hit, 1, 0))
    rec["max"] = best
    rec["n_samples"] = count
    rec["mean"] = np.where(hit, (2 * total + count) // np.maximum(2 * count, 1), 0)
    rec["t"] = F(-1.0)
    f = np.flatnonzero(found)
    tb = t_entry[f] + best_k[f].astype(F) * step
    rec["t"][f] = tb
    ix, iy, iz = _project_texels(o, d[f], tb, (nx, ny, nz))
    rec["x"][f], rec["y"][f], rec["z"][f] = ix, iy, iz
    if labels is not None:
        lab = np.ascontiguousarray(labels, np.uint8).ravel()
        if lab.size != nx * ny * nz:
            raise ValueError("project_frame: the labels have %d bytes, the volume %d" % (lab.size, nx * ny * nz))
        rec["label"][f] = lab[ix + nx * (iy + ny * iz)]
    elif p.flags & _lib.PROJECT_LABELS:
        raise ValueError("project_frame: PROJECT_LABELS needs labels")

    rec = rec.reshape(h, w)
    return rec, project_image(rec, p, lut)


def project_image(records, projection, lut=None):
    """The image rules of the projection pass (include/volym_hip.h at volym_project), from the records of the same rays: a miss
    is `background`; otherwise v = max or mean by the mode, the base (v, v, v, 255) or, with PROJECT_TF, the r, g, b of texel
    (v * tf_n) >> 8 of `lut` with alpha 255; with PROJECT_LABELS and status 2, palette[label] blended over it by the outline's
    formula.  Returns uint8 of the records' shape + (4,)."""
    p = check_projection(projection)
    rec = np.asarray(records)
    if rec.dtype != _lib.PROJECTION_DTYPE:
        raise ValueError("the records are an array of PROJECTION_DTYPE")
    v = (rec["mean"] if p.mode == _lib.PROJECT_MEAN else rec["max"]).astype(np.int64)
    base = np.empty(rec.shape + (4,), np.uint8)
    if p.flags & _lib.PROJECT_TF:
        if lut is None:
            raise ValueError("project_image: PROJECT_TF needs the transfer function's RGBA8 bytes")
        table = np.ascontiguousarray(lut, np.uint8).reshape(-1, 4)
        base[:] = table[(v * table.shape[0]) >> 8]
    else:
        base[..., 0] = base[..., 1] = base[..., 2] = v
    base[..., 3] = 255
    if p.flags & _lib.PROJECT_LABELS:
        f = rec["status"] == 2
        base[f] = outline_blend_each(base[f], np.ascontiguousarray(p.palette, np.uint8).reshape(256, 4)[rec["label"][f]])
    hit = rec["status"] != 0
    image = np.empty(rec.shape + (4,), np.uint8)
    image[:] = np.array(_rgba(p.background, "background"), np.uint8)
    image[hit] = base[hit]
    return image


def outline_blend_each(src, col):
    """outline_blend with a colour per pixel: src and col are (n, 4) uint8, col's alpha byte is the strength"""
    col = np.asarray(col, np.uint8).astype(np.uint32)
    a8 = col[:, 3:4].copy()
    col[:, 3] = 255
    return ((np.asarray(src, np.uint8).astype(np.uint32) * (255 - a8) + col * a8 + 127) // 255).astype(np.uint8)


def map_segments_to_importance(labels, segments):
    """src/demos/simple/importance.rs:148-158"""
    data = np.array(labels, np.uint8, copy=True).ravel()
    lv = np.array([s["label_value"] for s in segments], np.uint8)
    im = np.array([s["importance"] for s in segments], np.uint8)
    _lib.check(_lib.lib().volym_map_segments_to_importance(_u8p(data), data.size, _u8p(lv), _u8p(im), len(segments)))
    return data
