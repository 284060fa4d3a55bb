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


def map_segments_to_importance(labels, segments):
    """src/demos/simple/importance.rs:148-158"""
    data = np.array(labels, np.uint8, copy=True).ravel()
    lv = np.array([s["label_value"] for s in segments], np.uint8)
    im = np.array([s["importance"] for s in segments], np.uint8)
    _lib.check(_lib.lib().volym_map_segments_to_importance(_u8p(data), data.size, _u8p(lv), _u8p(im), len(segments)))
    return data
