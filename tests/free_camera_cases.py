"""The cases of the camera axis, shared by tests/test_oracle_free_cameras.py (which pins the oracle on them and asserts that they
are worth drawing) and tests/test_gpu_free_cameras.py (which draws them on the device).  Inputs, the enumeration of cases and what
each case declares about itself only: no expected pixels live here.  The oracle's frame of a case is rendered once per process.

Every other GPU test looks through oracle.benchmark_camera_uniforms: an orbit about the cube's centre at distance 1 to 10, no
roll, fovy 90, znear 0.01.  The cameras here are what volym_update also takes: any position, target, up, field of view, aspect and
near plane, and uniforms whose camera_position is not the centre of projection of their matrix ("displaced eyes").

What is kept out: every eye is at least 1e-3 away from the six face planes of the cube, and off the lines where a ray's direction
component and the matching slab numerator are both 0.  There the slab test (wgsl:162-179) forms 0/0, the NaN ends in WGSL's min /
max, whose result for a NaN operand the language leaves to the implementation, and the oracle does not pin it."""
import math

import numpy as np

from tests import common

OCTANT_DIMS = (40, 36, 44)
BALL_CENTRE, BALL_RADIUS = (0.72, 0.7, 0.3), 0.2
SIZES = [(96, 64), (80, 60)]
RAGGED = (37, 23)
CROSS = (24, 16)                    # the frame of the C oracle against the NumPy oracle
STEP = 0.01
SLACK_PIXELS = 0.375                # include/volym_hip.h VOLYM_VIEW_EYE_SLACK_PIXELS

MODES = [
    ("base", dict()),
    ("importance straight", dict(use_importance_rendering=1, importance_check_ahead_steps=6)),
    ("importance cone", dict(use_importance_rendering=1, use_cone_importance_check=1, importance_check_ahead_steps=6)),
    ("smoothed", dict(use_gaussian_smoothing=1, density_threshold=0.12)),
]

_scenes = {}


def scene(name):
    """-> (dims, volume, importances): prepared bytes, the same for the oracle and the device"""
    if name in _scenes:
        return _scenes[name]
    if name == "bonsai":
        from oracle import oracle as O
        raw, labels = common.bonsai(64)
        dims = (64, 64, 64)
        vol, imp = common.oracle_scene(O, raw, labels, common.BONSAI_SEGMENTS, dims)
        out = (dims, vol, imp)
    elif name == "octant":
        # a ball in one corner octant, faint noise below every threshold elsewhere: the AABB of the occupied cells is a small part
        # of the cube, and an eye can be inside the cube and outside that AABB.  Three voxels in ten of the ball are important, so
        # a look-ahead finds something whichever way its probes walk (their step is negative where |pos| exceeds t_exit, wgsl:145).
        nx, ny, nz = OCTANT_DIMS
        rng = np.random.default_rng(41)
        zz, yy, xx = np.meshgrid(*((np.arange(d) + 0.5) / d for d in (nz, ny, nx)), indexing="ij")
        r = np.sqrt((xx - BALL_CENTRE[0]) ** 2 + (yy - BALL_CENTRE[1]) ** 2 + (zz - BALL_CENTRE[2]) ** 2)
        vol = np.where(r < BALL_RADIUS, 90 + 150 * (1.0 - r / BALL_RADIUS), rng.integers(0, 6, r.shape)).astype(np.uint8).ravel()
        imp = np.where((r < BALL_RADIUS) & (rng.random(r.shape) < 0.3), 255, 0).astype(np.uint8).ravel()
        out = (OCTANT_DIMS, vol, imp)
    else:
        raise KeyError(name)
    _scenes[name] = out
    return out


class Case:
    """One camera on one scene at one frame size.
    cam: fields of oracle.Camera (position, target, up, fovy, znear, aspect; aspect defaults to W / H).
    shift: None, or (axis, amount): camera_position moved by `amount` along the view matrix's "right", "up" or "forward" vector
    after the uniforms were built -- the matrix keeps its centre of projection.
    floor: what the oracle's base frame must at least show -- non-constant pixels ("pixels"), n_hit, n_steps, n_dense; a case that
    declares pixels == 0 must show exactly none.
    culled: whether compute_culling may use its devices for these uniforms (a consistent eye, or one displaced by less than the
    slack).  catches: a displaced eye whose picture leaves the consistent camera's picture by more than the culling margins."""

    def __init__(self, name, scene_name, size, cam, floor, shift=None, culled=True, catches=False, of=None):
        self.name, self.scene, self.size, self.cam, self.floor = name, scene_name, tuple(size), dict(cam), dict(floor)
        self.shift, self.culled, self.catches, self.of = shift, culled, catches, of

    def __repr__(self):
        return "%s (%s, %dx%d)" % (self.name, self.scene, self.size[0], self.size[1])

    def camera(self, O):
        W, H = self.size
        c = O.camera_default(self.cam.get("aspect", W / H), self.cam["position"])
        for k in ("target", "up"):
            if k in self.cam:
                for i in range(3):
                    getattr(c, k)[i] = self.cam[k][i]
        for k in ("fovy", "znear"):
            if k in self.cam:
                setattr(c, k, self.cam[k])
        return c

    def uniforms(self, O):
        u = O.camera_uniforms(self.camera(O))
        if self.shift:
            axis, amount = self.shift
            v = view_axes(u)[axis]
            for i in range(3):
                u.camera_position[i] = float(np.float32(u.camera_position[i]) + np.float32(amount * v[i]))
        return u

    def parameters(self, O, mode):
        kw = dict(raymarching_step_size=STEP)
        kw.update(dict(MODES)[mode])
        return O.make_parameters(**kw)


def view_axes(u):
    """right, up and forward of a look-at view matrix (column-major: m[c][r]), as float64 triples"""
    m = u.view_matrix
    return {"right": [float(m[i][0]) for i in range(3)], "up": [float(m[i][1]) for i in range(3)],
            "forward": [-float(m[i][2]) for i in range(3)]}


def _roll(position, target, degrees):
    """an `up` rolled about the view direction by `degrees` from +y, and deliberately not orthogonal to that direction"""
    f = np.subtract(target, position)
    f = f / np.linalg.norm(f)
    s = np.cross(f, (0.0, 1.0, 0.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    a = math.radians(degrees)
    return tuple(float(v) for v in (math.cos(a) * u + math.sin(a) * s + 0.3 * f))


INSIDE_EMPTY = (0.35, 0.4, 0.62)            # inside the cube, 0.1 and more away from the ball's cells on every axis
INSIDE_MATTER = (0.7, 0.68, 0.33)           # inside the ball
OUTSIDE = (1.15, 0.78, 1.02)                # off every axis, 0.9 from the centre
BALL_VIEW = (1.2, 0.95, 0.85)               # the ball from outside the cube
GRAZE = (0.45, 0.6, 1.02)                   # 0.02 outside the face z = 1

Z = dict(pixels=0, n_hit=0, n_steps=0, n_dense=0)


def _floor(pixels, n_hit, n_steps, n_dense):
    return dict(pixels=pixels, n_hit=n_hit, n_steps=n_steps, n_dense=n_dense)


def consistent_cases():
    b, o = "bonsai", "octant"
    A, B = SIZES
    out = [
        Case("inside the cube, outside the AABB, looking at the matter", o, A, dict(position=INSIDE_EMPTY, target=BALL_CENTRE), _floor(350, 6144, 300000, 7000)),
        Case("inside the cube, looking away from the matter", o, B, dict(position=INSIDE_EMPTY, target=(0.0, 0.1, 0.94)), _floor(0, 4800, 150000, 0)),
        Case("inside the matter", o, A, dict(position=INSIDE_MATTER, target=(0.9, 0.75, 0.1)), _floor(6144, 6144, 30000, 30000)),
        Case("inside the bonsai's cube", b, B, dict(position=(0.5, 0.75, 0.85), target=(0.5, 0.35, 0.4)), _floor(800, 4800, 250000, 15000)),
        Case("panned: the cube cut by two frame edges", b, A, dict(position=OUTSIDE, target=(0.3, 1.2, 1.0)), _floor(350, 1500, 100000, 3000)),
        Case("panned: the ball cut by two frame edges", o, B, dict(position=BALL_VIEW, target=(0.3, 1.3, 0.8)), _floor(150, 1200, 70000, 3500)),
        Case("panned until the cube is off screen", b, A, dict(position=OUTSIDE, target=(3.5, 0.9, 0.3)), Z),
        Case("looking away: the cube behind the eye", o, B, dict(position=BALL_VIEW, target=(2.1, 1.2, 1.9)), Z),
        Case("rolled by 30 degrees", b, A, dict(position=OUTSIDE, up=_roll(OUTSIDE, (0.5, 0.5, 0.5), 30.0)), _floor(350, 2500, 150000, 5000)),
        Case("rolled by 90 degrees", o, B, dict(position=BALL_VIEW, target=(0.7, 0.7, 0.3), up=_roll(BALL_VIEW, (0.7, 0.7, 0.3), 90.0)), _floor(150, 1600, 120000, 3000)),
        Case("fovy 20", b, B, dict(position=(2.1, 1.2, 2.4), fovy=20.0), _floor(1000, 4800, 220000, 15000)),
        Case("fovy 140", o, A, dict(position=(0.95, 0.85, 0.62), target=(0.7, 0.7, 0.3), fovy=140.0), _floor(90, 6144, 200000, 2000)),
        Case("aspect 0.6 on a 96x64 frame", b, A, dict(position=OUTSIDE, aspect=0.6), _floor(900, 4000, 300000, 12000)),
        Case("znear 0.5", o, A, dict(position=BALL_VIEW, target=(0.7, 0.7, 0.3), znear=0.5), _floor(170, 2200, 160000, 3500)),
        Case("znear 0.001", b, B, dict(position=OUTSIDE, znear=0.001), _floor(330, 1900, 120000, 4500)),
        Case("distance 40", b, A, dict(position=(23.4, 14.2, 31.2)), _floor(1, 1, 50, 10)),
        Case("0.02 outside a face, looking along it", o, B, dict(position=GRAZE, target=(0.95, 0.72, 0.9)), _floor(200, 1800, 130000, 4500)),
        Case("0.02 outside a face, looking along it, bonsai", b, A, dict(position=(0.35, 0.4, 1.02), target=(0.9, 0.45, 0.97)), _floor(330, 2100, 180000, 5500)),
        Case("ragged frame, inside the cube", o, RAGGED, dict(position=INSIDE_EMPTY, target=BALL_CENTRE), _floor(40, 851, 40000, 900)),
        Case("ragged frame, panned", b, RAGGED, dict(position=OUTSIDE, target=(0.2, 1.3, 0.9)), _floor(30, 200, 12000, 250)),
    ]
    return out


# the consistent cameras whose eye is then moved
DISPLACED_BASE = Case("ball from outside", "octant", (96, 64), dict(position=BALL_VIEW, target=(0.7, 0.7, 0.3)), _floor(170, 2200, 160000, 3500))
NEAR_SIZE = (128, 80)               # the largest frame of the axis: see displaced_cases
DISPLACED_BASE_NEAR = Case("ball from outside, fovy 40, znear 0.001", "octant", NEAR_SIZE, dict(position=(1.2, 0.98, 0.86), target=(0.6, 0.66, 0.3), fovy=40.0, znear=0.001),
                           _floor(1900, 8000, 550000, 40000))


def displaced_cases():
    """camera_position moved off the matrix's centre of projection.  The first three pass the test of clip w alone that
    compute_culling used to make; all of them but the last are further off than the slack.  A move along the view axis rescales
    the picture about the principal point by w_N / (w_N - move), so it shows only under a small near plane (w_N = 0.002 for znear
    0.001: 12 % for a move the old test let through) and on a picture that fills the frame: fovy 40, the ball off-centre, 128x80.
    At 96x64 the same pose puts exactly 16 pixels outside the consistent picture's rectangle, the least the oracle test asks for."""
    f = _floor(95, 1800, 120000, 2000)
    A, N = DISPLACED_BASE, DISPLACED_BASE_NEAR
    mk = lambda name, base, shift, **kw: Case(name, base.scene, base.size, base.cam, kw.pop("floor", f), shift=shift, of=base, **kw)
    return [
        mk("eye moved 0.01 to the right", A, ("right", 0.01), culled=False, catches=True),
        mk("eye moved 0.01 up", A, ("up", 0.01), culled=False, catches=True),
        mk("eye moved 2.5e-4 backwards, znear 0.001", N, ("forward", -2.5e-4), culled=False, catches=True, floor=_floor(2400, 8000, 550000, 50000)),
        mk("eye moved 0.005 forwards", A, ("forward", 0.005), culled=False),
        mk("eye moved 1e-4 to the right: inside the slack", A, ("right", 1.0e-4), culled=True),
    ]


def all_cases():
    return consistent_cases() + [DISPLACED_BASE, DISPLACED_BASE_NEAR] + displaced_cases()


def by_name(name):
    for c in all_cases():
        if c.name == name:
            return c
    raise KeyError(name)


NAMES = [c.name for c in all_cases()]

# subsets of the device tests: each holds an eye inside the cube and a panned camera
SUBSET = ["inside the cube, outside the AABB, looking at the matter", "inside the bonsai's cube", "panned: the cube cut by two frame edges",
          "panned: the ball cut by two frame edges"]
RAGGED_NAMES = ["ragged frame, inside the cube", "ragged frame, panned"]
BOUNDS_NAMES = ["inside the cube, outside the AABB, looking at the matter", "panned: the ball cut by two frame edges"]
PICK_NAMES = ["inside the cube, outside the AABB, looking at the matter", "inside the matter", "rolled by 30 degrees", "panned: the cube cut by two frame edges"]


_refs = {}


def reference(O, case, mode="base", filt=0, size=None):
    """The C oracle's (rgba32f, rgba8, counters) of a case under a mode; rendered once, shared, never written to"""
    key = (case.name, mode, filt, size)
    if key not in _refs:
        dims, vol, imp = scene(case.scene)
        W, H = size or case.size
        f, u, k = O.render(vol, imp, dims, O.tf_default_lut(), case.uniforms(O), case.parameters(O, mode), W, H, filter=filt)
        f.setflags(write=False)
        u.setflags(write=False)
        _refs[key] = (f, u, k)
    return _refs[key]


def non_constant(frame_f32):
    """the pixels that are neither a miss, (0, 0, 0, 1), nor a hit that saw nothing dense, (0, 0, 0, 0): [H, W] bool"""
    f = np.asarray(frame_f32)
    return (f[..., :3] != 0).any(axis=-1) | ((f[..., 3] != 0) & (f[..., 3] != 1))


# ---- the consistency bound, restated in float64 ("a consistent eye") ------------------------------------------------

def eye_displacement(u, W, H, w_min=0.0):
    """The largest distance, in pixels, between a ray's pixel and the projection of a point of that ray with clip w >= w_min
    (w_min <= 0: any point beyond the near plane), for uniforms u: numpy float64 from the f32 fields, nothing shared with the
    library.  ndc(X) - n = (1 - s)(e.xy - n e.w) / w_X for X = (1 - s) E + s N, e = clip(E), and s = (w_X - e.w) / (w_N - e.w)."""
    ivp = np.array([[u.inverse_view_proj[c][r] for c in range(4)] for r in range(4)], np.float64)       # ivp[r, c]
    M = np.linalg.inv(ivp)
    e = M @ np.array([u.camera_position[0], u.camera_position[1], u.camera_position[2], 1.0], np.float64)
    wn = [1.0 / (ivp[3, 0] * sx + ivp[3, 1] * sy + ivp[3, 3]) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)]
    assert min(wn) > 0.0
    ew = abs(e[3])
    if not ew < min(wn):
        return math.inf
    g = 1.0
    if w_min > 0.0:
        if not ew < w_min:
            return math.inf
        g = max(1.0, max(wn) / w_min - 1.0)
    k = g / (min(wn) - ew)
    return max((abs(e[0]) + ew) * k * 0.5 * W, (abs(e[1]) + ew) * k * 0.5 * H)


def old_w_test(u):
    """what compute_culling asked before: |clip w of camera_position| <= 1e-4 |w row|_1"""
    ivp = np.array([[u.inverse_view_proj[c][r] for c in range(4)] for r in range(4)], np.float64)
    M = np.linalg.inv(ivp)
    e = M @ np.array([u.camera_position[0], u.camera_position[1], u.camera_position[2], 1.0], np.float64)
    return abs(e[3]) <= 1e-4 * np.abs(M[3]).sum()
