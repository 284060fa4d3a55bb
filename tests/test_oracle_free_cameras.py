"""The camera axis on the CPU: tests/free_camera_cases.py's cameras through the C oracle, the NumPy oracle and the host shim.

Every case must be worth drawing (its oracle frame shows what its entry declares), the two oracles must agree on it, the host
shim must build the oracle's uniforms for its camera byte for byte, and the displaced eyes must be classified by the consistency
bound the way the case list says -- by the library (volym_view_eye_displacement) and by a float64 restatement that shares nothing
with it.  tests/test_gpu_free_cameras.py draws the same cases on the device.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import free_camera_cases as FC
from tests.test_oracle_crosscheck import _compare

CASES = FC.all_cases()
IDS = [c.name for c in CASES]


def test_the_list_is_whole():
    """what the other tests lean on: unique names, every subset names existing cases, every displaced case has its base"""
    assert len(set(IDS)) == len(IDS) == 27
    for name in FC.SUBSET + FC.RAGGED_NAMES + FC.BOUNDS_NAMES + FC.PICK_NAMES:
        FC.by_name(name)
    for c in FC.displaced_cases():
        assert c.of is not None and c.of.name in IDS and c.shift is not None
    assert {c.size for c in CASES} == set(FC.SIZES) | {FC.RAGGED, FC.NEAR_SIZE}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_eye_keeps_off_the_undefined_rays(oracle, case):
    """at least 1e-3 from the six face planes: both slab numerators of every axis, 0 - o and 1 - o (wgsl:162-179), are then away
    from 0 in f32, so a direction component of 0 gives +-inf and never 0/0"""
    u = case.uniforms(oracle)
    e = [float(u.camera_position[i]) for i in range(3)]
    assert all(abs(v) >= 1e-3 and abs(v - 1.0) >= 1e-3 for v in e), e


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c_and_numpy_oracles_agree(oracle, case):
    """the criterion of tests/test_oracle_crosscheck.py (counters equal, floats within 1e-6, bytes equal), on the case's uniforms at
    24x16, under the four modes"""
    from oracle import oracle_np
    dims, vol, imp = FC.scene(case.scene)
    W, H = FC.CROSS
    u, lut = case.uniforms(oracle), oracle.tf_default_lut()
    for mode, _ in FC.MODES:
        par = case.parameters(oracle, mode)
        a = oracle.render(vol, imp, dims, lut, u, par, W, H, threads=2)
        b = oracle_np.render(vol, imp, dims, lut, u, par, W, H)
        _compare(a, b, "%r, %s" % (case, mode))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_worth_drawing(oracle, case):
    f32, _, k = FC.reference(oracle, case)
    assert not np.isnan(f32).any()
    pixels = int(FC.non_constant(f32).sum())
    if case.floor["pixels"] == 0:
        assert pixels == 0, "%r: declared to show nothing, shows %d pixels" % (case, pixels)
    assert pixels >= case.floor["pixels"], (case, pixels)
    for key in ("n_hit", "n_steps", "n_dense"):
        assert k[key] >= case.floor[key], (case, key, k[key])
    if case.name in ("panned until the cube is off screen", "looking away: the cube behind the eye"):
        assert case.floor == FC.Z and k["n_hit"] == 0 and (np.asarray(f32) == np.float32([0, 0, 0, 1])).all()
    for mode, _ in FC.MODES[1:]:
        assert not np.isnan(FC.reference(oracle, case, mode)[0]).any()


def test_modes_differ_where_there_is_matter(oracle):
    """the four parameter sets are four pictures on a case with matter of both importances in view"""
    case = FC.by_name("inside the cube, outside the AABB, looking at the matter")
    frames = [FC.reference(oracle, case, mode)[1] for mode, _ in FC.MODES]
    for i in range(4):
        for j in range(i):
            assert (frames[i] != frames[j]).any(axis=-1).sum() >= 16, (FC.MODES[i][0], FC.MODES[j][0])


def _outside_the_base_picture(oracle, case):
    base = FC.non_constant(FC.reference(oracle, case.of)[0])
    moved = FC.non_constant(FC.reference(oracle, case)[0])
    ys, xs = np.nonzero(base)
    W, H = case.size
    gx, gy = np.arange(W)[None, :], np.arange(H)[:, None]
    beyond = (gx < xs.min() - 3) | (gx > xs.max() + 3) | (gy < ys.min() - 3) | (gy > ys.max() + 3)
    return int((moved & beyond).sum())


@pytest.mark.parametrize("case", [c for c in FC.displaced_cases() if c.catches], ids=lambda c: c.name)
def test_displaced_eye_leaves_the_picture(oracle, case):
    """at least 16 non-constant pixels of the displaced frame lie more than 3 pixels outside the bounding rectangle of the
    consistent camera's non-constant pixels: hulls and rectangles computed from the matrix (margins: 1.5 and 3 pixels) call them
    constant.  The axis case sits on the 128x80 frame: at 96x64 the same pose counts exactly 16, with nothing to spare."""
    assert FC.old_w_test(case.uniforms(oracle)), "the old test of clip w alone would not have let this case through"
    n = _outside_the_base_picture(oracle, case)
    assert n >= 16, (case, n)


def test_displaced_eye_inside_the_slack_stays_in_the_picture(oracle):
    case = FC.displaced_cases()[-1]
    assert case.culled and _outside_the_base_picture(oracle, case) == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_shim_builds_the_same_uniforms(volym_lib, oracle, case):
    """volym_camera_uniforms_from against vo_camera_uniforms_from on the same Camera struct"""
    from volym_amd import _lib
    cam = case.camera(oracle)
    mine = _lib.CCamera.from_buffer_copy(bytes(cam))
    u = _lib.CameraUniforms()
    assert volym_lib.volym_camera_uniforms_from(C.byref(mine), C.byref(u)) == 0
    assert bytes(u) == bytes(oracle.camera_uniforms(cam))


# ---- the consistency bound -----------------------------------------------------------------------------------------------------

# two float64 inversions of one f32 matrix differ in the last bits, and clip(eye) is a difference of terms of size |M| |eye| <= 1e3:
# 2^-52 * 1e3 / w_N (>= 0.002) * W / 2 (<= 1920) is 2e-7 pixels
ABS_NOISE = 1e-6

def _lib_displacement(volym_lib, u, W, H, w_min=0.0):
    from volym_amd import _lib
    out = C.c_double()
    rc = volym_lib.volym_view_eye_displacement(C.byref(_lib.CameraUniforms.from_buffer_copy(bytes(u))), W, H, w_min, C.byref(out))
    assert rc == 0
    return out.value


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bound_classifies_the_case(volym_lib, oracle, case):
    """The float64 restatement (free_camera_cases.eye_displacement) puts the case on the side of the slack that the list says, with
    room: a consistent f32 camera uses less than a tenth of the slack, a displaced one that must lose its culling is over it
    by a factor of two.  The library's figure is the restatement's."""
    u = case.uniforms(oracle)
    W, H = case.size
    d = FC.eye_displacement(u, W, H)
    if case.shift is None:
        assert d <= 0.1 * FC.SLACK_PIXELS, (case, d)
    elif case.culled:
        assert 0.1 * FC.SLACK_PIXELS < d <= 0.5 * FC.SLACK_PIXELS, (case, d)
    else:
        assert d >= 2.0 * FC.SLACK_PIXELS, (case, d)
    for w_min in (0.0, 1e-3, 0.05, 1.0):
        a, b = _lib_displacement(volym_lib, u, W, H, w_min), FC.eye_displacement(u, W, H, w_min)
        assert (math.isinf(a) and math.isinf(b)) or abs(a - b) <= 1e-6 * b + ABS_NOISE, (case, w_min, a, b)
    assert FC.eye_displacement(u, W, H, 1e-3) >= FC.eye_displacement(u, W, H, 0.05) >= d


def test_old_test_let_the_bug_through(oracle):
    """clip w alone: passes the two sideways moves and the small move along the axis, refuses only the large one"""
    got = [FC.old_w_test(c.uniforms(oracle)) for c in FC.displaced_cases()]
    assert got == [True, True, True, False, True]


SUITE_POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0), (35.0, 20.0, 0.5), (-120.0, -60.0, 2.0), (90.0, 89.0, 9.0), (40.0, 25.0, 3.0), (10.0, -70.0, 0.2),
               (40.0, 30.0, -1.0), (-150.0, -40.0, 0.5), (20.0, 10.0, 0.0), (133.0, 41.0, 0.6), (-58.0, -37.0, 0.9), (171.0, 12.0, 0.2), (725.0, -89.0, -3.0)]


@pytest.mark.parametrize("size", [(96, 64), (1920, 1080), (3840, 2160)], ids=lambda s: "%dx%d" % s)
def test_bound_accepts_the_orbit_cameras(volym_lib, oracle, size):
    """What f32 callers produce: the orbit poses the rest of the suite draws (distance 1 to 10) and the headline's, up to 3840x2160,
    are accepted, the box factor of the unit cube included (its corners' clip w is at least distance - 0.87).  An f32 eye at distance
    10 is rounded by up to 5e-7 per coordinate, which the near plane at w = 0.02 turns into 2.5e-5 of the frame: 0.1 pixels at 3840.
    The headline's eye, (0.5, 0.5, 1.5), is exact in f32 and uses a thousandth of the slack."""
    W, H = size
    worst = 0.0
    for pose in SUITE_POSES:
        u = oracle.benchmark_camera_uniforms(W / H, *pose)
        ivp = np.array([[u.inverse_view_proj[c][r] for c in range(4)] for r in range(4)], np.float64)
        M = np.linalg.inv(ivp)
        corners = np.array([[x, y, z, 1.0] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
        w_min = float((corners @ M.T)[:, 3].min())
        assert w_min > 0.1
        d = FC.eye_displacement(u, W, H, w_min)
        assert abs(_lib_displacement(volym_lib, u, W, H, w_min) - d) <= 1e-6 * d + ABS_NOISE
        worst = max(worst, d)
    print("largest displacement bound of an orbit camera at %dx%d: %.3g pixels" % (W, H, worst))
    assert worst <= FC.SLACK_PIXELS, worst
    head = oracle.benchmark_camera_uniforms(W / H)
    assert FC.eye_displacement(head, W, H, 0.5) <= 1e-3 * FC.SLACK_PIXELS


def test_bound_refuses_what_it_cannot_judge(volym_lib, oracle):
    from volym_amd import _lib
    u = _lib.CameraUniforms.from_buffer_copy(bytes(oracle.benchmark_camera_uniforms(1.5)))
    out = C.c_double()
    assert volym_lib.volym_view_eye_displacement(None, 8, 8, 0.0, C.byref(out)) == _lib.E_INVALID
    assert volym_lib.volym_view_eye_displacement(C.byref(u), 0, 8, 0.0, C.byref(out)) == _lib.E_INVALID
    bad = _lib.CameraUniforms.from_buffer_copy(bytes(u))
    for r in range(4):
        bad.inverse_view_proj[2][r] = 0.0                       # singular
    assert volym_lib.volym_view_eye_displacement(C.byref(bad), 8, 8, 0.0, C.byref(out)) == _lib.E_INVALID
    bad = _lib.CameraUniforms.from_buffer_copy(bytes(u))
    bad.inverse_view_proj[1][1] = float("nan")
    assert volym_lib.volym_view_eye_displacement(C.byref(bad), 8, 8, 0.0, C.byref(out)) == _lib.E_INVALID
    # an eye at the near plane's w or beyond: no bound
    far = _lib.CameraUniforms.from_buffer_copy(bytes(u))
    far.camera_position[2] = far.camera_position[2] - 0.05
    assert volym_lib.volym_view_eye_displacement(C.byref(far), 8, 8, 0.0, C.byref(out)) == 0 and math.isinf(out.value)
