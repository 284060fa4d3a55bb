"""The step-size and look-ahead axes on the CPU: raymarching_step_size from f32(1e-4) to 1 and importance_check_ahead_steps from 0
to 4096, the whole range volym_update accepts.  The C oracle against the independent NumPy restatement on every value of both
axes, the constant cube's alpha against its float64 closed form at every step, and -- for every frame that
tests/test_gpu_step_lookahead.py draws on the device -- that the oracle's work stays under the cap and that the frame shows
something a wrong step or count would change.  What is pinned here is the reference side of the GPU comparison."""
import ctypes

import numpy as np
import pytest

from tests import common
from tests import step_lookahead_cases as SC
from tests.test_oracle_crosscheck import _compare
from tests.test_oracle_tf_threshold import _alpha_lookup_f64, _tf_256, _tf_7

STEPS = common.step_axis()
COUNTS = common.ahead_axis()


def test_the_axes_are_what_they_claim():
    f = np.float32
    assert len(STEPS) == 8 and STEPS == sorted(STEPS) and all(float(f(s)) == s for s in STEPS)
    assert STEPS[0] == float(f(1e-4)) and f(STEPS[1]).view(np.uint32) == f(STEPS[0]).view(np.uint32) + 1
    assert STEPS[7] == 1.0 and f(STEPS[6]).view(np.uint32) + 1 == f(1.0).view(np.uint32)
    assert COUNTS == [0, 1, 2, 3, 25, 26, 63, 65, 255, 256, 1000, 4095, 4096]
    bad = common.refused_steps()
    assert len(bad) == 6 and bad[0] < STEPS[0] and f(bad[0]).view(np.uint32) + 1 == f(STEPS[0]).view(np.uint32)
    assert bad[1] > 1.0 and f(bad[1]).view(np.uint32) == f(1.0).view(np.uint32) + 1
    assert bad[2] == 0.0 and bad[3] < 0.0 and np.isnan(bad[4]) and bad[5] == float("inf")
    vol, imp = common.noise_scene(np.random.default_rng(1), (24, 20, 28))
    assert vol.dtype == imp.dtype == np.uint8 and vol.size == imp.size == 24 * 20 * 28
    assert set(np.unique(imp)) == {0, 255} and 0.22 < (imp == 255).mean() < 0.28 and len(np.unique(vol)) == 256


# ---- 1. the C oracle against the NumPy restatement -------------------------------------------------------------------------------

def _np_cases(i):
    """(scene, mode index, filter, pose index) of step i.  From 0.1 up: both scenes x four modes at 24x16.  Below, the
    restatement walks 4000 to 40 000 samples a ray in Python, up to 30 s a frame whatever its size (measured at 1e-4, 12x8: noise
    plain 2.1 s, smoothed 7.2 s, straight 7.1 s, cone 29 s; saturated 0.2, 0.5, 5.8 and 16 s), so there the cases are what fits in
    the time: at 0.001 everything but the cone, at 12x8 for the two finest steps plain and smoothed (the noise at 1e-4 only; the
    float above it draws the cube, whose rays end early), and at 1e-4 the straight look-ahead on the saturated cube.  The look-aheads do not read the step; they are restated at every count by
    test_ahead_axis_c_oracle_against_numpy."""
    if i == 0:
        return [("noise", 0, 0, 0), ("saturated", 0, 1, 1), ("saturated", 1, 0, 0), ("saturated", 2, 0, 0)]
    if i == 1:
        return [("saturated", 1, 1, 1), ("saturated", 0, 0, 0), ("saturated", 0, 1, 1)]
    out = [(name, mi, (mi + si + i) % 2, 1 if mi >= 2 else (mi + si) % 2) for si, name in enumerate(("noise", "saturated")) for mi in range(4)]
    return [c for c in out if i > 2 or c[1] != 3]


@pytest.mark.parametrize("i", range(len(STEPS)), ids=["step-1e-4", "step-next-1e-4"] + ["step-%g" % s for s in STEPS[2:6]] + ["step-prev-1", "step-1"])
def test_step_axis_c_oracle_against_numpy(oracle, i):
    """One step of the axis on the noise scene and on the saturated cube: plain, smoothed, importance straight and cone (6
    probes), nearest and linear in turn, both poses; 24x16, and 12x8 below the GUI's finest step (_np_cases)."""
    from oracle import oracle_np
    step = STEPS[i]
    W, H = SC.SMALL if step >= 0.001 - 1e-9 else (12, 8)
    lut = oracle.tf_default_lut()
    for name, mi, filt, pi in _np_cases(i):
        dims, vol, imp = SC.scene(name)
        mode, kw = SC.MODES[mi]
        par = dict(density_threshold=SC.threshold(name), raymarching_step_size=step)
        par.update(kw)
        par = oracle.make_parameters(**par)
        cam = oracle.benchmark_camera_uniforms(W / H, *SC.POSES[pi])
        a = oracle.render(vol, imp, dims, lut, cam, par, W, H, filter=filt, threads=2)
        b = oracle_np.render(vol, imp, dims, lut, cam, par, W, H, filter=filt)
        _compare(a, b, "step %r %s %s filter %d" % (step, name, mode, filt))
        assert a[2]["n_hit"] > 0 and a[2]["n_dense"] > 0


def _np_ahead_steps(count):
    """The restatement walks probes one Python iteration each, for every sample of the march: up to 3 probes at steps 0.05 and
    0.013, 25 to 65 at 0.05, 255 and 256 at 0.25, the thousands at 1 (four samples a ray; 4096 probes at 0.05 take two minutes)"""
    return (0.05, 0.013) if count <= 3 else (0.05,) if count <= 65 else (0.25,) if count <= 256 else (1.0,)


@pytest.mark.parametrize("count", COUNTS)
def test_ahead_axis_c_oracle_against_numpy(oracle, count):
    """One look-ahead count, straight and cone, on the noise scene (nearest; linear too up to 26) and on the saturated cube (up
    to 1000), at 24x16 and the steps of _np_ahead_steps."""
    from oracle import oracle_np
    W, H = SC.SMALL
    lut = oracle.tf_default_lut()
    cases = 0
    for cone in (0, 1):
        for si, (name, filt) in enumerate((("noise", 0), ("noise", 1), ("saturated", cone))):
            if (count > 26 and si == 1) or (count > 1000 and si == 2) or (count == 4095 and cone == 1):
                continue                # (4095, 4096: the noise alone, or they take 9 s each; the cone at 4096 and 1000)
            dims, vol, imp = SC.scene(name)
            for step in _np_ahead_steps(count)[:1 if si == 1 else 2]:
                par = oracle.make_parameters(density_threshold=SC.threshold(name), raymarching_step_size=step, use_importance_rendering=1,
                                             use_cone_importance_check=cone, importance_check_ahead_steps=count)
                cam = oracle.benchmark_camera_uniforms(W / H, *SC.POSES[(si + cone) % 2])
                a = oracle.render(vol, imp, dims, lut, cam, par, W, H, filter=filt, threads=2)
                b = oracle_np.render(vol, imp, dims, lut, cam, par, W, H, filter=filt)
                _compare(a, b, "count %d cone %d %s filter %d step %r" % (count, cone, name, filt, step))
                assert a[2]["n_dense"] > 0
                cases += 1
    assert cases == (10 if count <= 3 else 6 if count <= 26 else {1000: 4, 4095: 1, 4096: 2}.get(count, 4))


# ---- 2. closed form ----------------------------------------------------------------------------------------------------------------

_chords = {}


def _chord(step):
    """the chord's step count: path 1.0 in steps of 0.25 step, accumulated in float32 from t_entry = 0.5 (test_oracle_kat.py)"""
    if step not in _chords:
        t, n, ds = np.float32(0.5), 0, np.float32(step) * np.float32(0.25)
        while t < np.float32(1.5):
            t = np.float32(t + ds)
            n += 1
        _chords[step] = n
    return _chords[step]


# the largest distance of the C oracle from the float64 closed form seen at each step of the axis (18 cases a step); the bar is
# four times that, the ratio of test_oracle_tf_threshold.py (8.85e-6 observed, 3.54e-5 bar)
KAT_OBSERVED = [3.17e-4, 3.17e-4, 4.63e-5, 2.02e-6, 3.26e-6, 2.59e-6, 2.75e-6, 2.75e-6]


@pytest.mark.parametrize("step", STEPS, ids=["%.9g" % s for s in STEPS])
@pytest.mark.parametrize("b", [39, 45, 60, 128, 200, 255])
@pytest.mark.parametrize("tf", ["256 texels", "7 texels", "default"])
def test_closed_form_alpha_of_a_constant_cube_at_every_step(oracle, tf, b, step):
    """test_oracle_tf_threshold.py's closed form -- a constant 16^3 cube of byte b at the benchmark pose, centre pixel: k dense
    steps leave alpha = 1 - (1 - a)^k with a = 1 - (1 - A)^(25 step) and A the float64 lookup of the table -- at every step of
    the axis, three tables and six bytes.  At step 1 a ray has 4 samples; at 1e-4 it has 40 000, each adding as little as
    a = 1e-5.

    Bar, per step: four times the largest distance of the C oracle from the float64 value over the 18 cases of that step, measured
    on the CPU (KAT_OBSERVED).  Observed / bar: 1e-4 and its neighbour 3.17e-4 / 1.27e-3; 0.001 4.63e-5 / 1.85e-4; 0.1 2.02e-6 /
    8.1e-6; 0.25 3.26e-6 / 1.3e-5; 0.5 2.59e-6 / 1.04e-5; the float below 1 and 1 2.75e-6 / 1.1e-5.  The fine end is the faint
    texel of the 256-texel table (byte 200, A = 0.005): one step adds a = 1 - (1 - A)^0.0025 = 1.3e-5, which the shader's float32
    pow gives to 3 digits, the same way at each of the 39 994 steps -- this is the arithmetic the oracle restates, not a fault of
    its sums (which are within 1.8e-6 of float64 sums of the same terms) -- so at steps below 0.001 the alpha of a faint medium
    is further from the real-number model than the 1e-4 that separates the device from the oracle.  From 0.1 up the largest
    distance is the 7-texel table at byte 128 (A = 0.00065)."""
    lut = {"256 texels": _tf_256, "7 texels": _tf_7, "default": oracle.tf_default_lut}[tf]()
    n = 16
    vol = np.full(n ** 3, b, np.uint8)
    imp = np.zeros(n ** 3, np.uint8)
    cam = oracle.benchmark_camera_uniforms(1.0)
    par = oracle.make_parameters(raymarching_step_size=step, density_threshold=0.15)
    rgba = (ctypes.c_float * 4)()
    k = oracle.Counters()
    W = H = 64
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    oracle.lib().vo_render_pixel(u8(vol), u8(imp), n, n, n, 0, u8(lut), lut.size // 4, ctypes.byref(cam), ctypes.byref(par),
                                 W, H, W // 2, H // 2, rgba, ctypes.byref(k))
    A = _alpha_lookup_f64(lut, b)
    alpha = 1.0 - (1.0 - A) ** (25.0 * float(np.float32(step)))
    kk = k.n_dense
    chord = _chord(step)
    assert k.n_steps == kk and 1 <= kk <= chord
    want = 1.0 - (1.0 - alpha) ** kk
    err = abs(float(rgba[3]) - want)
    print("tf %s byte %d step %.9g: A %.6f, k %d of %d, alpha %.9f, closed form %.9f, distance %.3g" % (tf, b, step, A, kk, chord, rgba[3], want, err))
    KAT_TOL = 4 * KAT_OBSERVED[STEPS.index(step)]
    assert err <= KAT_TOL, (err, KAT_TOL)
    if kk < chord:
        assert want >= 0.95 - KAT_TOL and 1.0 - (1.0 - alpha) ** (kk - 1) < 0.95 + KAT_TOL
    else:
        assert 1.0 - (1.0 - alpha) ** (kk - 1) < 0.95 + KAT_TOL
    if A == 1.0:
        assert kk == 1 and rgba[3] == 1.0
    if A == 0.0:
        assert kk == chord and rgba[3] == 0.0 and not any(rgba[:3])


# ---- 3. the frames the device draws ------------------------------------------------------------------------------------------------

def _lit(f):
    return int((np.nan_to_num(f[..., :3]) != 0.0).any(axis=-1).sum())


def _with(case, **par):
    p = dict(case.par)
    p.update(par)
    return SC.Case(case.scene, case.size, case.pose, case.filt, **p)


def test_device_cases_stay_under_the_work_cap_and_show_something(oracle):
    """Every frame of the GPU file: n_vol + n_imp <= 2e7; on the noise and saturated scenes at least a quarter of the rays that
    meet the cube carry colour (the bonsai and the cup show less and are not what this relies on)."""
    cases = SC.device_cases()
    assert len(cases) > 400
    worst, dimmest = 0, 1.0
    for c in cases:
        f, u, k = SC.reference(oracle, c)
        work = k["n_vol"] + k["n_imp"]
        worst = max(worst, work)
        assert work <= SC.WORK_CAP, (c, work)
        assert k["n_hit"] > 0, c
        if c.scene == "boxed":
            assert _lit(f) >= 16, (c, _lit(f))       # (the importance modes at step 1 hide most of it; plain shows 72 and more)
        if c.scene in ("noise", "saturated"):
            frac = _lit(f) / k["n_hit"]
            dimmest = min(dimmest, frac)
            assert 4 * _lit(f) >= k["n_hit"], (c, _lit(f), k["n_hit"])
        if c.par["raymarching_step_size"] < 0.001 - 1e-9:
            assert c.par.get("importance_check_ahead_steps", 0) <= 25, c
        if c.par.get("importance_check_ahead_steps", 0) > 256:
            assert c.par["raymarching_step_size"] >= 0.05 and c.size == SC.SMALL, c
    print("%d cases; largest n_vol + n_imp %.3g; smallest lit fraction on noise / saturated %.3f" % (len(cases), worst, dimmest))


def test_boxed_noise_has_empty_steps_in_front_of_what_it_shows(oracle):
    """The boxed noise at steps 0.1 to 1, both poses, 48x32, pixel by pixel: every ray that carries colour took at least one sample
    that was not dense (its first one lies on a face of the cube that the content does not touch; after the content a ray at
    the benchmark pose leaves through the far face, which the content does touch), and at least 50 rays carry colour at every
    step: the empty steps the device replays in closed form at base / ulp(t) >= 2^22 lie in front of something to see."""
    dims, vol, imp = SC.scene("boxed")
    lut = oracle.tf_default_lut()
    W, H = SC.SIZES[0]
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    for step in STEPS[3:]:
        for pose in SC.POSES:
            case = SC.Case("boxed", (W, H), pose, 0, raymarching_step_size=step)
            cam, par = case.uniforms(oracle)
            f, _, _ = SC.reference(oracle, case)
            lit = np.argwhere((np.nan_to_num(f[..., :3]) != 0.0).any(axis=-1))
            assert len(lit) >= 50, (step, pose, len(lit))
            for y, x in lit:
                rgba = (ctypes.c_float * 4)()
                k = oracle.Counters()
                oracle.lib().vo_render_pixel(u8(vol), u8(imp), dims[0], dims[1], dims[2], 0, u8(lut), lut.size // 4, ctypes.byref(cam),
                                             ctypes.byref(par), W, H, int(x), int(y), rgba, ctypes.byref(k))
                assert k.n_dense >= 1 and k.n_steps > k.n_dense, (step, pose, x, y, k.n_steps, k.n_dense)
                if pose == SC.POSES[0]:
                    assert any(rgba[:3])


POINTS = [0, 2, 3, 4, 5, 7]          # the distinct points of the step axis: 1e-4 and 1 stand for their float neighbours too


def test_neighbouring_steps_give_different_frames(oracle):
    """Every frame of the GPU file on the noise and saturated scenes whose step is 1e-4, 0.001, 0.1, 0.25 or 0.5 differs in at
    least one float from the frame of the next point of the axis (0.001, 0.1, 0.25, 0.5, 1) with everything else the same: a
    frame drawn with a neighbouring step is not taken for the right one.  Measured exceptions, left out: the saturated cube from
    0.25 up (its first sample is opaque there: the noise scene tells those steps apart), and the pairs of float neighbours (1e-4 and the float
    above, 1 and the float below), whose frames coincide more often than not -- those two values are on the axis for
    volym_update's range check and for base / ulp(t) >= 2^22, not for their pictures."""
    n = 0
    for c in SC.device_cases():
        step = c.par["raymarching_step_size"]
        if c.scene not in ("noise", "saturated") or step not in STEPS or STEPS.index(step) not in POINTS[:-1]:
            continue
        i = POINTS.index(STEPS.index(step))
        if c.scene == "saturated" and i >= 3:
            continue
        nxt = _with(c, raymarching_step_size=STEPS[POINTS[i + 1]])
        a, b = SC.reference(oracle, c), SC.reference(oracle, nxt)
        assert not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (c, nxt)
        n += 1
    assert n > 150, n


def test_neighbouring_counts_give_different_frames(oracle):
    """Every frame of test_ahead_axis on the noise scene with a count of 0, 1, 2 or 3 differs in at least one float from the frame
    with the next count of the axis (1, 2, 3, 25).  Beyond 25 the probes lie so close together that frames may coincide: not
    compared.  (On the cup with one important voxel hardly any look-ahead finds it at any count; its frames are about the walks
    that find nothing.)"""
    n = 0
    for ci, count in enumerate(COUNTS[:4]):
        for cone in (0, 1):
            for c in SC.ahead_cases(count, cone):
                if c.scene != "noise":
                    continue
                nxt = _with(c, importance_check_ahead_steps=COUNTS[ci + 1])
                a, b = SC.reference(oracle, c), SC.reference(oracle, nxt)
                assert not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (c, nxt)
                n += 1
    assert n == 4 * 2 * 2
