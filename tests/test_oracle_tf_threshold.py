"""The transfer-function and threshold axes on the CPU: the C oracle against the independent NumPy restatement over a family
of transfer-function tables (1 to 256 texels, opaque, transparent, comb, step, baked) and over thresholds that are the float of
b/255 or one of its two neighbours, and a closed-form float64 known answer for the alpha of a constant cube that uses neither
oracle's arithmetic.  The GPU counterpart (test_gpu_tf_threshold.py) renders the same inputs against the C oracle, so what is
pinned here is that the reference side of that comparison is itself right on them."""
import ctypes
import math

import numpy as np
import pytest

from tests import common
from tests.test_oracle_crosscheck import _compare

# plain, smoothed, importance rendering with look-ahead 5, no opacity, importance colouring
MODES = {
    "plain": dict(),
    "smoothed": dict(use_gaussian_smoothing=1),
    "importance rendering": dict(use_importance_rendering=1, importance_check_ahead_steps=5),
    "no opacity": dict(use_opacity=0),
    "importance colouring": dict(use_importance_coloring=1),
}
BYTE_51 = float(np.float32(51) / np.float32(255))
TF_THRESHOLDS = [0.15, BYTE_51, float(np.nextafter(np.float32(BYTE_51), np.float32(1))), 0.0, -1.0, 1.0, 1.5]


@pytest.fixture(scope="module")
def bonsai32(oracle):
    raw, labels = common.bonsai(32)
    dims = (32, 32, 32)
    vol, imp = common.oracle_scene(oracle, raw, labels, common.BONSAI_SEGMENTS, dims)
    return dims, vol, imp


def test_tf_family_c_oracle_against_numpy(oracle, bonsai32):
    """Every table of the family under both filters and the five modes; each (table, filter, mode) takes two of the seven
    thresholds in rotation, so that every table meets every threshold and every mode: 13 x 2 x 5 x 2 = 260 renders a side."""
    from oracle import oracle_np
    dims, vol, imp = bonsai32
    W, H = 28, 20
    cam = oracle.benchmark_camera_uniforms(W / H, 25.0, 15.0, 0.0)
    cases = 0
    seen = set()
    for ti, (name, lut) in enumerate(common.tf_family(np.random.default_rng(5))):
        for filt in (0, 1):
            for mi, (mode, kw) in enumerate(MODES.items()):
                for j in range(2):
                    thr = TF_THRESHOLDS[(ti + 3 * mi + 2 * filt + 4 * j) % len(TF_THRESHOLDS)]
                    par = oracle.make_parameters(density_threshold=thr, raymarching_step_size=0.02, **kw)
                    a = oracle.render(vol, imp, dims, lut, cam, par, W, H, filter=filt, threads=2)
                    b = oracle_np.render(vol, imp, dims, lut, cam, par, W, H, filter=filt)
                    _compare(a, b, "tf %s filter %d %s thr %r" % (name, filt, mode, thr))
                    if name == "transparent" and kw.get("use_opacity", 1) == 1 and not kw.get("use_importance_coloring"):
                        hit = a[0][..., 3] != 1.0
                        assert not a[0][hit].any(), (mode, thr)        # alpha 0 texels: nothing accumulates, ever
                    seen.add((name, thr))
                    cases += 1
    assert cases == 13 * 2 * 5 * 2
    assert len(seen) == 13 * len(TF_THRESHOLDS)


TERRACE_DIMS = (24, 20, 28)
TERRACE_BYTES = (40, 51, 128, 255)


def test_terraced_thresholds_c_oracle_against_numpy(oracle):
    """Thresholds one float below, at and one float above b/255 on a volume of plateaus of byte b.  With the nearest filter the
    three differ only by whether byte b itself is dense; with the trilinear filter or the Gaussian smoothing an interpolated
    plateau value lands an ulp on either side of b/255, so the count of dense samples moves between the three neighbours -- which
    is asserted, or this would not test the edge it claims to."""
    from oracle import oracle_np
    vol = common.terraced_volume(TERRACE_DIMS, TERRACE_BYTES)
    imp = np.random.default_rng(8).integers(0, 256, vol.size).astype(np.uint8)
    lut = oracle.tf_default_lut()
    W, H = 30, 22
    thrs = common.byte_thresholds((51, 128))           # then 0, -1, 1, next(1), 1.5
    modes = (("nearest", 0, dict()), ("trilinear", 1, dict()), ("smoothed", 0, dict(use_gaussian_smoothing=1)))
    sharp = {}
    for pi, pose in enumerate(((25.0, 15.0, 0.0), (0.0, 0.0, 0.0))):
        cam = oracle.benchmark_camera_uniforms(W / H, *pose)
        for name, filt, kw in modes:
            if pi == 1 and name == "nearest":
                continue
            dense = []
            for thr in thrs:
                par = oracle.make_parameters(density_threshold=thr, raymarching_step_size=0.013, **kw)
                a = oracle.render(vol, imp, TERRACE_DIMS, lut, cam, par, W, H, filter=filt, threads=2)
                b = oracle_np.render(vol, imp, TERRACE_DIMS, lut, cam, par, W, H, filter=filt)
                _compare(a, b, "terraced pose %s %s thr %r" % (pose, name, thr))
                dense.append(a[2]["n_dense"])
                if thr > 1.0:
                    assert a[2]["n_dense"] == 0 and not a[0][a[0][..., 3] != 1.0].any(), (name, thr)
                if thr <= 0.0 and name != "smoothed":
                    assert a[2]["n_dense"] == a[2]["n_steps"], (name, thr)
            print("pose %s %-9s n_dense at prev/at/next(51/255): %s   (128/255): %s" % (pose, name, dense[0:3], dense[3:6]))
            # the edge proper: plateau samples that are dense one float below b/255 and not dense at b/255 itself
            sharp[(pi, name)] = (dense[0] != dense[1], dense[3] != dense[4])
            if name == "nearest":
                # a byte is dense at and below its own value: nothing changes one float below it, plateau b goes one float above
                assert dense[0] == dense[1] > dense[2] and dense[3] == dense[4] > dense[5], dense[0:6]
    # measured: trilinear sums of a plateau of 51 and Gaussian sums of a plateau of 128 fall below b/255, at both poses
    assert all(sharp[(pi, "trilinear")][0] for pi in (0, 1)), sharp
    assert all(sharp[(pi, "smoothed")][1] for pi in (0, 1)), sharp


# ---- closed form ------------------------------------------------------------------------------------------------------------

def _tf_256():
    """256 texels: byte 60 reads alpha 0 (texels 59..61), byte 200 reads between alpha 1/255 and 2/255 (so faint that the ray runs
    its whole chord), byte 255 reads texel 255 alone, alpha 1."""
    t = np.random.default_rng(21).integers(0, 256, (256, 4), dtype=np.uint8)
    t[:, 3] = np.arange(256) // 3 + 20
    t[59:62, 3] = 0
    t[200, 3], t[201, 3] = 1, 2
    t[254:, 3] = 255
    return t.ravel()


def _tf_7():
    """7 texels: byte 60 reads between texels 1 and 2, byte 200 between 4 and 5, byte 255 the last one, alpha 1"""
    t = np.random.default_rng(22).integers(0, 256, (7, 4), dtype=np.uint8)
    t[:, 3] = (0, 30, 90, 0, 12, 40, 255)
    return t.ravel()


def _alpha_lookup_f64(lut, b):
    """Linear / ClampToEdge lookup of the alpha channel at u = b/255 in float64 (x = u n - 0.5; wgsl:297-302)"""
    a = lut.reshape(-1, 4)[:, 3].astype(np.float64) / 255.0
    n = a.size
    x = b / 255.0 * n - 0.5
    i = math.floor(x)
    w = x - i
    return a[min(max(i, 0), n - 1)] * (1.0 - w) + a[min(max(i + 1, 0), n - 1)] * w


KAT_TOL = 4 * 8.85e-6


@pytest.mark.parametrize("step", [0.005, 0.02])
@pytest.mark.parametrize("b", [60, 200, 255])
@pytest.mark.parametrize("tf", ["256 texels", "7 texels"])
def test_closed_form_alpha_of_a_constant_cube(oracle, tf, b, step):
    """A constant, all-dense cube of byte b seen from the benchmark pose, centre pixel.  Every dense step adds
    alpha = 1 - (1 - A)^(25 step) with A the float64 lookup of the table at b/255, so after k steps the accumulated alpha is
    1 - (1 - alpha)^k; the ray stops at the first k that reaches 0.95 or at its step count.  k is the oracle's n_dense.  An
    A = 1 texel (byte 255, both tables) ends the ray on its first sample with alpha exactly 1; an A = 0 texel (byte 60, 256
    texels) leaves alpha exactly 0 over the whole chord.

    Tolerance: the largest distance of the C oracle from the closed form over the twelve cases, measured on the CPU, is 8.85e-6
    (256 texels, byte 200, step 0.005: the faint texel, 800 steps of alpha = 6.3e-4 each, where 1 - pow(...) in float32 loses
    four digits to cancellation; the next largest is 1.76e-6 for the same texel at step 0.02, and every case that exits early is
    within 1.5e-7).  The bar is four times that maximum, 3.54e-5, for float32 sums over k steps rounded another way; it is below
    the project's 1e-4."""
    lut = _tf_256() if tf == "256 texels" else _tf_7()
    n = 16
    vol = np.full(n ** 3, b, np.uint8)
    imp = np.zeros(n ** 3, np.uint8)
    cam = oracle.benchmark_camera_uniforms(1.0)
    par = oracle.make_parameters(raymarching_step_size=step)
    rgba = (ctypes.c_float * 4)()
    k = oracle.Counters()
    W = H = 64
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    oracle.lib().vo_render_pixel(u8(vol), u8(imp), n, n, n, 0, u8(lut), lut.size // 4, ctypes.byref(cam), ctypes.byref(par),
                                 W, H, W // 2, H // 2, rgba, ctypes.byref(k))
    # the chord's step count: path 1.0 in steps of 0.25 step, accumulated in float32 from t_entry = 0.5 (test_oracle_kat.py)
    t, chord, ds = np.float32(0.5), 0, np.float32(step) * np.float32(0.25)
    while t < np.float32(1.5):
        t = np.float32(t + ds)
        chord += 1
    A = _alpha_lookup_f64(lut, b)
    alpha = 1.0 - (1.0 - A) ** (25.0 * float(np.float32(step)))
    kk = k.n_dense
    assert k.n_steps == kk and 1 <= kk <= chord
    want = 1.0 - (1.0 - alpha) ** kk
    err = abs(float(rgba[3]) - want)
    print("tf %s byte %d step %g: A %.6f, k %d of %d, alpha %.9f, closed form %.9f, distance %.3g" % (tf, b, step, A, kk, chord, rgba[3], want, err))
    assert KAT_TOL <= 1e-4 and err <= KAT_TOL, (err, KAT_TOL)
    # k itself: the first count that reaches 0.95, or the chord
    if kk < chord:
        assert want >= 0.95 - KAT_TOL and 1.0 - (1.0 - alpha) ** (kk - 1) < 0.95 + KAT_TOL
    else:
        assert 1.0 - (1.0 - alpha) ** (kk - 1) < 0.95 + KAT_TOL
    if A == 1.0:
        assert kk == 1 and rgba[3] == 1.0
    if A == 0.0:
        assert kk == chord and rgba[3] == 0.0 and not any(rgba[:3])
    if (tf, b) == ("256 texels", 200):
        assert kk == chord and 0.0 < rgba[3] < 0.95         # faint: the whole chord, no early exit
