"""tests/pick_reference.py, the test-side restatement of the pick rule, pinned to the oracle without touching the oracle (no GPU).

  * its by-product frame and fetch counters equal oracle.render (the C oracle): f32 within 1e-6, rgba8 identical, counters identical;
  * in first-hit mode a ray is picked exactly where the oracle's pixel has alpha = 1 on a ray that hits the cube, and the shaded TF
    colour at eye + d * t of the record is the oracle's pixel;
  * closed forms on a constant-density cube;
  * the rays the GPU comparison may leave out (a composited sample within 1e-6 of alpha_min) are counted for every combination
    tests/test_gpu_pick.py compares: at most 0.1 % of the rays that hit the cube.
"""
import math

import numpy as np
import pytest

from tests import pick_reference as R
from tests.test_gpu_crop_box import PARAMS, _bonsai, _ragged, _table, _uniforms, CANOPY

W, H = 96, 64
POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0)]
ALPHA_MINS = (0.0, 0.3, 0.9)
# the six parameter sets of tests/test_gpu_crop_box.py plus trilinear: (name, parameters, filter)
CASES = [(k, v, 0) for k, v in PARAMS.items()] + [("trilinear", dict(), 1)]


def scenes():
    """name -> (dims, prepared density, prepared labels, label -> importance table)"""
    b, r = _bonsai(), _ragged()
    return {"bonsai64": (b[0], b[1], b[2], CANOPY), "ragged": (r[0], r[1], r[2], _table(l2=255))}


@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_frame_and_counters_equal_the_oracle(oracle, volym_lib, volume):
    dims, vol, labels, table = scenes()[volume]
    imp = table[labels]
    lut = oracle.tf_default_lut()
    for name, kw, filt in CASES:
        cam, par, _, _ = _uniforms(oracle, W, H, POSES[1], **kw)
        got = R.frame(vol, imp, dims, lut, cam, par, W, H, 0.3, filter=filt, labels=labels)
        ref_f32, ref_u8, ref_k = oracle.render(vol, imp, dims, lut, cam, par, W, H, filter=filt)
        err = float(np.abs(got["f32"].astype(np.float64) - ref_f32).max())
        print("%s, %s: max |f32 - oracle| = %.3g, picked %d of %d hit rays" % (volume, name, err, int((got["picks"]["status"] == 2).sum()), ref_k["n_hit"]))
        assert err <= 1e-6, (volume, name, err)
        assert np.array_equal(got["u8"], ref_u8), (volume, name)
        for k in ("n_vol", "n_imp", "n_steps", "n_dense", "n_hit"):
            assert got["counters"][k] == ref_k[k], (volume, name, k, got["counters"][k], ref_k[k])
        assert int(got["hit"].sum()) == ref_k["n_hit"]
        p = got["picks"]
        assert ((p["status"] == 0) == ~got["hit"]).all()
        none = p["status"] != 2
        for f in ("x", "y", "z", "label", "density"):
            assert not p[f][none].any()
        assert (p["t"][none] == -1.0).all() and (p["alpha8"][p["status"] == 0] == 255).all()
        assert (p["alpha8"][p["status"] == 1] == got["u8"][..., 3][p["status"] == 1]).all()     # status 1: the ray's final alpha


@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_first_hit_pick_is_the_oracles_pixel(oracle, volym_lib, volume):
    dims, vol, labels, table = scenes()[volume]
    imp = table[labels]
    lut = oracle.tf_default_lut()
    for pose in POSES:
        cam, par, _, _ = _uniforms(oracle, W, H, pose, **PARAMS["no opacity"])
        ref_f32, _, ref_k = oracle.render(vol, imp, dims, lut, cam, par, W, H)
        for a_min in ALPHA_MINS:                                # alpha becomes 1 at the first composited sample: the same pick for each
            got = R.frame(vol, imp, dims, lut, cam, par, W, H, a_min, labels=labels)
            p = got["picks"]
            want = got["hit"] & (ref_f32[..., 3] == 1.0)
            assert np.array_equal(p["status"] == 2, want), (volume, pose, a_min)
            assert want.sum() > 100
            sel = np.flatnonzero(want.ravel())
            rgb = R.shade_at(vol, dims, lut, cam, 0, got["eye"], got["d"][sel], p["t"].ravel()[sel])
            err = float(np.abs(rgb.astype(np.float64) - ref_f32.reshape(-1, 4)[sel, :3]).max())
            assert err <= 1e-6, (volume, pose, a_min, err)
            assert (p["alpha8"][want] == 255).all() and not got["near"].any()
            assert (p["density"][want] >= 39).all()             # a composited sample is dense: byte / 255 >= 0.15
            assert np.array_equal(p["label"][want], labels[(p["x"].astype(np.int64) + dims[0] * (p["y"].astype(np.int64) + dims[1] * p["z"].astype(np.int64)))[want]])


def test_closed_forms_on_a_constant_cube(oracle, volym_lib):
    """Every sample of a ray through a cube of one density byte b >= threshold is dense and composited, with the same opacity a:
    after k samples alpha = 1 - (1 - a)^k.  So the alpha_min = 0 pick is the ray's first sample, at t = t_entry, and the pick for
    alpha_min = A is composited sample number k = ceil(log(1 - A) / log(1 - a)), counted from 1, k - 1 minimum steps further on."""
    n, b, A = 32, 128, 0.6
    dims = (n, n, n)
    vol = np.full(n ** 3, b, np.uint8)
    imp = np.zeros(n ** 3, np.uint8)
    lut = oracle.tf_default_lut()
    cam, par, _, _ = _uniforms(oracle, W, H, POSES[0])
    assert tuple(np.round(list(cam.camera_position), 6)) == (0.5, 0.5, 1.5)       # the benchmark pose
    first = R.frame(vol, imp, dims, lut, cam, par, W, H, 0.0)
    hit = first["hit"]
    assert hit.sum() > 1000
    p0 = first["picks"]
    assert (p0["status"][hit] == 2).all() and (p0["status"][~hit] == 0).all()
    assert np.array_equal(p0["t"][hit].view(np.uint32), first["t_entry"][hit].view(np.uint32))
    assert (p0["density"][hit] == b).all() and (p0["has_labels"] == 0).all() and (p0["label"] == 0).all()
    # the per-sample opacity of byte b (wgsl:297-303, :314), in double precision: the margin below is what makes k unambiguous
    rho = b / 255.0
    x = rho * 256 - 0.5
    i0 = int(math.floor(x))
    tf_a = (float(lut.reshape(-1, 4)[i0, 3]) * (1 - (x - i0)) + float(lut.reshape(-1, 4)[i0 + 1, 3]) * (x - i0)) / 255.0
    min_step = 0.01 * 0.25
    a = 1.0 - (1.0 - tf_a) ** (min_step * 100.0)
    k = math.ceil(math.log(1.0 - A) / math.log(1.0 - a))
    assert k >= 3
    for j in (k - 1, k):
        assert abs((1.0 - a) ** j - (1.0 - A)) > 1e-3, (j, (1.0 - a) ** j)      # not within 1e-3 of the bar: f32 cannot move k
    got = R.frame(vol, imp, dims, lut, cam, par, W, H, A)
    p = got["picks"]
    t_k = first["t_entry"].copy()
    for _ in range(k - 1):
        t_k = (t_k + np.float32(par.raymarching_step_size) * np.float32(0.25)).astype(np.float32)
    long_enough = hit & (t_k < (first["t_entry"] + np.float32(0.9)))             # (every hit ray here crosses the whole cube)
    inside = hit & (p["status"] == 2)
    assert inside.sum() > 1000 and not got["near"].any()
    assert np.array_equal(p["t"][inside].view(np.uint32), t_k[inside].view(np.uint32))
    want8 = int(math.floor((1.0 - (1.0 - a) ** k) * 255.0 + 0.5))
    assert (np.abs(p["alpha8"][inside].astype(np.int32) - want8) <= 1).all()
    # a ray too short for k samples (it clips a corner of the cube) has status 1 and its final alpha
    short = hit & (p["status"] == 1)
    assert (p["alpha8"][short] < want8).all() and long_enough.sum() > 0


def test_rays_within_the_last_bit_of_alpha_min_are_rare(oracle, volym_lib):
    """The GPU comparison (tests/test_gpu_pick.py) leaves out a ray only when some composited sample of it has
    |alpha - alpha_min| <= 1e-6, and fails above 0.1 % of the hit rays of a frame: count them here for every combination it compares."""
    lut = oracle.tf_default_lut()
    worst = 0.0
    for volume, (dims, vol, labels, table) in scenes().items():
        imp = table[labels]
        for name, kw, filt in CASES:
            for pose in POSES:
                cam, par, _, _ = _uniforms(oracle, W, H, pose, **kw)
                for a_min in ALPHA_MINS:
                    got = R.frame(vol, imp, dims, lut, cam, par, W, H, a_min, filter=filt, labels=labels)
                    n_hit, n_near = int(got["hit"].sum()), int(got["near"].sum())
                    worst = max(worst, n_near / n_hit)
                    if n_near:
                        print("%s, %s, %s, alpha_min %.1f: %d of %d hit rays near" % (volume, name, pose, a_min, n_near, n_hit))
                    assert n_near <= 0.001 * n_hit, (volume, name, pose, a_min, n_near, n_hit)
                    assert (got["picks"]["status"] == 2).sum() > 50
    print("worst fraction of near rays: %.4f %%" % (100 * worst))
