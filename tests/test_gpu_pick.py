"""Pick on the device (volym_pick_pass / volym_read_picks / volym_pick): segment, texel and depth under a pixel.

The expected records come from tests/pick_reference.py, the test-side restatement of the rule (pinned to the oracle by
tests/test_pick_reference.py): status, x, y, z, label, density and has_labels equal, t bit-equal, alpha8 within 1.  A ray may be left
out of a comparison only when, in the restatement, some composited sample of it has |alpha - alpha_min| <= 1e-6; at most 0.1 % of
the rays that hit the cube in any compared frame, above which the comparison fails.
"""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import pick_reference as R
from tests.test_gpu_crop_box import PARAMS, CANOPY, _bonsai, _ragged, _table, _uniforms, _ctx

pytestmark = pytest.mark.gpu

W, H = 96, 64
POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0)]
ALPHA_MINS = (0.0, 0.3, 0.9)
CASES = [(k, v, 0) for k, v in PARAMS.items()] + [("trilinear", dict(), 1)]
EXACT = ("status", "x", "y", "z", "label", "density", "has_labels", "reserved")

_refs = {}


def _ref(key, *args, **kw):
    """the restatement's answer, marched once per combination (both layouts compare against the same records)"""
    if key not in _refs:
        _refs[key] = R.frame(*args, **kw)
    return _refs[key]


def _compare(what, got, ref):
    """got: records of the device, ref: a dict of pick_reference.frame, same shape"""
    want, near = ref["picks"], ref["near"]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    n_hit, n_near = int(ref["hit"].sum()), int(near.sum())
    assert n_near <= 0.001 * n_hit, (what, "rays within 1e-6 of alpha_min", n_near, n_hit)
    ok = ~near
    for f in EXACT:
        bad = (got[f] != want[f]) & ok
        assert not bad.any(), (what, f, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
    bad = (got["t"].view(np.uint32) != want["t"].view(np.uint32)) & ok
    assert not bad.any(), (what, "t", int(bad.sum()), got[bad][:4], want[bad][:4])
    d8 = np.abs(got["alpha8"].astype(np.int32) - want["alpha8"].astype(np.int32))
    assert d8[ok].max() <= 1, (what, "alpha8", int(d8[ok].max()))
    return n_hit, int((want["status"] == 2).sum()), n_near


def _pick_frame(ctx, a_min, rect=None):
    ctx.pick_pass(rect, a_min)
    return ctx.read_picks()


# ---- 1. whole small frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_whole_small_frames(oracle, volym_lib, volume, layout):
    """bonsai64: importances from labels through a table; ragged (97 x 80 x 71): uploaded importances, then labels.  Every
    parameter set, both poses, three values of alpha_min.  The first pick of a context runs before any frame, so without a distance
    field (a direct march); after the first frame the pick leaps through the slot's distance field: the same records."""
    from volym_amd import scene
    if volume == "bonsai64":
        dims, vol, labels = _bonsai()
        table = CANOPY
    else:
        dims, vol, labels = _ragged()
        table = _table(l2=255)
    imp = table[labels]
    lut = scene.default_lut()
    lut_o = oracle.tf_default_lut()
    total = picked = 0
    for filt in (0, 1):
        with _ctx(layout) as ctx:
            ctx.set_volume(vol, dims, filt)
            ctx.set_transfer_function(lut)
            if volume == "bonsai64":
                ctx.set_labels(labels, dims)
                ctx.set_segment_importances(table)
            else:
                ctx.set_importances(imp, dims)
                ctx.set_labels(labels, dims)
            assert ctx.pick_device_ptr() is None
            framed = False
            for name, kw, f in CASES:
                if f != filt:
                    continue
                for pose in POSES:
                    cam, par, cu, pu = _uniforms(oracle, W, H, pose, **kw)
                    ctx.update(cu, pu)
                    for a_min in ALPHA_MINS:
                        what = (volume, layout, name, pose, a_min)
                        ref = _ref((volume, name, pose, a_min), vol, imp, dims, lut_o, cam, par, W, H, a_min, filter=filt, labels=labels)
                        got = _pick_frame(ctx, a_min)
                        assert got.dtype.itemsize == 16 and got.shape == (H, W)
                        n_hit, n_picked, _ = _compare(what, got, ref)
                        total += n_hit
                        picked += n_picked
                        if not framed:
                            ctx.compute_pass()                  # builds the distance field of this threshold in stream order
                            framed = True
                            again = _pick_frame(ctx, a_min)
                            assert np.array_equal(again.view(np.uint8), got.view(np.uint8)), (what, "with and without the distance field")
                    assert ctx.pick_device_ptr()
    print("%s, layout %d: %d hit rays compared, %d picked" % (volume, layout, total, picked))
    assert picked > 5000


# ---- 2. the workflow ------------------------------------------------------------------------------------------------------------
def test_click_to_hide_workflow(oracle, volym_lib):
    from volym_amd import _lib, demo, scene
    raw, labels_raw = common.bonsai(64)
    dims = (64, 64, 64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    with demo.GpuContext(W, H, 0) as ctx, demo.GpuContext(W, H, 0) as twin:
        for c in (ctx, twin):
            c.set_option(_lib.OPT_WRITE_F32, 1)
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        t = demo.Simple.init(twin, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        first = d.pick(ctx, 0, 0)                                   # puts the labels on the device
        assert first["status"] in ("miss", "none") and first["label"] is None
        ctx.pick_pass(None, 0.5)
        recs = ctx.read_picks()
        assert (recs["has_labels"] == 1).all()
        canopy = np.argwhere((recs["status"] == 2) & (recs["label"] == 2))
        assert len(canopy) > 50, "the view must show the canopy"
        y, x = (int(v) for v in canopy[len(canopy) // 2])
        p = d.pick(ctx, x, y)
        assert p["status"] == "hit" and p["label"] == 2 and p["segment"] == "Canopy" and p["segment_id"] == "canopy"
        assert p["texel"] == (int(recs[y, x]["x"]), int(recs[y, x]["y"]), int(recs[y, x]["z"])) and p["t"] == float(recs[y, x]["t"])
        assert all(abs(c - (i + 0.5) / 64) < 1e-12 for c, i in zip(p["pos"], p["texel"]))
        hid = d.hide_at(ctx, x, y)
        assert hid["label"] == 2 and hid["hidden"] == [2]
        assert ctx.segment_visibility()[2] == 0
        after = d.pick(ctx, x, y)
        assert after["label"] != 2, after                           # another segment behind it, or nothing
        ctx.pick_pass(None, 0.5)
        assert not (ctx.read_picks()["label"] == 2).any()
        d.compute_pass(ctx)
        ctx.sync()
        t.set_hidden(twin, [2])
        t.compute_pass(twin)
        twin.sync()
        assert np.array_equal(ctx.read_rgba8(), twin.read_rgba8())
        assert np.array_equal(ctx.read_rgba32f().view(np.uint32), twin.read_rgba32f().view(np.uint32))
        # a second click adds to the hidden set; a click on the background changes nothing
        d.set_hidden(ctx, [])
        lo, hi = d.set_crop(ctx, (0.1, 0.1, 0.0), (0.8, 1.0, 0.625))
        for a_min in (0.0, 0.5):
            ctx.pick_pass(None, a_min)
            r = ctx.read_picks()
            hit = r["status"] == 2
            assert hit.sum() > 100
            for f, a in (("x", 0), ("y", 1), ("z", 2)):
                assert (r[f][hit] >= lo[a]).all() and (r[f][hit] < hi[a]).all(), (f, lo, hi)
        assert d.hide_at(ctx, 0, 0)["hidden"] == []


# ---- 3. rects -------------------------------------------------------------------------------------------------------------------
def test_rects(oracle, volym_lib):
    from volym_amd import _lib, scene
    w, h = 107, 75                                                   # not multiples of 16
    dims, vol, labels = _bonsai()
    cam, par, cu, pu = _uniforms(oracle, w, h, (35.0, 20.0, 0.0))
    with _ctx(0, w=w, h=h) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(labels, dims)
        ctx.set_segment_importances(CANOPY)
        ctx.update(cu, pu)
        ctx.compute_pass()
        ctx.pick_pass((40, 30, 1, 1), 0.3)                            # a small buffer first: the later passes grow it
        one = ctx.read_picks()
        whole = _pick_frame(ctx, 0.3).copy()
        assert whole.shape == (h, w) and (whole["status"] == 2).sum() > 300
        ref = R.frame(vol, CANOPY[labels], dims, oracle.tf_default_lut(), cam, par, w, h, 0.3, labels=labels)
        _compare("107 x 75", whole, ref)
        assert one.shape == (1, 1) and one[0, 0] == whole[30, 40]
        for rect in ((0, 0, 16, 16), (3, 5, 21, 13), (37, 22, 50, 41), (w - 19, h - 11, 19, 11), (w - 1, h - 1, 1, 1), (0, 33, w, 1), (61, 0, 1, h),
                     (16, 16, 32, 32), (0, 0, w, h)):
            x0, y0, rw, rh = rect
            got = _pick_frame(ctx, 0.3, rect)
            assert got.shape == (rh, rw)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(whole[y0:y0 + rh, x0:x0 + rw]).view(np.uint8)), rect
        for x, y in ((0, 0), (40, 30), (w - 1, h - 1), (53, 37), (106, 0), (0, 74)):
            assert ctx.pick(x, y, 0.3) == whole[y, x], (x, y)
        # the one-pixel call at the C boundary
        rec = _lib.Pick()
        assert _lib.lib().volym_pick(ctx.handle, 53, 37, C.c_float(0.3), C.byref(rec)) == _lib.OK
        assert np.frombuffer(bytes(rec), _lib.PICK_DTYPE)[0] == whole[37, 53]


# ---- 4. it disturbs nothing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 2], ids=["one slot", "two in flight"])
def test_a_pick_pass_changes_no_frame(oracle, volym_lib, slots):
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    views = [_uniforms(oracle, W, H, pose, **PARAMS[name]) for pose, name in (((0.0, 0.0, 0.0), "base"), ((35.0, 20.0, 0.0), "straight"), ((35.0, 20.0, 0.0), "base"))]

    def run(with_picks):
        frames = []
        with _ctx(-1, [(_lib.OPT_FRAMES_IN_FLIGHT, slots)]) as ctx:
            ctx.set_volume(vol, dims, 0)
            ctx.set_importances(imp, dims)
            ctx.set_transfer_function(scene.default_lut())
            for cam, par, cu, pu in views:
                ctx.update(cu, pu)
                for _ in range(3):
                    ctx.compute_pass()
                ctx.settle()                                         # kernel 2 on its final list for the view
                for k in range(4):
                    ctx.compute_pass()
                    if with_picks:
                        ctx.pick_pass(None, 0.3 if k % 2 else 0.0)   # enqueued between two frames, no sync
                        if k == 1:
                            ctx.pick_pass((5, 7, 33, 21), 0.9)
                    ctx.compute_pass()
                    ctx.sync()
                    frames.append((ctx.read_rgba8(), ctx.read_rgba32f()))
                    if with_picks:
                        r = ctx.read_picks()                         # of the latest pass: the rect when k == 1, else the frame
                        assert r.shape == ((21, 33) if k == 1 else (H, W))
                        if k != 1:
                            assert (r["status"] == 2).any()
        return frames

    plain, picked = run(False), run(True)
    assert len(plain) == len(picked) == 12
    for i, ((a8, a32), (b8, b32)) in enumerate(zip(plain, picked)):
        assert np.array_equal(a8, b8), (slots, i)
        assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32)), (slots, i)
    assert plain[0][0][..., :3].any()


# ---- 5. without labels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_without_labels(oracle, volym_lib, layout):
    from volym_amd import scene
    dims, vol, labels = _ragged()
    imp = _table(l2=255)[labels]
    lut_o = oracle.tf_default_lut()
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_importances(imp, dims)
        ctx.set_transfer_function(scene.default_lut())
        for stage in ("never had labels", "labels dropped by set_importances", "labels of another size"):
            if stage == "labels dropped by set_importances":
                ctx.set_labels(labels, dims)
                cam, par, cu, pu = _uniforms(oracle, W, H, POSES[1])
                ctx.update(cu, pu)
                assert (_pick_frame(ctx, 0.0)["has_labels"] == 1).all()
                ctx.set_importances(imp, dims)
            elif stage == "labels of another size":
                ctx.set_labels(np.full(8 * 8 * 8, 7, np.uint8), (8, 8, 8))      # do not fit the volume: count as absent
            for name in ("base", "straight", "no opacity"):
                cam, par, cu, pu = _uniforms(oracle, W, H, POSES[1], **PARAMS[name])
                ctx.update(cu, pu)
                for a_min in ALPHA_MINS:
                    ref = _ref(("ragged, no labels", name, a_min), vol, imp, dims, lut_o, cam, par, W, H, a_min)
                    got = _pick_frame(ctx, a_min)
                    assert (got["has_labels"] == 0).all() and (got["label"] == 0).all(), stage
                    _compare((layout, stage, name, a_min), got, ref)


def test_labels_in_another_layout_than_the_volume(oracle, volym_lib):
    """VOLYM_OPT_VOLUME_LAYOUT changed between the uploads: the one label fetch of a ray takes the labels' own layout."""
    from volym_amd import _lib, scene
    dims, vol, labels = _ragged()
    imp = _table(l2=255)[labels]
    cam, par, cu, pu = _uniforms(oracle, W, H, POSES[1])
    ref = R.frame(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H, 0.3, labels=labels)
    for vol_layout, lab_layout in ((0, 1), (1, 0)):
        with _ctx(vol_layout) as ctx:
            ctx.set_volume(vol, dims, 0)
            ctx.set_importances(imp, dims)
            ctx.set_transfer_function(scene.default_lut())
            ctx.set_option(_lib.OPT_VOLUME_LAYOUT, lab_layout)
            ctx.set_labels(labels, dims)
            ctx.update(cu, pu)
            _compare((vol_layout, lab_layout), _pick_frame(ctx, 0.3), ref)


# ---- 6. sizes that matter -------------------------------------------------------------------------------------------------------
def test_bonsai256_at_1080p(oracle, volym_lib):
    from volym_amd import demo, scene
    n, w, h = 256, 1920, 1080
    dims, vol, labels = _bonsai(n)
    imp = CANOPY[labels]
    rows = list(range(3, h, 16))                                      # 68 rows
    assert len(rows) == 68
    with demo.GpuContext(w, h, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(labels, dims)
        ctx.set_segment_importances(CANOPY)
        for name, a_min in (("base", 0.5), ("straight", 0.0)):
            cam, par, cu, pu = _uniforms(oracle, w, h, **PARAMS[name])
            ctx.update(cu, pu)
            for _ in range(3):
                ctx.compute_pass()
            ctx.settle()
            ref = R.frame(vol, imp, dims, oracle.tf_default_lut(), cam, par, w, h, a_min, labels=labels, rows=rows)
            got = _pick_frame(ctx, a_min)
            n_hit, n_picked, n_near = _compare((n, w, h, name, a_min), got[rows], ref)
            print("256^3 at 1920x1080, %s, alpha_min %.1f: %d hit rays in 68 rows, %d picked, %d left out" % (name, a_min, n_hit, n_picked, n_near))
            assert n_picked > 5000
    common._cache.pop(("bonsai", n), None)


def test_1024cube_labels_at_4k(oracle, volym_lib):
    """synth_bonsai(1024) + labels on the auto-bricked layout at 3840 x 2160, straight look-ahead 15."""
    from volym_amd import demo, scene
    n, w, h = 1024, 3840, 2160
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol = scene.prepare_volume(raw, dims, True)
    labels = scene.prepare_volume(labels_raw, dims, True)
    del raw, labels_raw
    common._cache.pop(("bonsai", n), None)
    imp = CANOPY[labels]
    rows = list(range(3, h, 32))                                      # 68 rows
    assert len(rows) == 68
    cam, par, cu, pu = _uniforms(oracle, w, h, **PARAMS["straight"])
    a_min = 0.5
    with demo.GpuContext(w, h, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(labels, dims)
        ctx.set_segment_importances(CANOPY)
        ctx.update(cu, pu)
        ctx.compute_pass()
        got = _pick_frame(ctx, a_min)[rows]
    ref = R.frame(vol, imp, dims, oracle.tf_default_lut(), cam, par, w, h, a_min, labels=labels, rows=rows)
    n_hit, n_picked, n_near = _compare((n, w, h, a_min), got, ref)
    print("1024^3 at 3840x2160, straight 15, alpha_min %.1f: %d hit rays in 68 rows, %d picked, %d left out" % (a_min, n_hit, n_picked, n_near))
    assert n_picked > 10000                                        # (the restatement picks 15365 rays of these rows)


# ---- 7. refusals leave the context usable ---------------------------------------------------------------------------------------
def test_refusals_leave_the_context_rendering(oracle, volym_lib):
    from volym_amd import _lib, scene
    L = _lib.lib()
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    cam, par, cu, pu = _uniforms(oracle, W, H, POSES[1])
    rec = _lib.Pick()

    def code(call):
        with pytest.raises(_lib.VolymError) as e:
            call()
        return e.value.code

    with _ctx(-1) as c:
        assert code(lambda: c.pick_pass(None, 0.0)) == _lib.E_STATE                   # no volume
        assert code(c.read_picks) == _lib.E_STATE                                     # no pass yet
        assert c.pick_device_ptr() is None
        c.set_volume(vol, dims, 0)
        c.set_importances(imp, dims)
        assert code(lambda: c.pick_pass(None, 0.0)) == _lib.E_STATE                   # no transfer function
        c.set_transfer_function(scene.default_lut())
        assert code(lambda: c.pick_pass(None, 0.0)) == _lib.E_STATE                   # no volym_update
        assert code(lambda: c.pick(1, 1)) == _lib.E_STATE
        c.update(cu, pu)
        assert code(c.read_picks) == _lib.E_STATE                                     # still no pass
        for rect in ((W, 0, 1, 1), (0, H, 1, 1), (0, 0, W + 1, 1), (1, 0, W, 1), (0, 1, 1, H), (2 ** 32 - 1, 0, 2, 1), (0, 0, 2 ** 32 - 1, 2 ** 32 - 1),
                     (5, 5, 0, 3), (5, 5, 3, 0), (0, 0, 0, 0)):
            assert code(lambda: c.pick_pass(rect, 0.0)) == _lib.E_INVALID, rect
        for a_min in (float("nan"), -0.01, 0.951, 1.0, float("inf"), -float("inf")):
            assert code(lambda: c.pick_pass(None, a_min)) == _lib.E_INVALID, a_min
            assert code(lambda: c.pick(3, 3, a_min)) == _lib.E_INVALID, a_min
        assert code(lambda: c.pick(W, 0)) == _lib.E_INVALID
        assert L.volym_pick_pass(None, None, C.c_float(0.0)) == _lib.E_INVALID
        assert L.volym_read_picks(None, C.byref(rec)) == _lib.E_INVALID
        assert L.volym_read_picks(c.handle, None) == _lib.E_INVALID
        assert L.volym_pick(c.handle, 1, 1, C.c_float(0.0), None) == _lib.E_INVALID
        assert L.volym_pick(None, 1, 1, C.c_float(0.0), C.byref(rec)) == _lib.E_INVALID
        assert L.volym_pick_device_ptr(None) is None
        assert code(c.read_picks) == _lib.E_STATE                                     # none of the refused calls was a pass
        c.compute_pass()
        c.sync()
        ref = oracle.render(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H)
        err, over, du8, _ = common.compare_images(c.read_rgba32f(), c.read_rgba8(), ref[0], ref[1], 1e-4)
        assert over == 0 and du8 <= 1, (err, over, du8)
        got = _pick_frame(c, 0.95)                                                    # the largest valid alpha_min
        _compare("after the refusals", got, R.frame(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H, 0.95))
        assert _pick_frame(c, 0.0, (W - 1, H - 1, 1, 1)).shape == (1, 1)
