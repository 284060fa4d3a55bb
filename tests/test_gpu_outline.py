"""The outline pass on the device (volym_outline_pass / volym_read_outline / volym_outline_device_ptr).

The expected image is scene.outline_frame, the host twin of the rule (pinned to a brute-force double loop by
tests/test_outline_host.py), of the frame read before the pass and the records the pass was given.  Every comparison is over every
pixel and bit-exact: the rule is integer, so there is no tolerance and no pixel is left out.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests.test_gpu_crop_box import CANOPY, _bonsai, _uniforms, _ctx

pytestmark = pytest.mark.gpu

POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0)]
RING, FILL = (255, 200, 10, 180), (20, 40, 250, 77)
RADII = (1, 2, 8)


def _scene(ctx, pose=POSES[1], oracle=None, w=None, h=None, dims_vol_labels=None):
    """synth_bonsai(64) with labels and the canopy important, as tests/test_gpu_pick.py sets it up; one update"""
    from volym_amd import scene
    dims, vol, labels = dims_vol_labels or _bonsai()
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut())
    ctx.set_labels(labels, dims)
    ctx.set_segment_importances(CANOPY)
    cam, par, cu, pu = _uniforms(oracle, w or ctx.width, h or ctx.height, pose)
    ctx.update(cu, pu)


def _records(status, label, rng=None):
    """(h, w) records from status and label planes; the other fields random (the pass must not read them) or zero"""
    from volym_amd import _lib
    h, w = status.shape
    p = np.zeros((h, w), _lib.PICK_DTYPE)
    p["status"], p["label"] = status, label
    if rng is not None:
        p["t"] = rng.random((h, w))
        p["x"], p["y"], p["z"] = (rng.integers(0, 60000, (h, w)) for _ in range(3))
        for f in ("density", "alpha8", "has_labels", "reserved"):
            p[f] = rng.integers(0, 256, (h, w))
    return p


def _to_device(picks):
    return torch.from_numpy(np.ascontiguousarray(picks).view(np.uint8).reshape(-1).copy()).cuda()


def _same(what, got, want):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


def _three_targets(ctx, what, picks, rect, selected, ring, fill, radius):
    """one case through the own target, a caller's tensor and the frame buffer itself"""
    from volym_amd import scene
    W, H = ctx.width, ctx.height
    dev = _to_device(picks)
    frame = ctx.read_rgba8()
    want = scene.outline_frame(frame, picks, rect, selected, ring, fill, radius)
    # the context's own target
    ctx.outline_pass(selected, ring, fill, radius, records_ptr=dev.data_ptr(), rect=rect)
    _same((what, "own target"), ctx.read_outline(), want)
    assert ctx.outline_device_ptr()
    _same((what, "own target: the frame is untouched"), ctx.read_rgba8(), frame)
    # a caller's tensor
    target = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.outline_pass(selected, ring, fill, radius, records_ptr=dev.data_ptr(), rect=rect, target_ptr=target.data_ptr())
    ctx.sync()
    _same((what, "caller's tensor"), target.cpu().numpy().reshape(H, W, 4), want)
    _same((what, "caller's tensor: the frame is untouched"), ctx.read_rgba8(), frame)
    assert np.array_equal(dev.cpu().numpy(), np.ascontiguousarray(picks).view(np.uint8).reshape(-1)), (what, "the records changed")
    # in place: the frame buffer is the target, and then holds the annotated image
    ctx.outline_pass(selected, ring, fill, radius, records_ptr=dev.data_ptr(), rect=rect, target_ptr=ctx.frame_device_ptr())
    _same((what, "in place"), ctx.read_rgba8(), want)
    ctx.compute_pass()                                       # the standing view's frame again
    _same((what, "the frame after the next compute pass"), ctx.read_rgba8(), frame)
    return want, frame


# ---- 1. synthetic records -------------------------------------------------------------------------------------------------------
def test_synthetic_records(oracle, volym_lib):
    """200 x 72: three full mask words and one of 8 bits; 72 rows are 9 strips of the blend kernel and 4.5 blocks of the pack kernel"""
    from volym_amd import scene
    W, H = 200, 72
    rng = np.random.default_rng(11)
    whole = (0, 0, W, H)
    sel3 = scene.selection_mask([3])
    n = 0
    with _ctx(0, w=W, h=H) as ctx:
        _scene(ctx, oracle=oracle)
        ctx.compute_pass()
        assert ctx.outline_device_ptr() is None
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        # a single selected pixel
        for x, y in ((0, 0), (199, 71), (199, 0), (63, 10), (64, 10), (127, 35), (128, 35)):
            for radius in RADII:
                status, label = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
                status[y, x], label[y, x] = 2, 3
                want, before = _three_targets(ctx, ("one pixel", x, y, radius), _records(status, label), whole, sel3, RING, FILL, radius)
                changed = (want != before).any(axis=-1)
                yy, xx = np.mgrid[0:H, 0:W]
                assert not changed[(np.abs(xx - x) > radius) | (np.abs(yy - y) > radius)].any()
                n += 1
        # random masks with random statuses and labels, a random subset of the labels selected
        for density in (0.005, 0.3):
            for radius in RADII:
                picked = rng.random((H, W)) < density
                status = np.where(picked, 2, rng.integers(0, 2, (H, W))).astype(np.uint8)
                label = rng.integers(0, 256, (H, W)).astype(np.uint8)
                selected = (rng.random(256) < 0.5).astype(np.uint8)
                want, before = _three_targets(ctx, ("random", density, radius), _records(status, label, rng), whole, selected, RING, FILL, radius)
                assert (want != before).any()
                n += 1
        # records that cover a rect only
        for rect in ((37, 5, 101, 40), (64, 0, 64, 72)):
            for radius in RADII:
                h, w = rect[3], rect[2]
                status = np.where(rng.random((h, w)) < 0.1, 2, rng.integers(0, 2, (h, w))).astype(np.uint8)
                status[0, 0] = status[h - 1, w - 1] = status[0, w - 1] = 2          # the rect's corners: their rings lie outside it
                label = rng.integers(0, 6, (h, w)).astype(np.uint8)
                label[0, 0] = label[h - 1, w - 1] = label[0, w - 1] = 3
                want, before = _three_targets(ctx, ("rect", rect, radius), _records(status, label, rng), rect, scene.selection_mask([1, 3]), RING, FILL, radius)
                if rect[0] > 0:
                    assert (want[rect[1], rect[0] - 1] != before[rect[1], rect[0] - 1]).any(), "a ring pixel outside the rect"
                n += 1
        # nothing selected: the frame; everything selected and picked: the fill everywhere
        full = _records(np.full((H, W), 2, np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8), rng)
        for radius in RADII:
            want, before = _three_targets(ctx, ("nothing selected", radius), full, whole, np.zeros(256, np.uint8), RING, FILL, radius)
            assert np.array_equal(want, before)
            want, before = _three_targets(ctx, ("everything selected", radius), full, whole, np.ones(256, np.uint8), RING, FILL, radius)
            assert np.array_equal(want, scene.outline_blend(before, FILL))
            n += 2
        # statuses 0 and 1 with a selected label select nothing
        for status in (0, 1):
            want, before = _three_targets(ctx, ("status", status), _records(np.full((H, W), status, np.uint8), np.full((H, W), 3, np.uint8)), whole, sel3,
                                          RING, FILL, 2)
            assert np.array_equal(want, before)
            n += 1
    assert n == 21 + 6 + 6 + 6 + 2


def test_the_own_target_keeps_its_image_while_a_pass_goes_to_a_callers(oracle, volym_lib):
    """64 x 48: a pass into the context's own target, one into a caller's tensor -- read_outline still returns the first -- and one into
    the own target again"""
    from volym_amd import scene
    W, H = 64, 48
    rng = np.random.default_rng(5)
    whole = (0, 0, W, H)
    sel = scene.selection_mask([1, 3])

    def records():
        status = np.where(rng.random((H, W)) < 0.1, 2, rng.integers(0, 2, (H, W))).astype(np.uint8)
        return _records(status, rng.integers(0, 6, (H, W)).astype(np.uint8), rng)

    with _ctx(0, w=W, h=H) as ctx:
        _scene(ctx, oracle=oracle)
        ctx.compute_pass()
        frame = ctx.read_rgba8()
        first, second, third = records(), records(), records()
        want = [scene.outline_frame(frame, p, whole, sel, RING, FILL, 2) for p in (first, second, third)]
        assert (want[0] != want[1]).any() and (want[0] != want[2]).any() and (want[0] != frame).any()
        dev = [_to_device(p) for p in (first, second, third)]
        assert ctx.outline_device_ptr() is None
        ctx.outline_pass(sel, RING, FILL, 2, records_ptr=dev[0].data_ptr(), rect=whole)
        _same("own target", ctx.read_outline(), want[0])
        own = ctx.outline_device_ptr()
        assert own
        target = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.outline_pass(sel, RING, FILL, 2, records_ptr=dev[1].data_ptr(), rect=whole, target_ptr=target.data_ptr())
        ctx.sync()
        _same("caller's tensor", target.cpu().numpy().reshape(H, W, 4), want[1])
        _same("own target after a pass into a caller's", ctx.read_outline(), want[0])
        ctx.outline_pass(sel, RING, FILL, 2, records_ptr=dev[2].data_ptr(), rect=whole)
        _same("own target again", ctx.read_outline(), want[2])
        assert ctx.outline_device_ptr() == own
        _same("the frame is untouched", ctx.read_rgba8(), frame)


# ---- 2. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_end_to_end(oracle, volym_lib, layout):
    from volym_amd import scene
    W, H = 96, 64
    canopy = scene.selection_mask([2])
    with _ctx(layout, w=W, h=H) as ctx:
        for pose in POSES:
            _scene(ctx, pose, oracle)
            for stage in ("whole frame", "rect", "another segment hidden"):
                rect = None
                if stage == "rect":
                    rect = (10, 6, 50, 40)
                if stage == "another segment hidden":
                    ctx.set_segment_visibility(scene.visibility_mask([4]))
                ctx.compute_pass()
                ctx.pick_pass(rect, 0.3)
                ctx.outline_pass(canopy, RING, FILL, 2)              # enqueued behind both, no sync
                got = ctx.read_outline()
                frame, picks = ctx.read_rgba8(), ctx.read_picks()
                assert picks.shape == ((40, 50) if rect else (H, W))
                n_canopy = int(((picks["status"] == 2) & (picks["label"] == 2)).sum())
                assert n_canopy > 50, (pose, stage, n_canopy)
                want = scene.outline_frame(frame, picks, rect or (0, 0, W, H), canopy, RING, FILL, 2)
                _same((layout, pose, stage), got, want)
                assert (want != frame).any()
            ctx.set_segment_visibility(np.ones(256, np.uint8))


def test_two_frames_in_flight(oracle, volym_lib):
    """four alternating frames of two views, an outline after each, nothing but enqueues in between: each outline shows its own
    frame and its own pick pass"""
    from volym_amd import _lib, scene
    W, H = 96, 64
    canopy = scene.selection_mask([2])
    with _ctx(-1, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)], w=W, h=H) as ctx:
        _scene(ctx, POSES[0], oracle)
        views, want = [], []
        for pose in POSES:
            cam, par, cu, pu = _uniforms(oracle, W, H, pose)
            views.append((cu, pu))
            ctx.update(cu, pu)
            ctx.compute_pass()
            ctx.pick_pass(None, 0.3)
            frame, picks = ctx.read_rgba8(), ctx.read_picks()
            want.append((frame, scene.outline_frame(frame, picks, (0, 0, W, H), canopy, RING, FILL, 2)))
        assert (want[0][1] != want[1][1]).any() and all((o != f).any() for f, o in want)
        # own target, read after each frame
        for i in range(4):
            ctx.update(*views[i % 2])
            ctx.compute_pass()
            ctx.pick_pass(None, 0.3)
            ctx.outline_pass(canopy, RING, FILL, 2)
            _same(("own target, frame", i), ctx.read_outline(), want[i % 2][1])
            _same(("the frame itself, frame", i), ctx.read_rgba8(), want[i % 2][0])
        # a target per frame, no host wait until all four are enqueued
        targets = [torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        for i in range(4):
            ctx.update(*views[i % 2])
            ctx.compute_pass()
            ctx.pick_pass(None, 0.3)
            ctx.outline_pass(canopy, RING, FILL, 2, target_ptr=targets[i].data_ptr())
        ctx.sync()
        for i in range(4):
            _same(("a target per frame, frame", i), targets[i].cpu().numpy().reshape(H, W, 4), want[i % 2][1])
        # in place with two slots: the annotated frame, then the next frame of that slot is the plain one again
        for i in range(4):
            ctx.update(*views[i % 2])
            ctx.compute_pass()
            ctx.pick_pass(None, 0.3)
            ctx.outline_pass(canopy, RING, FILL, 2, target_ptr=ctx.frame_device_ptr())
            _same(("in place, frame", i), ctx.read_rgba8(), want[i % 2][1])


def test_highlight_at_outlines_the_canopy(oracle, volym_lib):
    from volym_amd import demo, scene
    W, H = 96, 64
    raw, labels_raw = common.bonsai(64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    with demo.GpuContext(W, H, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=(64, 64, 64))
        d.compute_pass(ctx)
        d.set_labels(ctx, labels_raw)
        ctx.pick_pass(None, 0.5)
        recs = ctx.read_picks()
        canopy = np.argwhere((recs["status"] == 2) & (recs["label"] == 2))
        assert len(canopy) > 50, "the view must show the canopy"
        y, x = (int(v) for v in canopy[len(canopy) // 2])
        frame = ctx.read_rgba8()
        ring, fill = (0, 255, 255, 255), (0, 255, 255, 64)
        want = scene.outline_frame(frame, recs, (0, 0, W, H), scene.selection_mask([2]), ring, fill, 3)
        p = d.highlight_at(ctx, x, y, ring_rgba=ring, fill_rgba=fill, radius=3)
        _same("highlight_at", ctx.read_outline(), want)
        assert p["status"] == "hit" and p["label"] == 2 and p["segment"] == "Canopy"
        again = d.highlight_at(ctx, x, y, ring_rgba=ring, fill_rgba=fill, radius=3)      # the records are current: no new pick pass
        assert again == p
        assert d.highlight(ctx, ["Canopy"], ring, fill, 3) == [2]
        _same("highlight by name", ctx.read_outline(), want)
        assert d.highlight(ctx, ["canopy", 2], ring, fill, 3) == [2]
        _same("highlight by id and value", ctx.read_outline(), want)
        assert p == d.pick(ctx, x, y)                                 # what Simple.pick returns
        # a pixel that shows nothing: nothing outlined, the image is the frame
        miss = np.argwhere(recs["status"] != 2)
        my, mx = (int(v) for v in miss[0])
        assert d.highlight_at(ctx, mx, my)["status"] in ("miss", "none")
        _same("hover over the background", ctx.read_outline(), frame)
        # hiding a segment makes the records stale: the next highlight picks again
        d.set_hidden(ctx, [4])
        d.compute_pass(ctx)
        d.highlight(ctx, ["Canopy"], ring, fill, 3)
        got = ctx.read_outline()
        _same("after set_hidden", got, scene.outline_frame(ctx.read_rgba8(), ctx.read_picks(), (0, 0, W, H), scene.selection_mask([2]), ring, fill, 3))


# ---- 3. one large frame ---------------------------------------------------------------------------------------------------------
def test_bonsai256_at_1080p(oracle, volym_lib):
    from volym_amd import demo, scene
    n, w, h = 256, 1920, 1080
    canopy = scene.selection_mask([2])
    with demo.GpuContext(w, h, 0) as ctx:
        _scene(ctx, POSES[0], oracle, dims_vol_labels=_bonsai(n))
        ctx.compute_pass()
        ctx.pick_pass(None, 0.5)
        ctx.outline_pass(canopy, RING, FILL, 3)
        got = ctx.read_outline()
        frame, picks = ctx.read_rgba8(), ctx.read_picks()
        n_canopy = int(((picks["status"] == 2) & (picks["label"] == 2)).sum())
        assert n_canopy > 5000, n_canopy
        _same("256^3 at 1920x1080, radius 3", got, scene.outline_frame(frame, picks, (0, 0, w, h), canopy, RING, FILL, 3))
    common._cache.pop(("bonsai", n), None)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(oracle, volym_lib):
    from volym_amd import _lib, scene
    L = _lib.lib()
    W, H = 96, 64
    sel = scene.selection_mask([2])

    def code(call):
        with pytest.raises(_lib.VolymError) as e:
            call()
        return e.value.code

    o = _lib.Outline(radius=2)
    out = np.zeros((H, W, 4), np.uint8)
    with _ctx(-1, w=W, h=H) as c:
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2)) == _lib.E_STATE                   # no compute pass (nor a scene)
        assert code(c.read_outline) == _lib.E_STATE
        assert c.outline_device_ptr() is None
        _scene(c, POSES[1], oracle)
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2)) == _lib.E_STATE                   # still no compute pass
        c.pick_pass(None, 0.3)
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2)) == _lib.E_STATE                   # a pick pass, but no compute pass
        records = torch.zeros(W * H * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2, records_ptr=records.data_ptr(), rect=(0, 0, W, H))) == _lib.E_STATE
    with _ctx(-1, w=W, h=H) as c:
        _scene(c, POSES[1], oracle)
        c.compute_pass()
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2)) == _lib.E_STATE                   # a compute pass, but no pick pass
        records = torch.zeros(W * H * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptr = records.data_ptr()
        for radius in (0, 9, 2 ** 32 - 1):
            assert code(lambda: c.outline_pass(sel, RING, FILL, radius, records_ptr=ptr, rect=(0, 0, W, H))) == _lib.E_INVALID, radius
        for rect in ((W, 0, 1, 1), (0, H, 1, 1), (0, 0, W + 1, 1), (1, 0, W, 1), (0, 1, 1, H), (2 ** 32 - 1, 0, 2, 1), (0, 0, 2 ** 32 - 1, 2 ** 32 - 1),
                     (5, 5, 0, 3), (5, 5, 3, 0), (0, 0, 0, 0)):
            assert code(lambda: c.outline_pass(sel, RING, FILL, 2, records_ptr=ptr, rect=rect)) == _lib.E_INVALID, rect
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2, records_ptr=ptr)) == _lib.E_INVALID          # records without rect
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2, rect=(0, 0, W, H))) == _lib.E_INVALID        # rect without records
        assert L.volym_outline_pass(None, C.byref(o), None, None, None) == _lib.E_INVALID
        assert L.volym_outline_pass(c.handle, None, None, None, None) == _lib.E_INVALID
        assert L.volym_read_outline(None, scene._u8p(out)) == _lib.E_INVALID
        assert L.volym_read_outline(c.handle, None) == _lib.E_INVALID
        assert L.volym_outline_device_ptr(None) is None
        assert code(c.read_outline) == _lib.E_STATE                                               # none of the refused calls was a pass
        target = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.outline_pass(sel, RING, FILL, 2, records_ptr=ptr, rect=(0, 0, W, H), target_ptr=target.data_ptr())
        c.sync()
        assert code(c.read_outline) == _lib.E_STATE                                               # a pass, but not into the own target
        assert c.outline_device_ptr() is None
        # the context still works
        frame = c.read_rgba8()
        c.pick_pass(None, 0.3)
        c.outline_pass(sel, RING, FILL, 8)
        _same("after the refusals", c.read_outline(), scene.outline_frame(frame, c.read_picks(), (0, 0, W, H), sel, RING, FILL, 8))
        assert c.outline_device_ptr()
    # a sharded context
    with _ctx(-1, w=W, h=H) as c:
        c.set_shard(0, 2)
        _scene(c, POSES[1], oracle)
        c.compute_pass()
        c.pick_pass(None, 0.3)
        assert code(lambda: c.outline_pass(sel, RING, FILL, 2)) == _lib.E_STATE
