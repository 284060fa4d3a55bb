"""The projection pass on the device (volym_project_pass / volym_project_image_pass / volym_read_projection / volym_project_at).

The expected records and images are scene.project_frame, the host twin of the rule (tests/test_project_host.py pins its rays to
tests/pick_reference.py and its values to closed forms), of the prepared arrays the context was given, the cut state it was put in
and the uniforms of its last update.  Every comparison is byte for byte, t bit for bit, over every ray: every decision of the rule
is on integers or on f32 values the ray set-up reproduces bit-equal, so there is no tolerance and no ray is left out.

Scenes: synth_bonsai(32) with labels at 96 x 64, and a non-cubic 40 x 24 x 56 cut out of synth_bonsai(64) at 72 x 40 (neither frame
dimension a multiple of 16; with 32 macro cells the cells of the 24-voxel axis share voxels).  Orbit poses only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests.project_scenes import BACKGROUND, BOXES, COMBOS, POSES, SCENES, STEPS, F, empty_cells, palette, scene_bytes, tie_fraction
from tests.test_gpu_crop_box import CANOPY, _uniforms, _ctx

pytestmark = pytest.mark.gpu

_twin = {}


def _twin_records(name, cu, pose, step, cut=None):
    """the twin's records of the whole frame, marched once per (scene, pose, step, cut)"""
    from volym_amd import scene
    key = (name, pose, step, repr(cut))
    if key not in _twin:
        dims, vol, labels = scene_bytes(name)
        w, h = SCENES[name]
        now = scene.cut_volume(vol, dims, cut, labels)
        _twin[key] = scene.project_frame(now, dims, cu, w, h, scene.Projection(step), labels=labels)[0]
    return _twin[key]


def _same_records(what, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = (got.view(np.uint8).reshape(got.shape + (16,)) != want.view(np.uint8).reshape(want.shape + (16,))).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _same_image(what, got, want):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


def _upload(ctx, name, labels=True, lut=None):
    from volym_amd import scene
    dims, vol, lab = scene_bytes(name)
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut() if lut is None else lut)
    if labels:
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(CANOPY)
    else:
        ctx.set_importances(CANOPY[lab], dims)
    return dims, vol, lab


def _projection(step, mode=0, flags=0):
    from volym_amd import scene
    return scene.Projection(step, mode, flags, BACKGROUND, palette())


# ---- 1. every record and image, over layouts, macro cells, steps, modes, flags, tables ---------------------------------------------------
@pytest.mark.parametrize("mc", [4, 32])
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("name", list(SCENES))
def test_records_and_images_equal_the_twin(oracle, volym_lib, name, layout, mc):
    from volym_amd import _lib, scene
    w, h = SCENES[name]
    rng = np.random.default_rng(17)
    luts = {n: rng.integers(0, 256, (n, 4)).astype(np.uint8) for n in (1, 7, 256)}
    with _ctx(layout, [(_lib.OPT_MACRO_CELLS, mc)], w=w, h=h) as ctx:
        dims, vol, labels = _upload(ctx, name, lut=luts[7])
        assert ctx.projection_device_ptr() is None and ctx.projection_image_device_ptr() is None
        for pose in POSES:
            _, _, cu, pu = _uniforms(oracle, w, h, pose)
            ctx.update(cu, pu)
            for step in STEPS:
                want = _twin_records(name, cu, pose, step)
                hit = want["status"] > 0
                if pose == POSES[0] and step == 0.01:
                    # a vacuous scene fails loudly: at least half the rays hit, at least half of the hit rays tie
                    assert hit.sum() >= w * h / 2, (name, int(hit.sum()))
                    assert tie_fraction(vol, dims, cu, w, h, step, want) >= 0.5, name
                    assert (want["status"] == 2).sum() > 0.9 * hit.sum() and (want["label"] != 0).any()
                default = None
                for mode, flags in COMBOS:
                    what = (name, layout, mc, pose, step, mode, flags)
                    p = _projection(step, mode, flags)
                    ctx.project_pass(p, own_image=True)
                    got = ctx.read_projection()
                    _same_records(what, got, want)
                    _same_image(what, ctx.read_projection_image(), scene.project_image(want, p, luts[7]))
                    if flags == 0 and mode == 0:
                        default = got
                    if flags == _lib.PROJECT_NO_SKIP:
                        _same_records(what + ("default against NO_SKIP",), default, got)
            # the table sizes, at the last step
            for tf_n in (1, 256, 7):
                ctx.set_transfer_function(luts[tf_n])
                for mode, flags in ((0, 1), (1, 1), (0, 3)):
                    p = _projection(step, mode, flags)
                    ctx.project_pass(p, own_image=True)
                    _same_image((name, layout, mc, pose, "tf_n", tf_n, mode, flags), ctx.read_projection_image(), scene.project_image(want, p, luts[tf_n]))
            # the same view under a crop box: the scenes' air is noise, so only a cut leaves macro cells empty -- with the box there
            # are empty cells at 4 and at 32 cells per axis, and the default path leaps (the records cannot show it: they are equal)
            box = BOXES[name]
            assert empty_cells(scene.crop_volume(vol, dims, *box), dims, mc) > 0, (name, mc)
            ctx.set_crop_box(*box)
            for step in STEPS:
                want = _twin_records(name, cu, pose, step, {"box": box})
                assert (want["status"] == 1).any() and (want["status"] == 2).any()
                for mode, flags in ((0, 0), (0, 4), (1, 1), (0, 7)):
                    p = _projection(step, mode, flags)
                    ctx.project_pass(p, own_image=True)
                    _same_records((name, layout, mc, pose, step, mode, flags, "box"), ctx.read_projection(), want)
                    _same_image((name, layout, mc, pose, step, mode, flags, "box"), ctx.read_projection_image(), scene.project_image(want, p, luts[7]))
            ctx.set_crop_box((0, 0, 0), dims)
        assert ctx.projection_device_ptr() and ctx.projection_image_device_ptr()


# ---- 2. rects and the one-pixel call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_rects_and_project_at(oracle, volym_lib, layout):
    from volym_amd import scene
    name, pose, step = "cut", POSES[1], 0.0025
    w, h = SCENES[name]
    with _ctx(layout, w=w, h=h) as ctx:
        _upload(ctx, name)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)
        want = _twin_records(name, cu, pose, step)
        p = _projection(step, 0, 2)
        for rect in ((35, 20, 1, 1), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (5, 3, 37, 21), (17, 9, 16, 16), (0, 0, w, h), None):
            x0, y0, rw, rh = rect or (0, 0, w, h)
            ctx.project_pass(p, rect, own_image=True)
            sub = want[y0:y0 + rh, x0:x0 + rw].copy()
            _same_records(("rect", rect), ctx.read_projection(), sub)
            _same_image(("rect", rect), ctx.read_projection_image(), scene.project_image(sub, p))
        # the one-pixel call has a record of its own: the whole frame's records, their size and their pointer stay
        ptr = ctx.projection_device_ptr()
        for x, y in ((35, 20), (0, 0), (w - 1, h - 1), (40, 11)):
            got = ctx.project_at(x, y, step)
            assert got.tobytes() == want[y, x].tobytes(), ((x, y), got, want[y, x])
        assert ctx.projection_device_ptr() == ptr
        _same_records("own records after project_at", ctx.read_projection(), want)
        # the sizes the reads copy, asked of the context
        size = (C.c_uint32 * 2)()
        assert volym_lib.volym_projection_size(ctx.handle, size) == 0 and tuple(size) == (w, h)
        ctx.project_pass(p, (5, 3, 37, 21))
        assert volym_lib.volym_projection_size(ctx.handle, size) == 0 and tuple(size) == (37, 21)
        assert volym_lib.volym_projection_image_size(ctx.handle, size) == 0 and tuple(size) == (w, h)      # the latest image pass was the whole frame
        assert ctx.read_projection().shape == (21, 37) and ctx.read_projection_image().shape == (h, w, 4)


# ---- 3. the cuts: box, plane, hidden segment and their removal, with no volym_update in between ------------------------------------------
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_records_follow_every_cut(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    name, pose, step = "bonsai32", POSES[0], 0.0025
    w, h = SCENES[name]
    dims = scene_bytes(name)[0]
    box, plane, hidden = ((3, 2, 5), (29, 30, 27)), ((5, -3, 7), 150), [2]
    full = {"box": ((0, 0, 0), dims), "plane": ((0, 0, 0), 0), "visible": scene.visibility_mask([])}
    states = [("box", dict(box=box)), ("box + plane", dict(box=box, plane=plane)), ("box + plane + hidden", dict(box=box, plane=plane, visible=scene.visibility_mask(hidden))),
              ("plane + hidden", dict(plane=plane, visible=scene.visibility_mask(hidden))), ("hidden", dict(visible=scene.visibility_mask(hidden))), ("all lifted", dict())]
    with _ctx(layout, w=w, h=h) as ctx:
        _upload(ctx, name)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)                                          # the only update of this test
        before = _twin_records(name, cu, pose, step)
        now = dict(full)
        for what, cut in states:
            new = dict(full, **cut)
            if new["box"] != now["box"]:
                ctx.set_crop_box(*new["box"])
            if new["plane"] != now["plane"]:
                ctx.set_clip_plane(*new["plane"])
            if not np.array_equal(new["visible"], now["visible"]):
                ctx.set_segment_visibility(new["visible"])
            now = new
            want = _twin_records(name, cu, pose, step, {k: (v.tolist() if k == "visible" else v) for k, v in new.items()} if cut else None)
            if cut:
                assert not np.array_equal(want.view(np.uint8), before.view(np.uint8)), (what, "the cut must show")
            for flags in (0, _lib.PROJECT_NO_SKIP):
                ctx.project_pass(_projection(step, 0, flags))
                _same_records((what, flags), ctx.read_projection(), want)
        _same_records("after the removal", ctx.read_projection(), before)


# ---- 4. labels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_labels_in_the_other_layout_than_the_volume(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    name, pose, step = "cut", POSES[0], 0.01
    w, h = SCENES[name]
    with _ctx(layout, w=w, h=h) as ctx:
        dims, vol, lab = scene_bytes(name)
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, 1 - layout)
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(CANOPY)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)
        want = _twin_records(name, cu, pose, step)
        p = _projection(step, 0, 2)
        ctx.project_pass(p, own_image=True)
        _same_records("labels in the other layout", ctx.read_projection(), want)
        _same_image("labels in the other layout", ctx.read_projection_image(), scene.project_image(want, p))


def test_without_labels(oracle, volym_lib):
    from volym_amd import _lib
    name, pose, step = "bonsai32", POSES[1], 0.01
    w, h = SCENES[name]
    with _ctx(0, w=w, h=h) as ctx:
        _upload(ctx, name, labels=False)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)
        want = _twin_records(name, cu, pose, step).copy()
        assert (want["label"] != 0).any()
        want["label"] = 0
        ctx.project_pass(_projection(step))
        _same_records("no labels", ctx.read_projection(), want)
        _refused(_lib.E_STATE, ctx.project_pass, _projection(step, 0, _lib.PROJECT_LABELS))
        # labels of other dimensions than the volume's count as absent
        ctx.set_labels(np.ones(33 * 32 * 32, np.uint8), (33, 32, 32))
        _refused(_lib.E_STATE, ctx.project_pass, _projection(step, 0, _lib.PROJECT_LABELS))
        ctx.project_pass(_projection(step))
        _same_records("labels of other dimensions", ctx.read_projection(), want)


# ---- 5. independence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_frame_is_the_same_with_and_without_projection_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib
    name, pose, step = "bonsai32", POSES[1], 0.0025
    w, h = SCENES[name]
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=w, h=h) as ctx:
        _upload(ctx, name)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)
        want = _twin_records(name, cu, pose, step)
        p = _projection(step, 1, 1)
        ctx.project_pass(p, own_image=True)                         # before any frame
        _same_records("before any frame", ctx.read_projection(), want)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.project_pass(p, own_image=True)
        _same_image("frame read after a projection pass", ctx.read_rgba8(), frame)
        for k in range(3):                                          # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.project_pass(p, own_image=True)
            ctx.compute_pass()
            _same_image(("frame", k), ctx.read_rgba8(), frame)
            _same_records(("records", k), ctx.read_projection(), want)


def test_a_sharded_context_projects_the_whole_frame(oracle, volym_lib):
    from volym_amd import scene
    name, pose, step = "cut", POSES[1], 0.01
    w, h = SCENES[name]
    with _ctx(0, w=w, h=h) as ctx:
        ctx.set_shard(1, 2)
        _upload(ctx, name)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)
        want = _twin_records(name, cu, pose, step)
        p = _projection(step, 0, 3)
        ctx.project_pass(p, own_image=True)
        _same_records("sharded", ctx.read_projection(), want)
        _same_image("sharded", ctx.read_projection_image(), scene.project_image(want, p, scene.default_lut()))


# ---- 6. targets -------------------------------------------------------------------------------------------------------------------------
def test_targets_and_growth(oracle, volym_lib):
    from volym_amd import _lib, scene
    name, pose, step = "bonsai32", POSES[0], 0.01
    w, h = SCENES[name]
    with _ctx(1, w=w, h=h) as ctx:
        _upload(ctx, name)
        _, _, cu, pu = _uniforms(oracle, w, h, pose)
        ctx.update(cu, pu)
        want = _twin_records(name, cu, pose, step)
        p = _projection(step, 0, 2)
        small, large = (30, 20, 9, 5), (3, 2, 70, 50)
        sub = lambda r: want[r[1]:r[1] + r[3], r[0]:r[0] + r[2]].copy()
        # the own buffers grow, then hold a smaller rect: the read is that of the latest pass, and no smaller buffer is made
        ctx.project_pass(p, small)                                  # records alone: no image target exists yet
        assert ctx.projection_device_ptr() and ctx.projection_image_device_ptr() is None
        _refused(_lib.E_STATE, ctx.read_projection_image)
        _same_records("small", ctx.read_projection(), sub(small))
        ctx.project_pass(p, large, own_image=True)
        _same_records("grown", ctx.read_projection(), sub(large))
        _same_image("grown", ctx.read_projection_image(), scene.project_image(sub(large), p))
        ptrs = (ctx.projection_device_ptr(), ctx.projection_image_device_ptr())
        ctx.project_pass(p, small, own_image=True)
        _same_records("shrunk", ctx.read_projection(), sub(small))
        _same_image("shrunk", ctx.read_projection_image(), scene.project_image(sub(small), p))
        assert (ctx.projection_device_ptr(), ctx.projection_image_device_ptr()) == ptrs
        # a caller's tensors, with guards behind them; the own buffers and their reads stay what they were
        n = large[2] * large[3]
        recs = torch.full((n * 16 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        img = torch.full((n * 4 + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.project_pass(p, large, records_ptr=recs.data_ptr(), image_ptr=img.data_ptr())
        ctx.sync()
        got_r, got_i = recs.cpu().numpy(), img.cpu().numpy()
        _same_records("caller's records", got_r[:n * 16].view(_lib.PROJECTION_DTYPE).reshape(large[3], large[2]), sub(large))
        _same_image("caller's image", got_i[:n * 4].reshape(large[3], large[2], 4), scene.project_image(sub(large), p))
        assert (got_r[n * 16:] == 0xA5).all() and (got_i[n * 4:] == 0x5A).all(), "the pass wrote behind its targets"
        _same_records("own records after a pass into a caller's", ctx.read_projection(), sub(small))
        _same_image("own image after a pass into a caller's", ctx.read_projection_image(), scene.project_image(sub(small), p))
        # a caller's records with no image at all
        recs.fill_(0xA5)
        torch.cuda.synchronize()
        ctx.project_pass(p, small, records_ptr=recs.data_ptr())
        ctx.sync()
        got_r = recs.cpu().numpy()
        m = small[2] * small[3]
        _same_records("caller's records, no image", got_r[:m * 16].view(_lib.PROJECTION_DTYPE).reshape(small[3], small[2]), sub(small))
        assert (got_r[m * 16:] == 0xA5).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals(oracle, volym_lib):
    from volym_amd import _lib, scene
    name, step = "bonsai32", 0.01
    w, h = SCENES[name]
    dims, vol, lab = scene_bytes(name)
    p = _projection(step)
    with _ctx(0, w=w, h=h) as ctx:
        _refused(_lib.E_STATE, ctx.project_pass, p)                 # no volume
        size = (C.c_uint32 * 2)(7, 7)
        assert volym_lib.volym_projection_size(ctx.handle, size) == 0 and tuple(size) == (0, 0)
        assert volym_lib.volym_projection_image_size(ctx.handle, size) == 0 and tuple(size) == (0, 0)
        assert volym_lib.volym_projection_size(ctx.handle, None) == _lib.E_INVALID and volym_lib.volym_projection_size(None, size) == _lib.E_INVALID
        _refused(_lib.E_STATE, ctx.read_projection)
        _refused(_lib.E_STATE, ctx.read_projection_image)
        ctx.set_volume(vol, dims, 0)
        assert "transfer function" in _refused(_lib.E_STATE, ctx.project_pass, p.replace(flags=_lib.PROJECT_TF))
        assert "labels" in _refused(_lib.E_STATE, ctx.project_pass, p.replace(flags=_lib.PROJECT_LABELS))
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(CANOPY)
        assert "volym_update" in _refused(_lib.E_STATE, ctx.project_pass, p)     # before any volym_update
        _refused(_lib.E_STATE, ctx.project_at, 3, 3, step)
        _, _, cu, pu = _uniforms(oracle, w, h, POSES[0])
        ctx.update(cu, pu)
        _refused(_lib.E_STATE, ctx.read_projection)                 # before any pass
        ctx.project_pass(p, (4, 4, 8, 8))
        good = ctx.read_projection()
        _refused(_lib.E_STATE, ctx.read_projection_image)           # no image pass yet
        for rect in ((0, 0, 0, 4), (0, 0, 4, 0), (w, 0, 1, 1), (0, h, 1, 1), (w - 3, 0, 4, 1), (0, h - 3, 1, 4), (0, 0, w + 1, h), (1, 1, 0xffffffff, 1)):
            _refused(_lib.E_INVALID, ctx.project_pass, p, rect)
            _refused(_lib.E_INVALID, ctx.project_pass, p, rect, own_image=True)
        _refused(_lib.E_INVALID, ctx.project_at, w, 0, step)
        for bad in (dict(step=0.0), dict(step=5.0e-5), dict(step=1.5), dict(step=float("nan")), dict(step=float("inf")), dict(mode=2), dict(flags=8),
                    dict(mode=1, flags=2)):
            _refused(_lib.E_INVALID, ctx.project_pass, p.replace(**bad))
        _refused(_lib.E_INVALID, ctx.project_at, 3, 3, 0.0)
        assert volym_lib.volym_project_pass(ctx.handle, None, None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_project_pass(None, C.byref(p.to_c()), None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_project_image_pass(None, C.byref(p.to_c()), None) == _lib.E_INVALID
        assert volym_lib.volym_read_projection(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_projection_image(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_project_at(ctx.handle, 1, 1, step, None) == _lib.E_INVALID
        # a refused pass leaves the latest records readable
        _same_records("after the refusals", ctx.read_projection(), good)
        # another volume: the frame of the last update no longer fits
        ctx.set_volume(np.zeros(8 * 8 * 9, np.uint8), (8, 8, 9), 0)
        _refused(_lib.E_STATE, ctx.project_pass, p)


# ---- 8. the demo's faces ------------------------------------------------------------------------------------------------------------------
def test_simple_project_and_brightest_slices(oracle, volym_lib):
    from volym_amd import _lib, demo, scene
    raw, labels_raw = common.bonsai(32)
    dims = (32, 32, 32)
    w, h = 96, 64
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(w / h, params)
    state.update()
    with demo.GpuContext(w, h, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        p = d.project(ctx, "MAX")
        assert F(p.step) == F(0.0025) and p.flags == _lib.PROJECT_LABELS
        _, vol, lab = scene_bytes("bonsai32")
        want, image = scene.project_frame(vol, dims, state.camera_uniforms(), w, h, p, labels=lab)
        _same_records("Simple.project", ctx.read_projection(), want)
        _same_image("Simple.project", ctx.read_projection_image(), image)
        pm = d.project(ctx, "MEAN", tf=True)
        assert pm.mode == _lib.PROJECT_MEAN and pm.flags == _lib.PROJECT_TF
        _same_image("Simple.project MEAN", ctx.read_projection_image(), scene.project_image(want, pm, scene.TransferFunction.default().bake_rgba8()))
        y, x = (int(v) for v in np.argwhere((want["status"] == 2) & (want["label"] == 2))[0])
        r = d.project_at(ctx, x, y)
        assert r["status"] == "hit" and r["label"] == 2 and r["segment"] == "Canopy" and r["max"] == int(want[y, x]["max"])
        assert r["texel"] == (int(want[y, x]["x"]), int(want[y, x]["y"]), int(want[y, x]["z"])) and r["t"] == float(want[y, x]["t"])
        b = d.brightest_slices_at(ctx, x, y)
        assert b["texel"] == r["texel"] and set(b["slices"]) == {"x", "y", "z"}
        for a, axis in enumerate("xyz"):
            s = d.slice(ctx, axis, r["texel"][a])
            assert np.array_equal(ctx.read_slice(), b["slices"][axis])
        miss = np.argwhere(want["status"] == 0)
        if len(miss):
            m = d.brightest_slices_at(ctx, int(miss[0][1]), int(miss[0][0]))
            assert m["status"] == "miss" and m["slices"] is None and m["texel"] is None


# ---- 9. one size check --------------------------------------------------------------------------------------------------------------------
def test_size_check_1080p_of_256_cubed(oracle, volym_lib):
    """synth_bonsai(256) at 1920 x 1080, step 0.0025: the whole frame on the device, 24 sampled rows against the twin"""
    from volym_amd import scene
    raw, lab = common.bonsai(256)
    dims = (256, 256, 256)
    vol, labels = scene.prepare_volume(raw, dims, True), scene.prepare_volume(lab, dims, True)
    w, h, step = 1920, 1080, 0.0025
    rows = np.unique(np.concatenate([[0, 1, h - 1], np.linspace(7, h - 9, 21).astype(np.int64)]))
    assert rows.size == 24
    with _ctx(-1, w=w, h=h) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(labels, dims)
        ctx.set_segment_importances(CANOPY)
        _, _, cu, pu = _uniforms(oracle, w, h, POSES[0])
        ctx.update(cu, pu)
        p = _projection(step, 0, 2)
        ctx.project_pass(p, own_image=True)
        got, image = ctx.read_projection(), ctx.read_projection_image()
        ctx.project_pass(p.replace(flags=6), own_image=True)
        _same_records("default against NO_SKIP", got, ctx.read_projection())
        for y in rows:
            want, wimg = scene.project_frame(vol, dims, cu, w, h, p, rect=(0, int(y), w, 1), labels=labels)
            _same_records(("row", int(y)), got[y:y + 1], want)
            _same_image(("row", int(y)), image[y:y + 1], wimg)
        # the same frame under a crop box, where the default path has empty cells to leap over: both paths, six of the rows
        box = ((40, 30, 50), (200, 220, 190))
        ctx.set_crop_box(*box)
        now = scene.crop_volume(vol, dims, *box)
        ctx.project_pass(p)
        got = ctx.read_projection()
        ctx.project_pass(p.replace(flags=6))
        _same_records("default against NO_SKIP, cropped", got, ctx.read_projection())
        for y in rows[2::4]:
            want, _ = scene.project_frame(now, dims, cu, w, h, p, rect=(0, int(y), w, 1), labels=labels)
            _same_records(("cropped row", int(y)), got[y:y + 1], want)
