"""Oblique clip plane on the device (volym_set_clip_plane).  A frame with plane (n, d) is the frame of the scene whose density AND
importance bytes are 0 in every texel with n . (x, y, z) > d: the expected pictures come from oracle.render on
scene.clip_volume-zeroed inputs (<= 1e-4 on f32, <= 1 rgba8 LSB), and a twin context that receives the zeroed bytes through
set_volume / set_importances must give bit-equal rgba8 and f32.  After every edit three frames of the standing view are read and
must be bit-equal to each other.  Scenes, helpers and tolerances are those of tests/test_gpu_crop_box.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import common
from tests.test_gpu_crop_box import (CANOPY, H, PARAMS, POT, W, _bonsai, _changed, _ctx, _frame, _near, _oracle, _ragged, _same, _table, _three,
                                     _uniforms)

pytestmark = pytest.mark.gpu

NONE = ((0, 0, 0), 0)
POSE = (35.0, 20.0, 0.0)
IMP_PLANES = [((0, 1, 0), 31), ((1, 3, 0), 128), ((-1, 4, 1), 128)]       # pot important, seen from below: tests/test_clip_plane.py
IMP_POSE = (0.0, -80.0, 0.0)


def _sequence(dims):
    nx, ny, nz = dims
    s = nx + ny + nz
    return [
        ("a z face", (0, 0, 1), 40 * nz // 64),
        ("diagonal half", (1, 1, 1), s // 2),
        ("one layer more", (1, 1, 1), s // 2 + 1),
        ("the flip", (-1, -1, -1), -(s // 2)),
        ("oblique", (3, -2, 5), 3 * nx // 2 - ny + 5 * nz // 2),
        ("largest coefficient", (4096, 1, 0), 4096 * (nx // 2)),
        ("negative, no y", (-7, 0, 2), -7 * (nx // 3)),
        ("nothing kept", (1, 0, 0), -1),
        ("no plane",) + NONE,
    ]


def _plane5(dims):
    return _sequence(dims)[4][1:]


def _clip(scene, dims, plane, *volumes):
    return [scene.clip_volume(v, dims, *plane) for v in volumes]


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_edit_sequence(oracle, volym_lib, volume, layout):
    """Plane after plane on one context against a twin that is handed the host-zeroed bytes, and against the oracle.  bonsai: the
    importances come from labels on the device; ragged (97 x 80 x 71: linear chunks wrap rows, bricks are partial): uploaded
    importances.  (On the CPU: 8 of the 8 planes change more than 1 % of the base-mode pixels on the bonsai, 7 on the ragged
    volume, whose flip changes none.)"""
    from volym_amd import scene
    if volume == "bonsai64":
        dims, vol, labels = _bonsai()
        table = CANOPY
    else:
        dims, vol, labels = _ragged()
        table = _table(l2=255)
    imp = table[labels]
    lut = scene.default_lut()
    modes = {k: _uniforms(oracle, W, H, POSE, **PARAMS[k]) for k in ("base", "straight")}
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        if volume == "bonsai64":
            dev.set_labels(labels, dims)
            dev.set_segment_importances(table)
        else:
            dev.set_importances(imp, dims)
        twin.set_transfer_function(lut)
        assert dev.clip_plane() == NONE
        before = {k: _three(dev, (k, "uncut"), cu, pu) for k, (cam, par, cu, pu) in modes.items()}
        uncut = {k: _oracle(oracle, vol, imp, dims, cam, par) for k, (cam, par, cu, pu) in modes.items()}
        for k in modes:
            _near((volume, layout, k, "uncut"), before[k], uncut[k])
        cutting = 0
        for name, n, d in _sequence(dims):
            cvol, cimp = _clip(scene, dims, (n, d), vol, imp)
            twin.set_volume(cvol, dims, 0)
            twin.set_importances(cimp, dims)
            for k, (cam, par, cu, pu) in modes.items():
                what = (volume, layout, name, k)
                if k == "base":
                    dev.update(cu, pu)                      # the view of this mode, then the edit with NO update after it
                    _frame(dev)
                    dev.set_clip_plane(n, d)
                    assert dev.clip_plane() == (n, d)
                    got = _three(dev, what)
                else:
                    got = _three(dev, what, cu, pu)
                _same(what + ("twin",), got, _frame(twin, cu, pu))
                ref = _oracle(oracle, cvol, cimp, dims, cam, par)
                _near(what, got, ref)
                if k == "base" and (n, d) != NONE and _changed(ref[1], uncut[k][1]) > 0.01:
                    cutting += 1
                if (n, d) == NONE:
                    _same(what + ("equals the frame before any plane",), got, before[k])
        assert cutting >= 6, "the sequence must cut into the picture: %d of 8 planes change more than 1 %% of the pixels" % cutting


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_modes(oracle, volym_lib, layout):
    """Every mode on the oblique plane, both filters.  The importance cases are ones where oracle(clipped density, clipped
    importances) differs from oracle(clipped density, FULL importances): a library that clipped the density alone fails them."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    plane = _plane5(dims)
    imp = CANOPY[labels]
    cvol, cimp = _clip(scene, dims, plane, vol, imp)
    for filt in (0, 1):
        with _ctx(layout) as dev, _ctx(layout) as twin:
            dev.set_volume(vol, dims, filt)
            dev.set_importances(imp, dims)
            dev.set_transfer_function(lut)
            twin.set_volume(cvol, dims, filt)
            twin.set_importances(cimp, dims)
            twin.set_transfer_function(lut)
            dev.set_clip_plane(*plane)
            for name in (("base", "no opacity", "smoothing", "colouring") if filt == 0 else ("base", "straight")):
                cam, par, cu, pu = _uniforms(oracle, W, H, POSE, **PARAMS[name])
                ref = _oracle(oracle, cvol, cimp, dims, cam, par, filter=filt)
                if name == "base" and filt == 0:
                    assert _changed(ref[1], _oracle(oracle, vol, imp, dims, cam, par)[1]) > 0.01, "the plane must cut into the picture"
                got = _three(dev, (layout, filt, name), cu, pu)
                _same((layout, filt, name, "twin"), got, _frame(twin, cu, pu))
                _near((layout, filt, name), got, ref)
    imp = POT[labels]
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_labels(labels, dims)
        dev.set_segment_importances(POT)
        dev.set_transfer_function(lut)
        twin.set_transfer_function(lut)
        for plane in IMP_PLANES:
            cvol, cimp = _clip(scene, dims, plane, vol, imp)
            twin.set_volume(cvol, dims, 0)
            twin.set_importances(cimp, dims)
            dev.set_clip_plane(*plane)
            for name in ("straight", "cone"):
                cam, par, cu, pu = _uniforms(oracle, W, H, IMP_POSE, **PARAMS[name])
                ref = _oracle(oracle, cvol, cimp, dims, cam, par)
                frac = _changed(ref[1], _oracle(oracle, cvol, imp, dims, cam, par)[1])
                assert frac > 0.01, (plane, name, frac)
                got = _three(dev, (layout, plane, name), cu, pu)
                _same((layout, plane, name, "twin"), got, _frame(twin, cu, pu))
                _near((layout, plane, name), got, ref)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_commutes(oracle, volym_lib, layout):
    """Box, plane and mask in three orders, and a fourth context that reaches the same state through detours: the box grown over
    clipped texels and shrunk again, the plane lifted and set again while a segment is hidden, the table set under all three."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    lo, hi = (5, 7, 9), (50, 61, 43)
    plane = _plane5(dims)
    visible = scene.visibility_mask([3])
    table = CANOPY

    def cut(v):
        return scene.crop_volume(scene.clip_volume(scene.hide_segments(v, labels, visible), dims, *plane), dims, lo, hi)

    cvol, cimp = cut(vol), cut(table[labels])
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE, **PARAMS["straight"])
    ref = _oracle(oracle, cvol, cimp, dims, cam, par)
    assert _changed(ref[1], _oracle(oracle, vol, table[labels], dims, cam, par)[1]) > 0.01
    with _ctx(layout) as twin:
        twin.set_volume(cvol, dims, 0)
        twin.set_importances(cimp, dims)
        twin.set_transfer_function(lut)
        want = _frame(twin, cu, pu)
    _near((layout, "twin"), want, ref)
    edits = {"box": lambda c: c.set_crop_box(lo, hi), "plane": lambda c: c.set_clip_plane(*plane), "mask": lambda c: c.set_segment_visibility(visible)}
    for order in (("box", "plane", "mask"), ("plane", "mask", "box"), ("mask", "box", "plane"), "detours"):
        with _ctx(layout) as dev:
            dev.set_volume(vol, dims, 0)
            dev.set_transfer_function(lut)
            dev.set_labels(labels, dims)
            if order == "detours":
                dev.set_clip_plane(*plane)
                dev.set_crop_box(lo, hi)
                dev.set_crop_box((0, 0, 0), dims)                  # the box grows over clipped texels: they stay 0
                dev.set_segment_visibility(visible)
                dev.set_clip_plane(*NONE)                          # lifted and set again while hidden
                dev.set_clip_plane((1, 1, 1), 80)
                dev.set_crop_box(lo, hi)
                dev.set_clip_plane(*plane)
                dev.set_segment_importances(table)                 # made under all three
            else:
                dev.set_segment_importances(table)
                for e in order:
                    edits[e](dev)
            assert dev.clip_plane() == plane and dev.crop_box() == (lo, hi)
            _same((layout, order), _three(dev, (layout, order), cu, pu), want)


@pytest.mark.parametrize("slots", [1, 2], ids=["one slot", "two in flight"])
def test_edit_between_enqueued_passes(oracle, volym_lib, slots):
    """A pass enqueued before the edit shows the old plane, the two enqueued after it the new one, with no volym_update and no
    sync by the caller in between; with VOLYM_OPT_FRAMES_IN_FLIGHT = 2 the later two come from both frame slots."""
    from volym_amd import _lib, scene
    import torch
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    lut = scene.default_lut()
    planes = [NONE, ((0, 0, 1), 40), ((1, 1, 1), 96), _plane5(dims), NONE]
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE, **PARAMS["straight"])
    refs = [_oracle(oracle, *_clip(scene, dims, p, vol, imp), dims, cam, par) for p in planes]
    assert _changed(refs[1][1], refs[0][1]) > 0.01 and _changed(refs[2][1], refs[1][1]) > 0.01
    bufs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    with _ctx(-1, [(_lib.OPT_FRAMES_IN_FLIGHT, slots)]) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_importances(imp, dims)
        dev.set_transfer_function(lut)
        dev.update(cu, pu)
        for i in range(1, len(planes)):
            dev.bind_output(None, bufs[0].data_ptr())
            dev.compute_pass()
            dev.set_clip_plane(*planes[i])
            for b in (1, 2):
                dev.bind_output(None, bufs[b].data_ptr())
                dev.compute_pass()
            dev.sync()
            old, new1, new2 = (b.cpu().numpy() for b in bufs)
            for what, got, ref in (("before the edit", old, refs[i - 1]), ("first after", new1, refs[i]), ("second after", new2, refs[i])):
                du8 = int(np.abs(got.astype(np.int32) - ref[1].astype(np.int32)).max())
                assert du8 <= 1, (slots, i, what, du8)
            assert np.array_equal(new1, new2), (slots, i)
        dev.bind_output(None, None)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_lifetime(oracle, volym_lib, layout):
    """The plane belongs to the scene: importances that arrive under it are clipped, and volym_set_volume resets it."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    plane = IMP_PLANES[1]
    cam, par, cu, pu = _uniforms(oracle, W, H, IMP_POSE, **PARAMS["straight"])
    cvol, cimp = _clip(scene, dims, plane, vol, POT[labels])
    ref = _oracle(oracle, cvol, cimp, dims, cam, par)
    assert _changed(ref[1], _oracle(oracle, cvol, POT[labels], dims, cam, par)[1]) > 0.01       # unclipped importances would show
    with _ctx(layout) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        dev.set_clip_plane(*plane)
        dev.set_importances(POT[labels], dims)                       # plane, then set_importances
        _near((layout, "set_importances under a plane"), _three(dev, "set_importances under a plane", cu, pu), ref)
        dev.set_importances(CANOPY[labels], dims)
        dev.set_labels(labels, dims)                                 # plane, then set_labels + table
        dev.set_segment_importances(POT)
        assert dev.clip_plane() == plane
        _near((layout, "labels + table under a plane"), _three(dev, "labels + table under a plane"), ref)
        dev.set_labels(labels, dims)                                 # labels again under the plane: the mapped importances stay
        dev.set_clip_plane((0, 1, 0), 40)
        dev.set_clip_plane(*plane)
        _near((layout, "labels replaced under a plane"), _three(dev, "labels replaced under a plane"), ref)
        # set_volume resets the plane, and the importances get their texels back
        dev.set_volume(vol, dims, 0)
        assert dev.clip_plane() == NONE
        _near((layout, "set_volume after a plane"), _three(dev, "set_volume after a plane", cu, pu), _oracle(oracle, vol, POT[labels], dims, cam, par))


def test_errors_leave_the_context_rendering(oracle, volym_lib):
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE)
    L = _lib.lib()
    i3 = C.c_int32 * 3
    with _ctx(-1) as c:
        for call in (lambda: c.set_clip_plane((0, 0, 1), 5), c.clip_plane):
            with pytest.raises(_lib.VolymError) as e:                  # no volume yet
                call()
            assert e.value.code == _lib.E_STATE
        c.set_volume(vol, dims, 0)
        c.set_importances(imp, dims)
        c.set_transfer_function(scene.default_lut())
        plane = _plane5(dims)
        c.set_clip_plane(*plane)
        for n, d in (((4097, 0, 0), 5), ((0, -4097, 1), 5), ((0, 0, 0), 1), ((0, 0, 0), -1), ((2 ** 31 - 1, 0, 0), 0)):
            assert L.volym_set_clip_plane(c.handle, i3(*n), d) == _lib.E_INVALID, (n, d)
            assert c.clip_plane() == plane
        assert L.volym_set_clip_plane(c.handle, None, 0) == _lib.E_INVALID
        with pytest.raises(ValueError):
            c.set_clip_plane((4097, 0, 0), 5)
        got = _three(c, "after the refused planes", cu, pu)
        _near("after the refused planes", got, _oracle(oracle, *_clip(scene, dims, plane, vol, imp), dims, cam, par))


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_fetch_counters(oracle, volym_lib, layout):
    """volym_stats_pass counts the reference's fetches whether or not the reject box spares one, so under a plane every field
    equals the twin's (whose reject box comes from a scan of the zeroed bytes), and the oracle's on the zeroed inputs."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    plane = IMP_PLANES[2]
    imp = POT[labels]
    cvol, cimp = _clip(scene, dims, plane, vol, imp)
    cam, par, cu, pu = _uniforms(oracle, W, H, IMP_POSE, **PARAMS["straight"])
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_importances(imp, dims)
        dev.set_transfer_function(scene.default_lut())
        dev.set_clip_plane(*plane)
        twin.set_volume(cvol, dims, 0)
        twin.set_importances(cimp, dims)
        twin.set_transfer_function(scene.default_lut())
        dev.update(cu, pu)
        twin.update(cu, pu)
        got, want = dev.stats_pass(), twin.stats_pass()
        assert got == want, (got, want)
        ref = _oracle(oracle, cvol, cimp, dims, cam, par)[2]
        for k in ("n_vol", "n_imp", "n_steps", "n_dense", "n_hit"):
            assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_pick(oracle, volym_lib, layout):
    """The pick marches the clipped bytes: a whole-frame pick pass equals, byte for byte, that of a twin handed clipped density
    and clipped labels (label 0 maps to importance 0, so its importances are the clipped ones).  Then click to cut."""
    from volym_amd import _lib, demo, scene
    dims, vol, labels = _bonsai()
    plane = _plane5(dims)
    table = CANOPY
    assert table[0] == 0
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE)
    with _ctx(layout) as dev, _ctx(layout) as twin:
        for c, v, l in ((dev, vol, labels), (twin,) + tuple(_clip(scene, dims, plane, vol, labels))):
            c.set_volume(v, dims, 0)
            c.set_labels(l, dims)
            c.set_segment_importances(table)
            c.set_transfer_function(scene.default_lut())
            c.update(cu, pu)
        dev.set_clip_plane(*plane)
        records = []
        for c in (dev, twin):
            c.compute_pass()
            c.pick_pass(None, 0.5)
            c.sync()
            records.append(c.read_picks())
        assert records[0].tobytes() == records[1].tobytes()
        assert (records[0]["status"] == 2).mean() > 0.01
    # Simple.clip_at: the plane through what the pixel shows, facing the eye
    raw, labels_raw = common.bonsai(64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    with demo.GpuContext(W, H, 0) as ctx:
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        d.set_labels(ctx, labels_raw)
        d.compute_pass(ctx)
        ctx.pick_pass(None, 0.5)
        ctx.sync()
        before, rec = ctx.read_rgba8(), ctx.read_picks()
        ys, xs = np.nonzero(rec["status"] != 2)                                     # a pixel that shows nothing
        assert ys.size and d.clip_at(ctx, int(xs[0]), int(ys[0])) is None and ctx.clip_plane() == NONE
        ys, xs = np.nonzero((rec["status"] == 2) & (rec["label"] == 2))             # the canopy
        assert ys.size > 20
        i = ys.size // 2
        x, y = int(xs[i]), int(ys[i])
        got = d.clip_at(ctx, x, y)
        assert got is not None and got == ctx.clip_plane()
        n, dd = got
        texel = tuple(int(rec[y, x][k]) for k in ("x", "y", "z"))
        assert sum(a * t for a, t in zip(n, texel)) <= dd                           # the picked texel's density is kept
        eye = state.camera.position
        assert sum(a * (e * s - 0.5) for a, e, s in zip(n, eye, dims)) > dd         # and the eye is on the side that goes
        d.compute_pass(ctx)
        ctx.sync()
        assert not np.array_equal(ctx.read_rgba8(), before)
        p = d.pick(ctx, x, y)
        assert p["status"] != "hit" or p["t"] >= float(rec[y, x]["t"]) - 1e-6       # nothing in front of the clicked point is left


def test_mgpu_virtual_ranks(oracle, volym_lib):
    from volym_amd import mgpu, scene
    dims, vol, labels = _bonsai()
    imp = POT[labels]
    w, h = 310, 170
    cam, par, cu, pu = _uniforms(oracle, w, h, IMP_POSE, **PARAMS["straight"])
    planes = [IMP_PLANES[1], _plane5(dims), ((1, 1, 1), 96), NONE]
    single = {}
    with _ctx(-1, w=w, h=h) as one:
        one.set_volume(vol, dims, 0)
        one.set_transfer_function(scene.default_lut())
        one.set_labels(labels, dims)
        one.set_segment_importances(POT)
        one.update(cu, pu)
        for p in planes:
            one.set_clip_plane(*p)
            one.compute_pass()
            one.sync()
            single[p] = one.read_rgba8()
    ref = _oracle(oracle, *_clip(scene, dims, planes[0], vol, imp), dims, cam, par, w, h, want_f32=False)
    assert int(np.abs(single[planes[0]].astype(np.int32) - ref[1].astype(np.int32)).max()) <= 1
    assert all(not np.array_equal(single[a], single[b]) for a, b in zip(planes, planes[1:]))
    with mgpu.MultiGpu(w, h, devices=[0, 0], transport=mgpu.COPY) as mg:
        mg.set_volume(vol, dims, 0)
        mg.set_transfer_function(scene.default_lut())
        mg.set_labels(labels, dims)
        mg.set_segment_importances(POT)
        mg.set_clip_plane(*planes[0])
        mg.update(cu, pu)
        mg.prepare(0)
        t = mg.run(3, use_graph=False)
        assert t["overflowed"] == 0
        assert np.array_equal(mg.read_rgba8(), single[planes[0]]), "plain enqueues"
        # the captured loop at a standing view: only the set-up call itself can tell the loop that its graph is of another scene
        t = mg.run(4 * 4, use_graph=True)
        assert t["graph_replays"] >= 1 and np.array_equal(mg.read_rgba8(), single[planes[0]])
        for p in planes[1:]:
            mg.set_clip_plane(*p)
            t = mg.run(4 * 4, use_graph=True)
            assert t["graph_replays"] >= 1 and t["overflowed"] == 0
            assert np.array_equal(mg.read_rgba8(), single[p]), ("graph after an edit at a standing view", p)


def test_simple_set_clip_plane(oracle, volym_lib):
    """demo.Simple.set_clip_plane: unit-cube normal and point (scene.clip_plane_texels)."""
    from volym_amd import demo, scene
    raw, labels_raw = common.bonsai(64)
    dims = (64, 64, 64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    with demo.GpuContext(W, H, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        assert d.set_clip_plane(ctx, (0, 0, 1), (0.5, 0.5, 0.625)) == ((0, 0, 4096), 161792) == ctx.clip_plane()
        n, dd = d.set_clip_plane(ctx, (1.0, 0.5, 1.0), (0.5, 0.5, 0.5))
        assert (n, dd) == scene.clip_plane_texels((1.0, 0.5, 1.0), (0.5, 0.5, 0.5), dims) == ctx.clip_plane()
        d.compute_pass(ctx)
        ctx.sync()
        vol, imp = common.oracle_scene(oracle, raw, labels_raw, common.BONSAI_SEGMENTS, dims)
        cam = oracle.benchmark_camera_uniforms(W / H)
        par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01)
        ref = _oracle(oracle, *_clip(scene, dims, (n, dd), vol, imp), dims, cam, par, want_f32=False)
        assert _changed(ref[1], _oracle(oracle, vol, imp, dims, cam, par, want_f32=False)[1]) > 0.01
        assert int(np.abs(ctx.read_rgba8().astype(np.int32) - ref[1].astype(np.int32)).max()) <= 1
        assert d.set_clip_plane(ctx, None, None) == NONE == ctx.clip_plane()


def test_flythrough_clip_plane_frames_match_oracle(oracle, volym_lib, tmp_path):
    """`python -m volym_amd flythrough --clip-plane`: frames.json records the integer plane, and every kept frame matches the
    oracle on those uniforms and the clipped bytes, rgba8 within 1 LSB."""
    from volym_amd import __main__ as cli, image, scene, synth
    out = str(tmp_path)
    assert cli.main(["flythrough", "--width", "192", "--height", "108", "--frames", "24", "--keep-every", "6", "--out", out,
                     "--clip-plane", "1,0.5,1,0.5,0.5,0.5"]) == 0
    meta = json.load(open(os.path.join(out, "frames.json")))
    Wf, Hf = meta["width"], meta["height"]
    raw, labels = common.teapot()
    dims = (256, 256, 256)
    want = scene.clip_plane_texels((1, 0.5, 1), (0.5, 0.5, 0.5), dims)
    vol, imp = common.oracle_scene(oracle, raw, labels, synth.TEAPOT_SEGMENTS, dims)
    cvol, cimp = _clip(scene, dims, want, vol, imp)
    lut = oracle.tf_default_lut()
    assert len(meta["frames"]) >= 3
    cut = 0
    for fr in meta["frames"]:
        assert (tuple(fr["clip_plane"]["n"]), fr["clip_plane"]["d"]) == want
        cam = oracle.CameraUniforms.from_buffer_copy(bytes.fromhex(fr["camera_uniforms"]))
        par = oracle.Parameters.from_buffer_copy(bytes.fromhex(fr["parameter_uniforms"]))
        _, ref, _ = oracle.render(cvol, cimp, dims, lut, cam, par, Wf, Hf, want_f32=False)
        got = image.read_png_rgba8(os.path.join(out, fr["png"]))
        assert int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max()) <= 1, (fr["frame"], fr["event"])
        _, full, _ = oracle.render(vol, imp, dims, lut, cam, par, Wf, Hf, want_f32=False)
        cut += int((ref != full).any(axis=-1).mean() > 0.01)
    assert cut >= 2, cut
