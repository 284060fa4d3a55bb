"""The surface passes on the device (volym_surface_pass / volym_read_surface / volym_surface_faces_pass / volym_read_surface_faces).

The expected result is scene.surface_volume, the host twin of the rule (pinned to a plain triple loop by tests/test_surface_host.py),
of the prepared arrays the context was given and the cut state it was put in.  Every comparison is over all 24584 bytes of the summary
and every byte of the face list, in its one canonical order: the rule is integer, so there is no tolerance and nothing is left out.
The scenes, boxes, cuts, select tables and thresholds are those of tests/surface_scenes.py, whose properties tests/test_surface_host.py
asserts on the twin.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import surface_scenes as S
from tests.test_gpu_crop_box import CANOPY, _bonsai, _uniforms, _ctx

pytestmark = pytest.mark.gpu


def _same(what, got, want):
    if S.as_bytes(got) == S.as_bytes(want):
        return
    for k in ("faces", "pos", "neg"):
        bad = np.argwhere(got[0][k] != want[0][k])
        assert bad.size == 0, (what, k, bad[:6].tolist(), got[0][k][got[0][k] != want[0][k]][:6].tolist(), want[0][k][got[0][k] != want[0][k]][:6].tolist())
    assert int(got[0]["total"]) == int(want[0]["total"]), (what, "total")
    assert len(got[1]) == len(want[1]), (what, "records", len(got[1]), len(want[1]))
    bad = np.flatnonzero(got[1] != want[1])
    assert bad.size == 0, (what, "records", bad[:6].tolist(), got[1][bad[:3]].tolist(), want[1][bad[:3]].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _run(ctx, s):
    """surface pass, emit pass into the context's own buffer, both reads"""
    ctx.surface_pass(s)
    ctx.surface_faces_pass()
    summary = ctx.read_surface()
    return summary, ctx.read_surface_faces(summary["total"])


def _check(ctx, host, what, s, labels=True):
    want = S.expect(host, s, labels)
    _same(what, _run(ctx, s), want)
    return want


# ---- 1. boxes, select tables, thresholds and cuts, both scenes, both layouts ----------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    """every box x select x min_byte before any cut; then after each edit, without a volym_update, in a context that never had a view"""
    from volym_amd import _lib
    host = S.scene_a() if which == "a" else S.scene_b()
    found = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.surface_device_ptr() is None
        for name, s in S.every_surface():
            found += int(_check(ctx, host, ("never cut", name), s)[0]["total"])
        assert ctx.surface_device_ptr()
        for name, s in S.surfaces(_lib.SURFACE_UNCUT):
            _check(ctx, host, ("uncut, never cut", name), s)
        for step, box, plane, hidden in S.CUTS:
            host.set_cut(ctx, box, plane, hidden)
            for name, s in S.surfaces():
                found += int(_check(ctx, host, (step, name), s)[0]["total"])
            for name, s in S.surfaces(_lib.SURFACE_UNCUT)[:4]:
                _check(ctx, host, (step, "uncut", name), s)
    assert found > 100000


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: a row is walked in chunks of 64, and a solid run is carried from one chunk into the next"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for name, box in S.LONG_BOXES.items():
            for min_byte, select in ((4, None), (1, None), (100, scene.surface_select([1, 5])), (3, scene.surface_select([0]))):
                s = scene.Surface(box, 0, min_byte, select)
                want = scene.surface_volume(vol, dims, s, labels=labels)
                assert int(want[0]["total"]) > 1000, (name, min_byte)
                _same((name, min_byte), _run(ctx, s), want)


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    host = S.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, s in S.surfaces():
            want = _check(ctx, host, ("no labels", name), s, labels=False)
            assert int(want[0]["faces"][1:].sum()) == 0
        host.set_cut(ctx, S.BOX, S.PLANE, None)
        for name, s in S.surfaces():
            _check(ctx, host, ("no labels, cut", name), s, labels=False)
        other = (S.NX + 1, S.NY, S.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, s in S.surfaces():
            _check(ctx, host, ("labels of other dimensions", name), s, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = S.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.surface_pass)
        _refused(_lib.E_STATE, ctx.surface_pass, scene.Surface(S.BOXES["texel"]))
        _refused(_lib.E_STATE, ctx.read_surface)
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Surface(dims=S.DIMS))


# ---- 3. repeats, buffers, staleness ---------------------------------------------------------------------------------------------------
def test_the_same_request_twice_gives_the_same_bytes_and_a_second_pass_carries_nothing_of_the_first(volym_lib):
    from volym_amd import scene
    host = S.scene_b()
    sel = S.selects()
    with _ctx(1) as ctx:
        host.upload(ctx)
        s = scene.Surface(S.BOXES["x 5..30"], 0, 128, sel["all"])
        first = _run(ctx, s)
        for k in range(3):
            assert S.as_bytes(_run(ctx, s)) == S.as_bytes(first), k
        _same("x 5..30", first, S.expect(host, s))
        ctx.surface_pass(scene.Surface(S.BOXES["whole"], 0, 1, sel["all"]))
        t = scene.Surface(S.BOXES["texel"], 0, 1, sel["all"])
        ctx.surface_pass(t)                                       # no read in between
        ctx.surface_faces_pass()
        got = ctx.read_surface(), ctx.read_surface_faces()
        _same("texel after whole", got, S.expect(host, t))
        assert int(got[0]["total"]) == 6 and got[1]["dir"].tolist() == [0, 1, 2, 3, 4, 5]
        ctx.surface_pass(None)
        ctx.surface_pass(scene.Surface(S.BOXES["empty"]))
        ctx.surface_faces_pass()
        _same("empty after whole", (ctx.read_surface(), ctx.read_surface_faces()), scene.empty_surface())
        ctx.surface_pass(None)                                    # NULL: the whole volume, min_byte 1, every label
        ctx.surface_faces_pass()
        _same("NULL", (ctx.read_surface(), ctx.read_surface_faces()), S.expect(host, scene.Surface(dims=S.DIMS)))


@pytest.mark.parametrize("layout", [0, 1])
def test_a_callers_buffer_gets_the_same_faces_and_too_small_a_one_is_refused_untouched(volym_lib, layout):
    from volym_amd import _lib, scene
    host = S.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx)
        s = scene.Surface(S.BOXES["rows"], 0, 128, S.selects()["mix"])
        want = S.expect(host, s)
        total = int(want[0]["total"])
        assert total > 1000
        guard = 256
        holder = torch.full((total * 8 + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.surface_pass(s)
        for capacity in (0, 1, total - 1):
            _refused(_lib.E_INVALID, ctx.surface_faces_pass, holder.data_ptr() + guard, capacity)
        _refused(_lib.E_INVALID, ctx.surface_faces_pass, holder.data_ptr() + guard + 4, total)      # misaligned
        ctx.sync()
        assert bool((holder == 0xA5).all()), "a refused faces pass wrote"
        _refused(_lib.E_STATE, ctx.read_surface_faces, total)     # nothing is in the context's own buffer yet
        ctx.surface_faces_pass(holder.data_ptr() + guard, total)
        ctx.sync()
        got = holder.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[guard + total * 8:] == 0xA5).all()
        assert got[guard:guard + total * 8].tobytes() == want[1].tobytes()
        ctx.surface_faces_pass(holder.data_ptr() + guard, total + 5)                                # more room than needed
        ctx.surface_faces_pass()                                  # and the context's own, from the same surface pass
        _same("own buffer after the caller's", (ctx.read_surface(), ctx.read_surface_faces()), want)
        assert ctx.surface_device_ptr()


def test_the_contexts_own_buffers_grow_and_then_serve_a_smaller_surface(volym_lib):
    """24^3 built like scene A (random density bytes 1..255, five labels in blocks): a small box, the whole volume, a small box again,
    each with a surface pass of its own and a faces pass into the context's own buffer.  64, then 576, then 64 rows, so the row offsets
    and their block sums grow with the face list at the second pass and are all larger than needed at the third"""
    from volym_amd import scene
    n = 24
    dims = (n, n, n)
    rng = np.random.default_rng(24)
    vol = rng.integers(1, 256, n ** 3).astype(np.uint8)
    labels = np.repeat(np.arange(n, dtype=np.uint8) // 5, n * n)              # blocks of five z planes: labels 0..4
    boxes = [((4, 4, 4), (12, 12, 12)), ((0, 0, 0), dims), ((0, 0, 0), (8, 8, 8))]
    totals, ptrs = [], []
    with _ctx(0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for box in boxes:
            s = scene.Surface(box, 0, 128)
            want = scene.surface_volume(vol, dims, s, labels=labels)
            got = _run(ctx, s)
            _same(box, got, want)
            assert got[1].tobytes() == want[1].tobytes(), box
            totals.append(int(want[0]["total"]))
            ptrs.append(ctx.surface_device_ptr())
    assert totals[0] > 100 and totals[2] > 100 and totals[1] > 8 * max(totals[0], totals[2]), totals
    assert S.rows(boxes[1]) > 256 > S.rows(boxes[0]) == S.rows(boxes[2])
    # (the face list's address has no accessor; the summary's is the one the context hands out)
    assert ptrs[2] and ptrs[2] == ptrs[1], ptrs


def test_a_faces_pass_after_an_edit_of_the_scenes_bytes_is_refused(volym_lib):
    from volym_amd import _lib, scene
    host = S.scene_a()
    s = scene.Surface(S.BOXES["whole"], 0, 128)
    with _ctx(0) as ctx:
        host.upload(ctx)
        edits = [("crop box", lambda: ctx.set_crop_box(*S.BOX)), ("clip plane", lambda: ctx.set_clip_plane(*S.PLANE)),
                 ("visibility", lambda: ctx.set_segment_visibility(scene.visibility_mask(S.HIDDEN))),
                 ("labels", lambda: ctx.set_labels(host.labels, host.dims)), ("volume", lambda: ctx.set_volume(host.vol, host.dims, 0))]
        for name, edit in edits:
            ctx.surface_pass(s)
            ctx.surface_faces_pass()
            edit()
            _refused(_lib.E_STATE, ctx.surface_faces_pass)
            ctx.surface_pass(s)                                   # a new pass describes the new scene
            ctx.surface_faces_pass()
            assert int(ctx.read_surface()["total"]) == len(ctx.read_surface_faces()) > 0, name
        # edits that change no byte of density or labels leave the pass valid: the importances, and a cut equal to the current one
        ctx.set_labels(host.labels, host.dims)
        ctx.surface_pass(s)
        ctx.set_segment_importances(host.table)
        ctx.set_crop_box(*ctx.crop_box())
        ctx.surface_faces_pass()
        assert len(ctx.read_surface_faces()) == int(ctx.read_surface()["total"])


# ---- 4. frames, shards ---------------------------------------------------------------------------------------------------------------
def _bonsai_scene(ctx):
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut())
    ctx.set_labels(labels, dims)
    ctx.set_segment_importances(CANOPY)
    return dims, vol, labels


@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_frame_is_the_same_with_and_without_surface_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        s = scene.Surface(((5, 3, 8), (60, 50, 64)), 0, 40, scene.surface_select([2, 3]))
        want = scene.surface_volume(vol, dims, s, labels=labels)
        assert int(want[0]["total"]) > 1000 and (want[0]["faces"].sum(axis=1) > 0).sum() == 2
        _same("before any update", _run(ctx, s), want)            # before any volym_update or compute pass
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.surface_pass(s)
        ctx.surface_faces_pass()
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after the surface passes"
        for k in range(3):                                        # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.surface_pass(s)
            ctx.compute_pass()
            ctx.surface_faces_pass()
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            _same(("surface", k), (ctx.read_surface(), ctx.read_surface_faces()), want)


def test_a_sharded_context_takes_the_surface_of_the_whole_volume(volym_lib):
    from volym_amd import scene
    with _ctx(0, w=160, h=96) as ctx:
        ctx.set_shard(1, 2)
        dims, vol, labels = _bonsai_scene(ctx)
        for s in (scene.Surface(dims=dims, min_byte=40), scene.Surface(((0, 10, 20), (64, 40, 50)), 0, 1, scene.surface_select([2, 4]))):
            _same("sharded", _run(ctx, s), scene.surface_volume(vol, dims, s, labels=labels))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = S.scene_a()
    whole = scene.Surface(dims=S.DIMS)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.surface_pass)                                # no volume
        _refused(_lib.E_STATE, ctx.surface_pass, whole)
        _refused(_lib.E_STATE, ctx.read_surface)                                # no pass
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        _refused(_lib.E_STATE, ctx.read_surface_faces, 0)
        assert ctx.surface_device_ptr() is None
        host.upload(ctx, labels=False)
        _refused(_lib.E_STATE, ctx.read_surface)                                # a volume, but still no pass
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        ctx.surface_pass(whole)                                                 # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(S.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.surface_pass, scene.Surface(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(S.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.surface_pass, scene.Surface((tuple(lo), tuple(hi))))
        _refused(_lib.E_INVALID, ctx.surface_pass, whole.replace(flags=2))
        _refused(_lib.E_INVALID, ctx.surface_pass, whole.replace(flags=_lib.SURFACE_UNCUT | 4))
        _refused(_lib.E_INVALID, ctx.surface_pass, whole.replace(min_byte=0))
        _refused(_lib.E_INVALID, ctx.surface_pass, whole.replace(min_byte=256))
        assert volym_lib.volym_surface_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_surface(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_surface(None, None) == _lib.E_INVALID
        assert volym_lib.volym_surface_faces_pass(None, None, 0) == _lib.E_INVALID
        assert volym_lib.volym_read_surface_faces(None, None, 0) == _lib.E_INVALID
        assert volym_lib.volym_surface_device_ptr(None) is None
        # a refused pass leaves the latest result usable
        ctx.surface_faces_pass()
        _same("after the refusals", (ctx.read_surface(), ctx.read_surface_faces()), S.expect(host, whole, labels=False))
        _refused(_lib.E_INVALID, ctx.read_surface_faces, 5)                     # room for fewer records than the pass wrote
        # a new volume: the result described the old one
        ctx.set_volume(host.vol, host.dims, 0)
        _refused(_lib.E_STATE, ctx.read_surface)
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        assert ctx.surface_device_ptr() is None
        _same("after the new volume", _run(ctx, None), S.expect(host, whole, labels=False))


# ---- 6. the Python callers ----------------------------------------------------------------------------------------------------------
def test_simple_takes_the_surface_of_the_bonsai_and_writes_it(oracle, volym_lib, tmp_path):
    from tests import common
    from volym_amd import demo, mesh, scene
    n = 32
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
                {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    spacing = (0.5, 0.25, 2.0)
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        s = scene.Surface(dims=dims, min_byte=30)
        alone = lambda l, vol_now=vol: scene.surface_volume(vol_now, dims, s.replace(select=scene.surface_select([l])), labels=lab)
        rec, _ = scene.measure_volume(vol, dims, scene.Measure(dims=dims), labels=lab)
        got = d.surface(ctx, ["Canopy", 4], min_byte=30, spacing=spacing)
        assert list(got) == ["Canopy", "Pot"]
        for name, l in (("Canopy", 2), ("Pot", 4)):
            assert got[name] == scene.surface_summary(alone(l)[0], l, spacing, rec[l]), name
            assert got[name]["measured"] >= got[name]["enclosed"] > 0
        assert set(d.surface(ctx, min_byte=1)) >= {"Canopy", "Trunk", "Pot"}
        assert d.surface(ctx, ["Trunk"], min_byte=255) == {}      # no texel that dense: no faces
        summary, faces = d.surface_faces(ctx, ["Canopy", 4], min_byte=30)
        want = scene.surface_volume(vol, dims, s.replace(select=scene.surface_select([2, 4])), labels=lab)
        _same("canopy and pot together", (summary, faces), want)
        # under a crop: the surface closes along the box
        lo, hi = d.set_crop(ctx, (0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        half = d.surface(ctx, ["Canopy"], min_byte=30)["Canopy"]
        cropped = alone(2, scene.cut_volume(vol, dims, {"box": (lo, hi)}, lab))
        assert half["faces"] == [int(v) for v in cropped[0]["faces"][2]] and 0 < half["enclosed"] < got["Canopy"]["enclosed"]
        assert d.surface(ctx, ["Canopy"], min_byte=30, uncut=True, spacing=spacing)["Canopy"] == got["Canopy"]
        ctx.set_crop_box((0, 0, 0), dims)
        # the files
        only = alone(2)
        for name in ("canopy.stl", "canopy.obj"):
            out = d.export_surface(ctx, str(tmp_path / name), ["Canopy"], min_byte=30, spacing=spacing, origin=(1.0, 2.0, 3.0))
            assert out == scene.surface_summary(only[0], None, spacing) and out["enclosed"] == got["Canopy"]["enclosed"]
        only = only[1]
        normals, tri = mesh.read_stl(str(tmp_path / "canopy.stl"))
        assert len(tri) == 2 * len(only) == 2 * sum(got["Canopy"]["faces"])
        vertices, quads = scene.surface_mesh(only, spacing, (1.0, 2.0, 3.0))
        assert np.array_equal(tri[0::2], vertices[quads[:, [0, 1, 2]]].astype(np.float32))
        v, q = mesh.read_obj(str(tmp_path / "canopy.obj"))
        assert np.array_equal(v, vertices) and np.array_equal(q, quads)
        # click for the surface: the summary of the segment the pixel shows
        d.compute_pass(ctx)
        hits = 0
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (2, 2)):
            p = d.surface_at(ctx, x, y, min_byte=30)
            if p["status"] == "hit" and p["label"] is not None:
                hits += 1
                assert p["surface"] == scene.surface_summary(alone(p["label"])[0], p["label"], (1, 1, 1), rec[p["label"]])
            else:
                assert p["surface"] is None
        assert hits >= 1


# ---- 7. the workload's scale: the scan spans workgroups ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_the_lobster_of_the_teapot(volym_lib, layout):
    from tests import common
    from volym_amd import _lib, scene
    dims = (256, 256, 178)
    raw, labels_raw = common.teapot()
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    s = scene.Surface(dims=dims, min_byte=1, select=scene.surface_select([2]))        # "Lobster"
    assert S.rows(s.box) == 45568 > 100 * _lib.SURFACE_SCAN_ROWS
    want = scene.surface_volume(vol, dims, s, labels=lab)
    assert int(want[0]["total"]) > 10000
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(lab, dims)
        got = _run(ctx, s)
        _same("lobster", got, want)
        # one device pass audits another: the divergence sums against the measure pass's count
        ctx.measure_pass(None)
        rec, _ = ctx.read_measure()
        solid = int(((vol >= 1) & (lab == 2)).sum())
        for a in range(3):
            assert int(got[0]["pos"][2][a]) - int(got[0]["neg"][2][a]) == solid <= int(rec["count"][2])


# ---- 8. the offset scan's second level: more than 256 blocks of 256 rows ----------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_the_offset_scan_with_two_block_sums_per_thread(volym_lib, layout):
    """65792 rows are 257 blocks of the scan, so the one workgroup that scans the block sums owns two per thread; more than a third of
    the rows have no face (tests/test_surface_host.py), so a wrong offset lands a row's faces on another's"""
    dims, vol, labels = S.scan_scene()
    s, want = S.scan_surface()
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        _same("scan", _run(ctx, s), want)
