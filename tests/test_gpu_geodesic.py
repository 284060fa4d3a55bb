"""The geodesic pass and the flood on the device (volym_geodesic_pass and its reads, volym_flood_labels).

The expected results are scene.geodesic_volume and scene.flood_volume, the host twins of the rules (pinned to a per-label
breadth-first search, to a restatement of the device's schedule, to closed forms and to per-texel loops by
tests/test_geodesic_host.py), of the prepared arrays the context was given and the cut state it was put in.  Every comparison is
over all 6184 bytes of the summary and the whole key map, and over the 4128 bytes of a flood's result and every label: the rules are
integer and the keys have one fixed point, so there is no tolerance and nothing is left out.  After a flood the context is compared
with one that was handed the edited labels, as tests/test_gpu_relabel.py compares it.  The scenes and requests are those of
tests/geodesic_scenes.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import geodesic_scenes as GS
from tests.test_gpu_crop_box import CANOPY, _bonsai, _ctx, _uniforms
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(what, got, want):
    if GS.as_bytes(got) == GS.as_bytes(want):
        return
    assert got[1].shape == want[1].shape, (what, got[1].shape, want[1].shape)
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (what, "keys [z, y, x]", len(bad), bad[:4].tolist(), got[1][got[1] != want[1]][:4].tolist(), want[1][got[1] != want[1]][:4].tolist())
    for k in ("n_seed", "n_medium", "n_reached", "max_steps"):
        assert int(got[0][k]) == int(want[0][k]), (what, k, int(got[0][k]), int(want[0][k]))
    for k in ("max_at", "cell", "cell_medium", "hist"):
        bad = np.argwhere(got[0][k] != want[0][k])
        assert bad.size == 0, (what, k, bad[:4].tolist(), got[0][k][got[0][k] != want[0][k]][:4].tolist(), want[0][k][got[0][k] != want[0][k]][:4].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _read(ctx):
    return ctx.read_geodesic(), ctx.read_geodesic_map()


def _run(ctx, g):
    """one pass and the two reads"""
    ctx.geodesic_pass(g)
    return _read(ctx)


def _check(ctx, host, what, g, labels=True):
    want = GS.expect(host, g, labels)
    _same(what, _run(ctx, g), want)
    return want


# ---- 1. boxes, tables, windows, step limits and cuts, both scenes, both layouts ---------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    """every box with rotating seed and through tables, windows and step limits before any cut; UNCUT; then a rotating subset after
    each edit of the cuts and each cut lifted, in a context that never had a view"""
    host = GS.scene_a() if which == "a" else GS.scene_b()
    reached = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.geodesic_device_ptr() is None and ctx.geodesic_map_device_ptr() is None
        for turn in range(4):
            for name, g in GS.requests(0, turn):
                reached += int(_check(ctx, host, ("never cut", name), g)[0]["n_reached"])
        assert ctx.geodesic_device_ptr() and ctx.geodesic_map_device_ptr()
        for name, g in GS.requests(GS.UNCUT)[::2]:
            _check(ctx, host, ("uncut, never cut", name), g)
        for turn, (step, box, plane, hidden) in enumerate(GS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for name, g in GS.requests(0, turn)[turn % 2::2]:
                reached += int(_check(ctx, host, (step, name), g)[0]["n_reached"])
            for name, g in GS.requests(GS.UNCUT, turn)[:3]:
                _check(ctx, host, (step, "uncut", name), g)
    assert reached > 50000


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: the init and finish kernels walk a row in chunks of 64, and a chunk marks two tiles"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    assert {b[1][0] - b[0][0] for b in GS.LONG_BOXES.values()} >= {64, 65, 97}
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for k, (name, box) in enumerate(GS.LONG_BOXES.items()):
            for window, seed, through, limit in (((4, 255), GS.table(1), GS.table(0, 2, 5), 0), ((0, 255), GS.table(2), GS.table(0, 1), 7),
                                                 ((0, 255), GS.table(1, 2), GS.table(0), 0), ((1, 255), GS.table(0), GS.table(1, 2, 5), 3))[k % 2::2]:
                g = scene.Geodesic(box, 0, window, seed, through, limit)
                want = scene.geodesic_volume(vol, dims, g, labels=labels)
                assert int(want[0]["n_seed"]) > 100, (name, window)
                _same((name, window), _run(ctx, g), want)


@pytest.mark.parametrize("layout", [0, 1])
def test_the_constructed_scenes(volym_lib, layout):
    """the open box, the serpentine whole, cut and at one step, the checkerboard, the walls with a hole, the mirrored seeds on a tile
    face and inside a tile, the late shorter route, no seed, no medium, the empty box, the extents of 1, the boxes off the tiles and
    the points: the twin, and the closed forms"""
    from volym_amd import scene
    with _ctx(layout) as ctx:
        for name, (dims, vol, lab, g, closed) in GS.constructed().items():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            got = _run(ctx, g)
            _same(name, got, scene.geodesic_volume(vol, dims, g, labels=lab))
            GS.check_closed(name, got, closed)


def test_a_volume_of_64_cubed_from_one_corner_and_from_every_label(volym_lib):
    from tests import common
    from volym_amd import scene
    n = 64
    dims = (n, n, n)
    with _ctx(1) as ctx:
        ctx.set_volume(np.full(n ** 3, 9, np.uint8), dims, 0)
        g = scene.Geodesic(dims=dims, seed=GS.table(), points=[(0, 0, 0)])
        summary, keys = _run(ctx, g)
        zz, yy, xx = np.indices((n, n, n))
        assert np.array_equal(keys.astype(np.int64), (xx + yy + zz) << 8) and int(summary["max_steps"]) == 3 * (n - 1) and summary["max_at"].tolist() == [n - 1] * 3
        raw, labels_raw = common.bonsai(n)
        vol, lab = scene.prepare_volume(raw, dims, True).ravel(), scene.prepare_volume(labels_raw, dims, True).ravel()
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(lab, dims)
        want = scene.geodesic_volume(vol, dims, scene.Geodesic(dims=dims), labels=lab)
        assert int(want[0]["n_reached"]) > int(want[0]["n_seed"]) > 1000
        _same("NULL on the bonsai", _run(ctx, None), want)


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    from volym_amd import scene
    host = GS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, g in GS.requests() + GS.requests(0, 1)[:4]:
            want = _check(ctx, host, ("no labels", name), g, labels=False)
            assert not want[0]["cell"][1:].any()
        wand = scene.Geodesic(dims=host.dims, window=(80, 255), seed=GS.table(), points=[(17, 9, 11), (3, 3, 3)])
        assert int(_check(ctx, host, "no labels, points", wand, labels=False)[0]["n_reached"]) > 100
        host.set_cut(ctx, GS.BOX, GS.PLANE, None)
        for name, g in GS.requests(0, 2)[::2]:
            _check(ctx, host, ("no labels, cut", name), g, labels=False)
        other = (GS.NX + 1, GS.NY, GS.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, g in GS.requests(0, 3)[::2]:
            _check(ctx, host, ("labels of other dimensions", name), g, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = GS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.geodesic_pass)
        _refused(_lib.E_STATE, ctx.geodesic_pass, scene.Geodesic(GS.BOXES["whole"]))
        _refused(_lib.E_STATE, ctx.read_geodesic)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Geodesic(dims=GS.DIMS))


# ---- 3. repeats, sub-boxes, snapshots, refusals ----------------------------------------------------------------------------------------
def test_the_same_request_three_times_gives_the_same_bytes(volym_lib):
    from volym_amd import scene
    host = GS.scene_b()
    with _ctx(1) as ctx:
        host.upload(ctx)
        g = scene.Geodesic(GS.BOXES["whole"], 0, (60, 255), GS.table(*range(0, 256, 5)), GS.table(*range(1, 256, 2)))
        first = _run(ctx, g)
        for k in range(3):
            assert GS.as_bytes(_run(ctx, g)) == GS.as_bytes(first), k
        _same("whole", first, GS.expect(host, g))
        d = scene.Distance(GS.BOXES["whole"])
        ctx.distance_pass(d)
        ctx.nearest_pass(d)
        others = ctx.read_distance_map(), ctx.read_nearest_sites(), ctx.read_nearest_labels()
        _same("beside a distance and a nearest pass", _run(ctx, g), first)
        for got, want in zip((ctx.read_distance_map(), ctx.read_nearest_sites(), ctx.read_nearest_labels()), others):
            assert np.array_equal(got, want)                       # (the map aliases no other pass's result)
        small = next(box for box in GS.BOXES.values() if 0 < np.prod(np.subtract(box[1], box[0])) < 50)
        t = scene.Geodesic(small)
        _same("a small box after the whole", _run(ctx, t), GS.expect(host, t))     # a second pass carries nothing of the first
        empty = ((3, 4, 5), (3, 9, 9))
        _same("empty after whole", _run(ctx, scene.Geodesic(empty)), scene.empty_geodesic())
        _same("NULL", _run(ctx, None), GS.expect(host, scene.Geodesic(dims=GS.DIMS)))


@pytest.mark.parametrize("layout", [0, 1])
def test_the_map_of_sub_boxes_and_single_texels(volym_lib, layout):
    from volym_amd import _lib, scene
    host = GS.scene_a()
    box = ((5, 3, 1), (30, 19, 18))
    g = scene.Geodesic(box, 0, (70, 255), GS.table(1, 3), GS.table(0, 2, 4))
    (x0, y0, z0), (x1, y1, z1) = box
    with _ctx(layout) as ctx:
        host.upload(ctx)
        ctx.geodesic_pass(g)
        summary, keys = GS.expect(host, g)
        assert len(np.unique(keys)) > 10 and (keys == np.uint32(GS.NONE)).any()
        for lo, hi in ((box[0], box[1]), ((7, 4, 2), (19, 11, 9)), ((5, 3, 1), (30, 19, 2)), ((5, 3, 4), (30, 19, 9)), ((29, 18, 17), (30, 19, 18)), ((9, 5, 5), (9, 9, 9))):
            part = (slice(lo[2] - z0, hi[2] - z0), slice(lo[1] - y0, hi[1] - y0), slice(lo[0] - x0, hi[0] - x0))
            got, want = ctx.read_geodesic_map((lo, hi)), keys[part]
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (lo, hi)
        seen = set()
        for x, y, z in ((5, 3, 1), (29, 18, 17), (17, 11, 9), (12, 4, 16), (20, 10, 3), (8, 15, 12)):
            k = int(keys[z - z0, y - y0, x - x0])
            want = {"steps": None, "label": 0} if k == GS.NONE else {"steps": k >> 8, "label": k & 0xFF}
            assert ctx.geodesic_at(x, y, z) == want, (x, y, z)
            seen.add(want["steps"] is None)
        for t in ((4, 3, 1), (30, 3, 1), (5, 19, 1), (5, 3, 18), (5, 2, 1)):
            _refused(_lib.E_INVALID, ctx.geodesic_at, *t)
        _refused(_lib.E_INVALID, ctx.read_geodesic_map, ((4, 3, 1), (30, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_geodesic_map, ((5, 3, 1), (31, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_geodesic_map, ((9, 3, 1), (8, 19, 18)))
        ctx.geodesic_pass(g.replace(seed=GS.table()))                               # no seed: nothing reached anywhere
        assert ctx.geodesic_at(17, 11, 9) == {"steps": None, "label": 0}


def test_the_reads_are_a_snapshot_and_a_new_volume_voids_it(volym_lib):
    from volym_amd import _lib, scene
    host = GS.scene_a()
    g = scene.Geodesic(GS.BOXES["rows"], 0, (90, 255), GS.table(1, 2), GS.table(0, 3, 4))
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.geodesic_pass)                                   # no volume
        for read in (ctx.read_geodesic, ctx.read_geodesic_map, lambda: ctx.geodesic_at(0, 0, 0)):
            _refused(_lib.E_STATE, read)                                            # no pass
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_geodesic)
        _refused(_lib.E_STATE, ctx.flood_labels, scene.Flood(dims=host.dims))
        want = _check(ctx, host, "before the edits", g)
        ctx.set_crop_box(*GS.BOX)                                                   # edits after the pass: the reads still give the snapshot
        ctx.set_segment_visibility(scene.visibility_mask(GS.HIDDEN))
        _same("after a crop", _read(ctx), want)
        ctx.edit_labels(scene.Relabel(dims=host.dims, to={0: 3, 1: 2, 2: 0}))
        _same("after an edit of the labels", _read(ctx), want)
        ctx.set_volume(host.vol, host.dims, 0)
        for read in (ctx.read_geodesic, ctx.read_geodesic_map, lambda: ctx.geodesic_at(0, 5, 2)):
            _refused(_lib.E_STATE, read)
        _refused(_lib.E_STATE, ctx.flood_labels, scene.Flood(dims=host.dims))
        assert ctx.geodesic_device_ptr() is None and ctx.geodesic_map_device_ptr() is None
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "after the new volume", g)               # (box and mask are reset)


def test_refusals_of_the_pass(volym_lib):
    from volym_amd import _lib, scene
    host = GS.scene_a()
    whole = scene.Geodesic(dims=GS.DIMS)
    with _ctx(0) as ctx:
        host.upload(ctx, labels=False)
        ctx.geodesic_pass(whole)                                                    # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(GS.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.geodesic_pass, scene.Geodesic(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(GS.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.geodesic_pass, scene.Geodesic((tuple(lo), tuple(hi))))
            p = [3, 3, 3]; p[a] = GS.DIMS[a]
            _refused(_lib.E_INVALID, ctx.geodesic_pass, whole.replace(points=[tuple(p)]))
        for bad in (dict(flags=2), dict(flags=4), dict(window=(9, 8)), dict(window=(0, 256)), dict(max_steps=2 ** 24 - 2), dict(points=[(1, 1, 1)] * 65),
                    dict(box=((3, 3, 3), (9, 9, 9)), points=[(2, 3, 3)])):
            _refused(_lib.E_INVALID, ctx.geodesic_pass, whole.replace(**bad))
        assert volym_lib.volym_geodesic_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_geodesic(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_geodesic(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_geodesic_map(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_geodesic_map(ctx.handle, None, None) == _lib.E_INVALID
        assert volym_lib.volym_geodesic_at(None, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_geodesic_at(ctx.handle, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_geodesic_device_ptr(None) is None and volym_lib.volym_geodesic_map_device_ptr(None) is None
        _same("after the refusals", _read(ctx), GS.expect(host, whole, labels=False))      # the latest result stays usable


# ---- 4. frames -------------------------------------------------------------------------------------------------------------------------
def _bonsai_scene(ctx):
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut())
    ctx.set_labels(labels, dims)
    ctx.set_segment_importances(CANOPY)
    return dims, vol, labels


@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_frame_is_the_same_with_and_without_geodesic_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        g = scene.Geodesic(((5, 3, 8), (60, 50, 64)), 0, (1, 255), GS.table(2, 3), GS.table(0, 4), 12)
        want = scene.geodesic_volume(vol, dims, g, labels=labels)
        assert int(want[0]["n_seed"]) > 1000 and int(want[0]["cell_medium"][2]) > 100 and int(want[0]["cell_medium"][3]) > 100
        _same("before any update", _run(ctx, g), want)            # before any volym_update or compute pass
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.geodesic_pass(g)
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after the geodesic pass"
        for k in range(3):                                        # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.geodesic_pass(g)
            ctx.compute_pass()
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            _same(("geodesic", k), _read(ctx), want)


# ---- 5. the flood ------------------------------------------------------------------------------------------------------------------------
def _flood(ctx, host, case, snap=None, passes=True):
    """run the pass `case` reads and the flood, compare the result with the twin's and take the twin's labels; returns the result"""
    if passes:
        ctx.geodesic_pass(case.geodesic)
    new, want = GS.flood_expect(host, case, snap)
    got = ctx.flood_labels(case.flood)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not case.flood.flags & GS.FLOOD_DRY_RUN:
        host.labels = new
    return got


@pytest.mark.parametrize("layout", [0, 1])
def test_every_flood_before_any_cut(oracle, volym_lib, layout):
    host = GS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(GS.flood_cases()):
            if k:
                _hand_labels(ctx, host, original)
            got = _flood(ctx, host, case)
            assert (int(got["changed"]) == 0) == case.trivial, case.name
            if case.flood.flags & GS.FLOOD_DRY_RUN or case.trivial:
                assert np.array_equal(host.labels, original), case.name
            changed += int(got["changed"])
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 10000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_of_the_floods_after_each_cut(oracle, volym_lib, layout):
    host = GS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    cases = GS.flood_cases()[:8]
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(GS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in cases[step % 4::4]:
                _hand_labels(ctx, host, original)
                _flood(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_flood_into_and_out_of_a_hidden_label(oracle, volym_lib, layout):
    from volym_amd import scene
    host = GS.scene_a()
    uniforms = _frame_uniforms(oracle)
    seeds = scene.Geodesic(dims=host.dims, flags=GS.UNCUT, seed=GS.table(1, 2, 3), through=GS.table(0, 4))
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [2])                             # hidden, with voxels: the seeds are read from the uncut copy
        into = GS.FloodCase("into the hidden label", seeds, scene.Flood(dims=host.dims, flags=GS.FLOOD_UNCUT, give=GS.table(0, 4), take=GS.table(1, 2, 3)))
        got = _flood(ctx, host, into)
        assert int(got["arrived"][2]) > 500
        _look(ctx, host, ref, "flooded into a hidden label", uniforms)
        out = GS.FloodCase("out of the hidden label", scene.Geodesic(dims=host.dims, flags=GS.UNCUT, seed=GS.table(1, 3), through=GS.table(2)),
                           scene.Flood(dims=host.dims, flags=GS.FLOOD_UNCUT, give=GS.table(2), take=GS.table(1, 3), steps=(0, 3)))
        got = _flood(ctx, host, out)
        assert int(got["left"][2]) > 500
        _look(ctx, host, ref, "flooded out of a hidden label", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "shown again", uniforms)
    host = GS.scene_a()
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:   # a hidden label without voxels, in a context that never cut
        host.upload(ctx)
        _hand_labels(ctx, host, np.where(host.labels == 3, 9, host.labels).astype(np.uint8))
        host.set_cut(ctx, None, None, [3])
        case = GS.FloodCase("9 grows, and becomes the hidden 3", scene.Geodesic(dims=host.dims, flags=GS.UNCUT, seed=GS.table(9), through=GS.table(0)),
                            scene.Flood(dims=host.dims, flags=GS.FLOOD_UNCUT, give=GS.table(0, 9), take=GS.table(9), to={9: 3}))
        assert int(_flood(ctx, host, case)["arrived"][3]) > 200
        _look(ctx, host, ref, "moved into the hidden label", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "the label shown again", uniforms)


def test_a_snapshot_applied_three_times_and_after_the_seeds_changed(oracle, volym_lib):
    from volym_amd import scene
    host = GS.scene_a()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in GS.flood_cases()}
    with _ctx(1) as ctx, Reference(1) as ref:
        host.upload(ctx)
        band = cases["0 within 2 steps of a seed"]
        snap = GS.expect(host, band.geodesic)
        first = int(_flood(ctx, host, band)["changed"])
        again = int(_flood(ctx, host, band, snap, passes=False)["changed"])        # the texels that went are no longer 0: nothing is left to give
        assert first > 1000 and again == 0
        wide = GS.FloodCase("the same snapshot, a wider band", band.geodesic, band.flood.replace(steps=(0, 5)))
        assert int(_flood(ctx, host, wide, snap, passes=False)["changed"]) > 20
        _look(ctx, host, ref, "one snapshot, three floods", uniforms)
        # a relabel moves the seeds' labels about: the snapshot's labels still decide, though no texel carries them where it says
        ctx.edit_labels(scene.Relabel(dims=host.dims, to={1: 2, 2: 3, 3: 1}))
        host.labels = np.array([0, 2, 3, 1, 4], np.uint8)[host.labels]
        stale = GS.FloodCase("after the seeds changed", band.geodesic, scene.Flood(dims=host.dims, give=GS.table(0, 4), take=GS.table(1, 2, 3)))
        assert int(_flood(ctx, host, stale, snap, passes=False)["changed"]) > 1000
        _look(ctx, host, ref, "a flood by a stale snapshot", uniforms)
        assert not np.array_equal(GS.expect(host, band.geodesic)[1], snap[1])


@pytest.mark.parametrize("layout", [0, 1])
def test_floods_undone_and_redone(oracle, volym_lib, layout):
    from tests.test_gpu_label_history import Run
    from volym_amd import _lib
    host = GS.scene_a()
    cases = [c for c in GS.flood_cases() if not c.trivial][:9]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, 64 << 20, bool(layout), ref, _frame_uniforms(oracle))
        states = [host.labels.copy()]
        for case in cases:
            old = host.labels.copy()
            got = _flood(ctx, host, case)
            if not case.flood.flags & GS.FLOOD_DRY_RUN and int(got["changed"]):
                run.twin.record(old, host.labels, box=case.flood.box)
            run.same_info(case.name)
            states.append(host.labels.copy())
        steps = run.twin.info()["undo_steps"]
        assert 4 <= steps < len(cases)                                  # (the dry run is no step)
        run.look("after the floods")
        for k in range(steps):
            run.swap(False, look=k == steps - 1)
        assert np.array_equal(host.labels, states[0])
        _refused(_lib.E_STATE, ctx.undo_labels)
        for k in range(steps):
            run.swap(True, look=k == steps - 1)
        assert np.array_equal(host.labels, states[-1])
        _refused(_lib.E_STATE, ctx.redo_labels)


def test_refusals_of_the_flood(volym_lib):
    from volym_amd import _lib, scene
    host = GS.scene_a()
    whole = scene.Flood(dims=host.dims, give=GS.table(0), take=GS.table(1, 2))
    inner = scene.Geodesic(GS.BOXES["x 5..30"], seed=GS.table(1, 2), through=GS.table(0))
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.flood_labels, whole)                             # no volume
        host.upload(ctx, labels=False)
        ctx.geodesic_pass(inner)
        _refused(_lib.E_STATE, ctx.flood_labels, whole)                             # no labels
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        ctx.geodesic_pass(inner)                                                    # (the pass above saw no labels: it had no seed)
        _refused(_lib.E_INVALID, ctx.flood_labels, whole)                           # the box reaches outside the pass's box
        for a in range(3):
            lo, hi = list(inner.box[0]), list(inner.box[1])
            lo[a] -= 1
            _refused(_lib.E_INVALID, ctx.flood_labels, whole.replace(box=(tuple(lo), tuple(hi))))
            lo[a] += 1
            hi[a] += 1
            _refused(_lib.E_INVALID, ctx.flood_labels, whole.replace(box=(tuple(lo), tuple(hi))))
        part = whole.replace(box=inner.box)
        for bad in (dict(flags=4), dict(flags=16), dict(window=(9, 8)), dict(window=(0, 256)), dict(steps=(5, 4)), dict(box=((0, 0, 0), (GS.NX + 1, 1, 1))),
                    dict(box=((9, 0, 0), (8, 1, 1)))):
            _refused(_lib.E_INVALID, ctx.flood_labels, part.replace(**bad))
        assert volym_lib.volym_flood_labels(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_flood_labels(ctx.handle, None, None) == _lib.E_INVALID
        before = ctx.read_labels()
        assert np.array_equal(before.ravel(), host.labels)                          # no refusal wrote a label
        assert volym_lib.volym_flood_labels(ctx.handle, part.to_c(), None) == 0     # out may be NULL
        assert not np.array_equal(ctx.read_labels(), before)
        other = (GS.NX + 1, GS.NY, GS.NZ)
        ctx.set_labels(np.zeros(other[0] * other[1] * other[2], np.uint8), other)
        _refused(_lib.E_STATE, ctx.flood_labels, part)                              # labels of other dimensions
    with _ctx(0) as ctx:
        host.upload(ctx, labels_layout=1)
        _refused(_lib.E_STATE, ctx.flood_labels, whole)                             # labels in the other layout


# ---- 6. the Python callers and the CLIs --------------------------------------------------------------------------------------------------
SEGMENTS = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
            {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]


def _simple(ctx, raw, labels_raw, dims, segments):
    from volym_amd import demo, scene
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    return demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)


def test_simple_reaches_and_grows_through_the_matter_alone(oracle, volym_lib):
    """The synthetic bonsai at 64^3 with a slab of air cut through the unlabelled matter, two texels thick, and a segment on either
    side of it within 5 texels of the other's margin: the Euclidean fill hands texels across the gap, the geodesic growth does not."""
    from tests import common
    from volym_amd import demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True).copy(), scene.prepare_volume(labels_raw, dims, True).copy()
    vol3, lab3 = vol.reshape(n, n, n), lab.reshape(n, n, n)
    # two new segments, 7 and 8, of matter: slabs of the volume's unlabelled matter at x = 27..28 and x = 33..34, and air between
    vol3[:, :, 27:35] = np.maximum(vol3[:, :, 27:35], 60)
    lab3[:, :, 27:35] = 0
    lab3[:, :, 27:29], lab3[:, :, 33:35] = 7, 8
    vol3[:, :, 30:32] = 0
    segments = SEGMENTS + [{"id": "Segment_7", "name": "Left", "label_value": 7, "importance": 0}, {"id": "Segment_8", "name": "Right", "label_value": 8, "importance": 0}]
    raw2, labels2 = np.ascontiguousarray(vol3[:, ::-1, :]).ravel(), np.ascontiguousarray(lab3[:, ::-1, :]).ravel()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = _simple(ctx, raw2, labels2, dims, segments)
        cells = d.reach(ctx, ["Left", "Right"], r=5)
        assert np.array_equal(ctx.read_labels().ravel(), lab.ravel())
        g = scene.Geodesic(dims=dims, seed=GS.table(7, 8), through=GS.table(0), max_steps=5)
        summary, keys = scene.geodesic_volume(vol, dims, g, labels=lab)
        assert cells == scene.geodesic_summary(summary, {7: "Left", 8: "Right"}) and 1 <= cells["max_steps"] <= 5 and cells["cells"]["Left"]["grown"] > 1000
        assert np.array_equal(ctx.read_geodesic_map(), keys)
        got = d.grow_through(ctx, ["Left", "Right"], 5)
        want_labels, want = scene.flood_volume(vol, dims, scene.Flood(None, 0, (0, 255), GS.table(0), GS.table(7, 8), None, (1, 0xFFFFFFFF), dims=dims), lab, keys, g.box)
        assert got == scene.relabel_result_dict(want) and got["changed"] > 2000 and set(got["arrived"]) == {7, 8}
        after = ctx.read_labels()
        assert np.array_equal(after, want_labels)
        # 7 grew to x = 29 and leftwards, 8 to x = 32 and rightwards: neither crossed the air
        assert not (after[:, :, 30:] == 7).any() and not (after[:, :, :32] == 8).any() and (after[:, :, 29] == 7).any() and (after[:, :, 32] == 8).any()
        # the Euclidean sibling on the twins, from 7 alone with a margin of 5: it crosses the gap of two texels
        seeds = scene.Distance(dims=dims, select=GS.table(7))
        _, sites, near = scene.nearest_volume(vol, dims, seeds, labels=lab)
        filled, _ = scene.fill_volume(vol, dims, scene.Fill(None, 0, (1, 255), GS.table(0), GS.table(7), (0, 25), dims=dims), lab, sites, near, seeds.box)
        assert (filled[:, :, 32] == 7).any()
        lone, _ = scene.flood_volume(vol, dims, scene.Flood(None, 0, (0, 255), GS.table(0), GS.table(7), None, (1, 5), dims=dims), lab,
                                     scene.geodesic_volume(vol, dims, g.replace(seed=GS.table(7)), labels=lab)[1], g.box)
        assert not (lone[:, :, 30:] == 7).any()


def test_simple_wand_at_a_pixel(oracle, volym_lib):
    from tests import common
    from volym_amd import demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    with demo.GpuContext(160, 96, 0) as ctx:
        d = _simple(ctx, raw, labels_raw, dims, SEGMENTS)
        d.compute_pass(ctx)
        hit = None
        for x, y in ((80, 48), (80, 30), (70, 40), (90, 60), (80, 70), (60, 48)):
            p = d.pick(ctx, x, y)
            if p["status"] == "hit":
                hit = (x, y, p)
                break
        assert hit is not None, "no pixel of the probe shows the bonsai"
        x, y, p = hit
        over = [l for l in range(5)]
        got = d.wand_at(ctx, x, y, "Wand", 25, r=9, over=over)
        value = got["relabel"]["label"]
        assert value not in (0, 2, 3, 4) and d._segment_name(value) == "Wand"
        window = (max(p["density"] - 25, 0), min(p["density"] + 25, 255))
        assert got["relabel"]["window"] == window
        g = scene.Geodesic(dims=dims, window=window, seed=GS.table(), through=GS.table(*over), max_steps=9, points=[p["texel"]])
        _, keys = scene.geodesic_volume(vol, dims, g, labels=lab)
        want_labels, want = scene.flood_volume(vol, dims, scene.Flood(None, 0, (0, 255), GS.table(*over), None, np.full(256, value), dims=dims), lab, keys, g.box)
        res = dict(got["relabel"])
        res.pop("label"), res.pop("window")
        assert res == scene.relabel_result_dict(want) and res["changed"] >= 1
        assert np.array_equal(ctx.read_labels(), want_labels) and int(want_labels[p["texel"][2], p["texel"][1], p["texel"][0]]) == value


@pytest.mark.parametrize("cli", ["python", "native"])
@pytest.mark.parametrize("args", [["--flood"], ["--flood", "Lobster:3"]])
def test_both_clis_flood(volym_lib, tmp_path, cli, args):
    """--flood on `run simple` with the built-in scene: how many texels joined which segment"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    head = [l for l in r.stdout.splitlines() if l.startswith("flood:")]
    assert len(head) == 1 and " texels joined " in head[0], r.stdout
    changed = int(head[0].split()[1])
    took = [l for l in r.stdout.splitlines() if l.startswith("  + ")]
    assert changed > 0 and len(took) >= 1 and sum(int(l.split()[-1]) for l in took) == changed, r.stdout


def test_the_python_cli_has_a_wand(volym_lib, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png"), "--wand-at", "80,45:Wand:40:6"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    head = [l for l in r.stdout.splitlines() if l.startswith("wand:")]
    assert len(head) == 1, r.stdout
