"""The cost pass and the spread on the device (volym_cost_pass and its reads, volym_spread_labels).

The expected results are scene.cost_volume and scene.spread_volume, the host twins of the rules (pinned to a heap-based search per
label, to a restatement of the device's schedule, to closed forms and to per-texel loops by tests/test_cost_host.py), of the prepared
arrays the context was given and the cut state it was put in.  Every comparison is over all 6184 bytes of the summary and the whole
key map, and over the 4128 bytes of a spread's result and every label: the rules are integer and the keys have one fixed point, so
there is no tolerance and nothing is left out.  After a spread the context is compared with one that was handed the edited labels, as
tests/test_gpu_relabel.py compares it.  The scenes and requests are those of tests/cost_scenes.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cost_scenes as CS
from tests import geodesic_scenes as GS
from tests.test_gpu_crop_box import CANOPY, _bonsai, _ctx, _uniforms
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(what, got, want):
    if CS.as_bytes(got) == CS.as_bytes(want):
        return
    assert got[1].shape == want[1].shape, (what, got[1].shape, want[1].shape)
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (what, "keys [z, y, x]", len(bad), bad[:4].tolist(), got[1][got[1] != want[1]][:4].tolist(), want[1][got[1] != want[1]][:4].tolist())
    for k in ("n_seed", "n_medium", "n_reached", "max_cost"):
        assert int(got[0][k]) == int(want[0][k]), (what, k, int(got[0][k]), int(want[0][k]))
    for k in ("max_at", "cell", "cell_medium", "hist"):
        bad = np.argwhere(got[0][k] != want[0][k])
        assert bad.size == 0, (what, k, bad[:4].tolist(), got[0][k][got[0][k] != want[0][k]][:4].tolist(), want[0][k][got[0][k] != want[0][k]][:4].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _read(ctx):
    return ctx.read_cost(), ctx.read_cost_map()


def _run(ctx, c):
    """one pass and the two reads"""
    ctx.cost_pass(c)
    return _read(ctx)


def _check(ctx, host, what, c, labels=True):
    want = CS.expect(host, c, labels)
    _same(what, _run(ctx, c), want)
    return want


# ---- 1. boxes, tables, windows, weights, limits and cuts, both scenes, both layouts -----------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    """every box with rotating tables, windows, weights and limits before any cut; UNCUT; then a rotating subset after each edit of the
    cuts and each cut lifted, in a context that never had a view"""
    host = CS.scene_a() if which == "a" else CS.scene_b()
    reached = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.cost_device_ptr() is None and ctx.cost_map_device_ptr() is None
        for turn in range(3):
            for name, c in CS.requests(0, turn):
                reached += int(_check(ctx, host, ("never cut", name), c)[0]["n_reached"])
        assert ctx.cost_device_ptr() and ctx.cost_map_device_ptr()
        for name, c in CS.requests(CS.UNCUT)[::2]:
            _check(ctx, host, ("uncut, never cut", name), c)
        for turn, (step, box, plane, hidden) in enumerate(CS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for name, c in CS.requests(0, turn)[turn % 2::2]:
                reached += int(_check(ctx, host, (step, name), c)[0]["n_reached"])
            for name, c in CS.requests(CS.UNCUT, turn)[:3]:
                _check(ctx, host, (step, "uncut", name), c)
    assert reached > 50000


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: the init and finish kernels walk a row in chunks of 64, and a chunk marks two tiles"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    assert {b[1][0] - b[0][0] for b in CS.LONG_BOXES.values()} >= {64, 65, 97}
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for k, (name, box) in enumerate(CS.LONG_BOXES.items()):
            for window, seed, through, weights in (((4, 255), CS.table(1), CS.table(0, 2, 5), (1, 6, 0)), ((0, 255), CS.table(2), CS.table(0, 1), (2, 30, 900)),
                                                   ((0, 255), CS.table(1, 2), CS.table(0), (3, 0, 0)), ((1, 255), CS.table(0), CS.table(1, 2, 5), (1, 255, 5000)))[k % 2::2]:
                c = scene.Cost(box, 0, window, seed, through, *weights, hist_shift=k)
                want = scene.cost_volume(vol, dims, c, labels=labels)
                assert int(want[0]["n_seed"]) > 100, (name, window)
                _same((name, window), _run(ctx, c), want)


@pytest.mark.parametrize("layout", [0, 1])
def test_the_constructed_scenes(volym_lib, layout):
    """the ramp, the ridge with its detour and between two labels, the tile lowered again and again, the ties on a tile face and
    inside a tile, the overflow trap, the wall with a hole, no seed, no medium, the empty box, the extents of 1, the boxes off the
    tiles with and without a limit, the points: the twin, and the closed forms"""
    from volym_amd import scene
    with _ctx(layout) as ctx:
        for name, (dims, vol, lab, c, closed) in CS.constructed().items():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            got = _run(ctx, c)
            _same(name, got, scene.cost_volume(vol, dims, c, labels=lab))
            CS.check_closed(name, got, closed)


def test_unit_steps_against_the_geodesic_pass_of_the_same_context(volym_lib):
    """scene 1: with step_cost 1 and contrast_cost 0 the key map is the device's own geodesic map, byte for byte, and the summaries
    too; with step_cost 3 that map with its steps tripled.  The geodesic snapshot is left as it was."""
    from volym_amd import scene
    with _ctx(1) as ctx:
        for name, dims, vol, lab, g, closed in CS.unit_cases():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            ctx.geodesic_pass(g)
            theirs = ctx.read_geodesic(), ctx.read_geodesic_map()
            assert GS.as_bytes(theirs) == GS.as_bytes(scene.geodesic_volume(vol, dims, g, labels=lab)), name
            got = _run(ctx, CS.unit_request(g))
            assert CS.as_bytes(got) == GS.as_bytes(theirs), name
            CS.check_closed(name, got, closed)
            tripled = _run(ctx, CS.unit_request(g, 3))
            assert np.array_equal(tripled[1], CS.times(theirs[1], 3)), name
            assert GS.as_bytes((ctx.read_geodesic(), ctx.read_geodesic_map())) == GS.as_bytes(theirs), name


def test_truncated_passes_are_the_untruncated_one_cut_off(volym_lib):
    """scene 7: limits on an attained cost and between two attained costs"""
    host = CS.scene_a()
    with _ctx(0) as ctx:
        host.upload(ctx)
        for name, c, limits in CS.limit_cases(host):
            full = _check(ctx, host, (name, "no limit"), c)[1]
            for r in limits:
                got = _run(ctx, c.replace(max_cost=r))
                assert np.array_equal(got[1], CS.cut_off(full, r)), (name, r)
                _same((name, r), got, CS.expect(host, c.replace(max_cost=r)))


def test_a_volume_of_64_cubed_from_one_corner_and_from_every_label(volym_lib):
    from tests import common
    from volym_amd import scene
    n = 64
    dims = (n, n, n)
    with _ctx(1) as ctx:
        zz, yy, xx = np.indices((n, n, n))
        ramp = np.minimum(xx + yy + zz, 255).astype(np.uint8)
        ctx.set_volume(ramp.ravel(), dims, 0)
        c = scene.Cost(dims=dims, window=(0, 255), seed=CS.table(), points=[(0, 0, 0)], step=2, contrast=5)
        summary, keys = _run(ctx, c)
        assert np.array_equal(keys.astype(np.int64), (2 * (xx + yy + zz) + 5 * ramp.astype(np.int64)) << 8)
        assert int(summary["max_cost"]) == 7 * 3 * (n - 1) and summary["max_at"].tolist() == [n - 1] * 3
        raw, labels_raw = common.bonsai(n)
        vol, lab = scene.prepare_volume(raw, dims, True).ravel(), scene.prepare_volume(labels_raw, dims, True).ravel()
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(lab, dims)
        want = scene.cost_volume(vol, dims, scene.Cost(dims=dims, hist_shift=4), labels=lab)
        assert int(want[0]["n_reached"]) > int(want[0]["n_seed"]) > 1000
        _same("NULL on the bonsai", _run(ctx, None), want)


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    from volym_amd import scene
    host = CS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, c in CS.requests() + CS.requests(0, 1)[:4]:
            want = _check(ctx, host, ("no labels", name), c, labels=False)
            assert not want[0]["cell"][1:].any()
        wand = scene.Cost(dims=host.dims, window=(80, 255), seed=CS.table(), points=[(17, 9, 11), (3, 3, 3)], step=1, contrast=3)
        assert int(_check(ctx, host, "no labels, points", wand, labels=False)[0]["n_reached"]) > 100
        host.set_cut(ctx, CS.BOX, CS.PLANE, None)
        for name, c in CS.requests(0, 2)[::2]:
            _check(ctx, host, ("no labels, cut", name), c, labels=False)
        other = (CS.NX + 1, CS.NY, CS.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, c in CS.requests(0, 3)[::2]:
            _check(ctx, host, ("labels of other dimensions", name), c, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.cost_pass)
        _refused(_lib.E_STATE, ctx.cost_pass, scene.Cost(CS.BOXES["whole"]))
        _refused(_lib.E_STATE, ctx.read_cost)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Cost(dims=CS.DIMS))


# ---- 3. repeats, sub-boxes, snapshots, refusals ----------------------------------------------------------------------------------------
def test_the_same_request_three_times_and_beside_the_other_passes(volym_lib):
    from volym_amd import scene
    host = CS.scene_b()
    with _ctx(1) as ctx:
        host.upload(ctx)
        c = scene.Cost(CS.BOXES["whole"], 0, (60, 255), CS.table(*range(0, 256, 5)), CS.table(*range(1, 256, 2)), 1, 9, hist_shift=3)
        first = _run(ctx, c)
        for k in range(3):
            assert CS.as_bytes(_run(ctx, c)) == CS.as_bytes(first), k
        _same("whole", first, CS.expect(host, c))
        d = scene.Distance(CS.BOXES["whole"])
        g = scene.Geodesic(CS.BOXES["whole"], 0, (60, 255), CS.table(*range(0, 256, 5)), CS.table(*range(1, 256, 2)))
        ctx.distance_pass(d)
        ctx.nearest_pass(d)
        ctx.geodesic_pass(g)
        read_others = lambda: (ctx.read_distance_map(), ctx.read_nearest_sites(), ctx.read_nearest_labels(), ctx.read_geodesic_map(), ctx.read_geodesic())
        others = read_others()
        _same("beside a distance, a nearest and a geodesic pass", _read(ctx), first)       # they left its results alone
        _same("after them", _run(ctx, c), first)
        for got, want in zip(read_others(), others):
            assert got.tobytes() == want.tobytes()                 # (the maps alias no other pass's result)
        small = next(box for box in CS.BOXES.values() if 0 < np.prod(np.subtract(box[1], box[0])) < 50)
        t = scene.Cost(small, step=2, contrast=40)
        _same("a small box after the whole", _run(ctx, t), CS.expect(host, t))     # a second pass carries nothing of the first
        empty = ((3, 4, 5), (3, 9, 9))
        _same("empty after whole", _run(ctx, scene.Cost(empty)), scene.empty_cost())
        _same("NULL", _run(ctx, None), CS.expect(host, scene.Cost(dims=CS.DIMS, hist_shift=4)))


@pytest.mark.parametrize("layout", [0, 1])
def test_the_map_of_sub_boxes_and_single_texels(volym_lib, layout):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    box = ((5, 3, 1), (30, 19, 18))
    c = scene.Cost(box, 0, (70, 255), CS.table(1, 3), CS.table(0, 2, 4), 1, 4)
    (x0, y0, z0), (x1, y1, z1) = box
    with _ctx(layout) as ctx:
        host.upload(ctx)
        ctx.cost_pass(c)
        summary, keys = CS.expect(host, c)
        assert len(np.unique(keys)) > 10 and (keys == np.uint32(CS.NONE)).any()
        for lo, hi in ((box[0], box[1]), ((7, 4, 2), (19, 11, 9)), ((5, 3, 1), (30, 19, 2)), ((5, 3, 4), (30, 19, 9)), ((29, 18, 17), (30, 19, 18)), ((9, 5, 5), (9, 9, 9))):
            part = (slice(lo[2] - z0, hi[2] - z0), slice(lo[1] - y0, hi[1] - y0), slice(lo[0] - x0, hi[0] - x0))
            got, want = ctx.read_cost_map((lo, hi)), keys[part]
            assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (lo, hi)
        seen = set()
        for x, y, z in ((5, 3, 1), (29, 18, 17), (17, 11, 9), (12, 4, 16), (20, 10, 3), (8, 15, 12)):
            k = int(keys[z - z0, y - y0, x - x0])
            want = {"cost": None, "label": 0} if k == CS.NONE else {"cost": k >> 8, "label": k & 0xFF}
            assert ctx.cost_at(x, y, z) == want, (x, y, z)
            seen.add(want["cost"] is None)
        for t in ((4, 3, 1), (30, 3, 1), (5, 19, 1), (5, 3, 18), (5, 2, 1)):
            _refused(_lib.E_INVALID, ctx.cost_at, *t)
        _refused(_lib.E_INVALID, ctx.read_cost_map, ((4, 3, 1), (30, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_cost_map, ((5, 3, 1), (31, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_cost_map, ((9, 3, 1), (8, 19, 18)))
        ctx.cost_pass(c.replace(seed=CS.table()))                                   # no seed: nothing reached anywhere
        assert ctx.cost_at(17, 11, 9) == {"cost": None, "label": 0}


def test_the_reads_are_a_snapshot_and_a_new_volume_voids_it(volym_lib):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    c = scene.Cost(CS.BOXES["rows"], 0, (90, 255), CS.table(1, 2), CS.table(0, 3, 4), 1, 7)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.cost_pass)                                       # no volume
        for read in (ctx.read_cost, ctx.read_cost_map, lambda: ctx.cost_at(0, 0, 0)):
            _refused(_lib.E_STATE, read)                                            # no pass
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_cost)
        _refused(_lib.E_STATE, ctx.spread_labels, scene.Spread(dims=host.dims))
        want = _check(ctx, host, "before the edits", c)
        ctx.set_crop_box(*CS.BOX)                                                   # edits after the pass: the reads still give the snapshot
        ctx.set_segment_visibility(scene.visibility_mask(CS.HIDDEN))
        _same("after a crop", _read(ctx), want)
        ctx.edit_labels(scene.Relabel(dims=host.dims, to={0: 3, 1: 2, 2: 0}))
        _same("after an edit of the labels", _read(ctx), want)
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        _same("after new labels and a new table", _read(ctx), want)
        ctx.set_volume(host.vol, host.dims, 0)
        for read in (ctx.read_cost, ctx.read_cost_map, lambda: ctx.cost_at(0, 5, 2)):
            _refused(_lib.E_STATE, read)
        _refused(_lib.E_STATE, ctx.spread_labels, scene.Spread(dims=host.dims))
        assert ctx.cost_device_ptr() is None and ctx.cost_map_device_ptr() is None
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "after the new volume", c)               # (box and mask are reset)


def test_refusals_of_the_pass(volym_lib):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    whole = scene.Cost(dims=CS.DIMS)
    with _ctx(0) as ctx:
        host.upload(ctx, labels=False)
        ctx.cost_pass(whole)                                                        # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(CS.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.cost_pass, scene.Cost(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(CS.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.cost_pass, scene.Cost((tuple(lo), tuple(hi))))
            p = [3, 3, 3]; p[a] = CS.DIMS[a]
            _refused(_lib.E_INVALID, ctx.cost_pass, whole.replace(points=[tuple(p)]))
        for bad in (dict(flags=2), dict(flags=4), dict(window=(9, 8)), dict(window=(0, 256)), dict(max_cost=2 ** 24 - 2), dict(step=0), dict(step=256), dict(contrast=256),
                    dict(hist_shift=17), dict(points=[(1, 1, 1)] * 65), dict(box=((3, 3, 3), (9, 9, 9)), points=[(2, 3, 3)])):
            _refused(_lib.E_INVALID, ctx.cost_pass, whole.replace(**bad))
        assert volym_lib.volym_cost_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_cost(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_cost(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_cost_map(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_cost_map(ctx.handle, None, None) == _lib.E_INVALID
        assert volym_lib.volym_cost_at(None, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_cost_at(ctx.handle, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_cost_device_ptr(None) is None and volym_lib.volym_cost_map_device_ptr(None) is None
        _same("after the refusals", _read(ctx), CS.expect(host, whole, labels=False))      # the latest result stays usable


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
def test_a_frame_is_the_same_with_and_without_cost_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        c = scene.Cost(((5, 3, 8), (60, 50, 64)), 0, (1, 255), CS.table(3, 4), CS.table(0, 2), 1, 1, 250, hist_shift=2)
        want = scene.cost_volume(vol, dims, c, labels=labels)
        assert int(want[0]["n_seed"]) > 100 and int(want[0]["cell_medium"][3]) > 10000 and int(want[0]["n_reached"]) < int(want[0]["n_seed"]) + int(want[0]["n_medium"])
        _same("before any update", _run(ctx, c), want)            # before any volym_update or compute pass
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.cost_pass(c)
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after the cost pass"
        for k in range(3):                                        # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.cost_pass(c)
            ctx.compute_pass()
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            _same(("cost", k), _read(ctx), want)


# ---- 5. the spread -----------------------------------------------------------------------------------------------------------------------
def _spread(ctx, host, case, snap=None, passes=True):
    """run the pass `case` reads and the spread, compare the result with the twin's and take the twin's labels; returns the result"""
    if passes:
        ctx.cost_pass(case.cost)
    new, want = CS.spread_expect(host, case, snap)
    got = ctx.spread_labels(case.spread)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not case.spread.flags & CS.SPREAD_DRY_RUN:
        host.labels = new
    return got


@pytest.mark.parametrize("layout", [0, 1])
def test_every_spread_before_any_cut(oracle, volym_lib, layout):
    host = CS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(CS.spread_cases()):
            if k:
                _hand_labels(ctx, host, original)
            got = _spread(ctx, host, case)
            assert (int(got["changed"]) == 0) == case.trivial, case.name
            if case.spread.flags & CS.SPREAD_DRY_RUN or case.trivial:
                assert np.array_equal(host.labels, original), case.name
                assert np.array_equal(ctx.read_labels().ravel(), original), case.name
            changed += int(got["changed"])
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 10000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_of_the_spreads_after_each_cut(oracle, volym_lib, layout):
    host = CS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    cases = CS.spread_cases()[:8]
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(CS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in cases[step % 4::4]:
                _hand_labels(ctx, host, original)
                _spread(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_spread_into_and_out_of_a_hidden_label(oracle, volym_lib, layout):
    from volym_amd import scene
    host = CS.scene_a()
    uniforms = _frame_uniforms(oracle)
    seeds = scene.Cost(dims=host.dims, flags=CS.UNCUT, seed=CS.table(1, 2, 3), through=CS.table(0, 4), step=1, contrast=2)
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [2])                             # hidden, with voxels: the seeds are read from the uncut copy
        into = CS.SpreadCase("into the hidden label", seeds, scene.Spread(dims=host.dims, flags=CS.SPREAD_UNCUT, give=CS.table(0, 4), take=CS.table(1, 2, 3)))
        got = _spread(ctx, host, into)
        assert int(got["arrived"][2]) > 500
        _look(ctx, host, ref, "spread into a hidden label", uniforms)
        out = CS.SpreadCase("out of the hidden label", scene.Cost(dims=host.dims, flags=CS.UNCUT, seed=CS.table(1, 3), through=CS.table(2), step=1, contrast=2),
                            scene.Spread(dims=host.dims, flags=CS.SPREAD_UNCUT, give=CS.table(2), take=CS.table(1, 3), cost=(0, 150)))
        got = _spread(ctx, host, out)
        assert int(got["left"][2]) > 500
        _look(ctx, host, ref, "spread out of a hidden label", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "shown again", uniforms)


def test_a_snapshot_applied_three_times_and_after_the_seeds_changed(oracle, volym_lib):
    from volym_amd import scene
    host = CS.scene_a()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in CS.spread_cases()}
    with _ctx(1) as ctx, Reference(1) as ref:
        host.upload(ctx)
        band = cases["0 within a cost of 60"]
        snap = CS.expect(host, band.cost)
        first = int(_spread(ctx, host, band)["changed"])
        again = int(_spread(ctx, host, band, snap, passes=False)["changed"])       # the texels that went are no longer 0: nothing is left to give
        assert first > 400 and again == 0
        wide = CS.SpreadCase("the same snapshot, a wider band", band.cost, band.spread.replace(cost=(0, 200)))
        assert int(_spread(ctx, host, wide, snap, passes=False)["changed"]) > 20
        _look(ctx, host, ref, "one snapshot, three spreads", uniforms)
        # a relabel moves the seeds' labels about: the snapshot's labels still decide, though no texel carries them where it says
        ctx.edit_labels(scene.Relabel(dims=host.dims, to={1: 2, 2: 3, 3: 1}))
        host.labels = np.array([0, 2, 3, 1, 4], np.uint8)[host.labels]
        stale = CS.SpreadCase("after the seeds changed", band.cost, scene.Spread(dims=host.dims, give=CS.table(0, 4), take=CS.table(1, 2, 3)))
        assert int(_spread(ctx, host, stale, snap, passes=False)["changed"]) > 1000
        _look(ctx, host, ref, "a spread by a stale snapshot", uniforms)
        assert not np.array_equal(CS.expect(host, band.cost)[1], snap[1])
        # the flood of the same context reads its own snapshot, not this one: none yet
        from volym_amd import _lib
        _refused(_lib.E_STATE, ctx.flood_labels, scene.Flood(dims=host.dims))


@pytest.mark.parametrize("layout", [0, 1])
def test_spreads_undone_and_redone(oracle, volym_lib, layout):
    from tests.test_gpu_label_history import Run
    from volym_amd import _lib
    host = CS.scene_a()
    cases = [c for c in CS.spread_cases() if not c.trivial][:9]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, 64 << 20, bool(layout), ref, _frame_uniforms(oracle))
        states = [host.labels.copy()]
        for case in cases:
            old = host.labels.copy()
            got = _spread(ctx, host, case)
            if not case.spread.flags & CS.SPREAD_DRY_RUN and int(got["changed"]):
                run.twin.record(old, host.labels, box=case.spread.box)
            run.same_info(case.name)
            states.append(host.labels.copy())
        steps = run.twin.info()["undo_steps"]
        assert 4 <= steps < len(cases)                                  # (the dry run is no step)
        run.look("after the spreads")
        for k in range(steps):
            run.swap(False, look=k == steps - 1)
        assert np.array_equal(host.labels, states[0])
        _refused(_lib.E_STATE, ctx.undo_labels)
        for k in range(steps):
            run.swap(True, look=k == steps - 1)
        assert np.array_equal(host.labels, states[-1])
        _refused(_lib.E_STATE, ctx.redo_labels)


def test_a_session_of_a_pass_a_brush_spreads_undo_redo_and_a_flood(oracle, volym_lib):
    """a cost pass; a brush; a spread by the now stale snapshot; undo, undo, redo; a flood; a spread -- labels and label_history_info
    after each step"""
    from tests.test_gpu_label_history import Run
    from volym_amd import scene
    host = CS.scene_a()
    cases = {c.name: c for c in CS.spread_cases()}
    first, second = cases["0 and 4 to the seeds 1, 2, 3"], cases["to renames: 1 -> 9, 2 -> 3"]
    with _ctx(1) as ctx, Reference(1) as ref:
        host.upload(ctx)
        run = Run(ctx, host, 64 << 20, True, ref, _frame_uniforms(oracle))

        def labels_are(what):
            assert np.array_equal(ctx.read_labels().ravel(), host.labels), what
            run.same_info(what)

        snap = CS.expect(host, first.cost)
        ctx.cost_pass(first.cost)
        labels_are("a cost pass")                                       # (a pass is no edit)
        stroke = scene.Brush([(10, 8, 9), (14, 9, 10), (18, 10, 11)], 9, to={0: 2, 1: 2, 4: 2}, dims=host.dims)
        now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
        painted, want = scene.brush_volume(now, host.dims, stroke, host.labels, uncut=host.vol)
        old = host.labels.copy()
        assert ctx.brush_labels(stroke).tobytes() == want.tobytes() and int(want["changed"]) > 20
        host.labels = painted.ravel()
        run.twin.record(old, host.labels, box=scene.brush_box(stroke, host.dims))
        labels_are("a brush")
        old = host.labels.copy()
        assert int(_spread(ctx, host, first, snap, passes=False)["changed"]) > 1000       # the snapshot is of the labels before the brush
        run.twin.record(old, host.labels, box=first.spread.box)
        labels_are("a spread by the stale snapshot")
        run.swap(False, look=False)
        labels_are("undo")
        run.swap(False, look=False)
        labels_are("undo again")
        assert np.array_equal(host.labels, CS.scene_a().labels)
        run.swap(True, look=True)
        labels_are("redo")
        flood = GS.flood_cases()[1]
        ctx.geodesic_pass(flood.geodesic)
        new, want = GS.flood_expect(host, flood)
        old = host.labels.copy()
        assert ctx.flood_labels(flood.flood).tobytes() == want.tobytes() and int(want["changed"]) > 100
        host.labels = new
        run.twin.record(old, host.labels, box=flood.flood.box)
        labels_are("a flood")
        old = host.labels.copy()
        assert int(_spread(ctx, host, second)["changed"]) > 100
        run.twin.record(old, host.labels, box=second.spread.box)
        labels_are("a spread")
        run.look("after the session")
        assert run.twin.info()["undo_steps"] == 3


def test_refusals_of_the_spread(volym_lib):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    whole = scene.Spread(dims=host.dims, give=CS.table(0), take=CS.table(1, 2))
    inner = scene.Cost(CS.BOXES["x 5..30"], seed=CS.table(1, 2), through=CS.table(0), step=1, contrast=2)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.spread_labels, whole)                            # no volume
        host.upload(ctx, labels=False)
        ctx.cost_pass(inner)
        _refused(_lib.E_STATE, ctx.spread_labels, whole)                            # no labels
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        ctx.geodesic_pass(scene.Geodesic(dims=host.dims))                           # (a geodesic pass over the whole volume does not widen the cost pass's box)
        ctx.cost_pass(inner)                                                        # (the pass above saw no labels: it had no seed)
        _refused(_lib.E_INVALID, ctx.spread_labels, whole)                          # the box reaches outside the pass's box
        for a in range(3):
            lo, hi = list(inner.box[0]), list(inner.box[1])
            lo[a] -= 1
            _refused(_lib.E_INVALID, ctx.spread_labels, whole.replace(box=(tuple(lo), tuple(hi))))
            lo[a] += 1
            hi[a] += 1
            _refused(_lib.E_INVALID, ctx.spread_labels, whole.replace(box=(tuple(lo), tuple(hi))))
        part = whole.replace(box=inner.box)
        for bad in (dict(flags=4), dict(flags=16), dict(window=(9, 8)), dict(window=(0, 256)), dict(cost=(5, 4)), dict(box=((0, 0, 0), (CS.NX + 1, 1, 1))),
                    dict(box=((9, 0, 0), (8, 1, 1)))):
            _refused(_lib.E_INVALID, ctx.spread_labels, part.replace(**bad))
        _refused(_lib.E_INVALID, ctx.flood_labels, scene.Flood(dims=host.dims, flags=4))       # the flood goes on refusing flag 4
        assert volym_lib.volym_spread_labels(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_spread_labels(ctx.handle, None, None) == _lib.E_INVALID
        before = ctx.read_labels()
        assert np.array_equal(before.ravel(), host.labels)                          # no refusal wrote a label
        assert volym_lib.volym_spread_labels(ctx.handle, part.to_c(), None) == 0    # out may be NULL
        assert not np.array_equal(ctx.read_labels(), before)
        other = (CS.NX + 1, CS.NY, CS.NZ)
        ctx.set_labels(np.zeros(other[0] * other[1] * other[2], np.uint8), other)
        _refused(_lib.E_STATE, ctx.spread_labels, part)                             # labels of other dimensions
    with _ctx(0) as ctx:
        host.upload(ctx, labels_layout=1)
        _refused(_lib.E_STATE, ctx.spread_labels, whole)                            # labels in the other layout


# ---- 6. the Python callers and the CLIs --------------------------------------------------------------------------------------------------
SEGMENTS = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
            {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]


def _simple(ctx, raw, labels_raw, dims, segments):
    from volym_amd import demo, scene
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    return demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)


def test_simple_grows_from_seeds_to_the_density_boundary(oracle, volym_lib):
    """The synthetic bonsai at 64^3 with a slab of matter laid through it, of byte 60 up to x = 39 and of byte 140 from x = 40, and a
    segment seeded in either part, at x = 24 and at x = 44: in steps they meet halfway, at x = 34, in cost at the boundary, x = 40."""
    from tests import common
    from volym_amd import demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True).copy(), scene.prepare_volume(labels_raw, dims, True).copy()
    vol3, lab3 = vol.reshape(n, n, n), lab.reshape(n, n, n)
    vol3[20:44, 20:44, 22:40], vol3[20:44, 20:44, 40:48] = 60, 140
    lab3[20:44, 20:44, 22:48] = 0
    lab3[20:44, 20:44, 24], lab3[20:44, 20:44, 44] = 7, 8
    segments = SEGMENTS + [{"id": "Segment_7", "name": "Left", "label_value": 7, "importance": 0}, {"id": "Segment_8", "name": "Right", "label_value": 8, "importance": 0}]
    raw2, labels2 = np.ascontiguousarray(vol3[:, ::-1, :]).ravel(), np.ascontiguousarray(lab3[:, ::-1, :]).ravel()
    block = (slice(24, 40), slice(24, 40))                                           # the slab's interior in z and y
    with demo.GpuContext(160, 96, 0) as ctx:
        d = _simple(ctx, raw2, labels2, dims, segments)
        # the step count first, against its twins
        got = d.grow_through(ctx, ["Left", "Right"], None)
        g = scene.Geodesic(dims=dims, seed=CS.table(7, 8), through=CS.table(0))
        _, steps = scene.geodesic_volume(vol, dims, g, labels=lab)
        by_steps, want = scene.flood_volume(vol, dims, scene.Flood(None, 0, (0, 255), CS.table(0), CS.table(7, 8), None, (1, 0xFFFFFFFF), dims=dims), lab, steps, g.box)
        assert got == scene.relabel_result_dict(want) and np.array_equal(ctx.read_labels(), by_steps)
        d.set_labels(ctx, labels2)                                                   # the labels as they were
        assert np.array_equal(ctx.read_labels().ravel(), lab.ravel())
        cells = d.cost_reach(ctx, ["Left", "Right"], contrast=9)
        c = scene.Cost(dims=dims, seed=CS.table(7, 8), through=CS.table(0), step=1, contrast=9, hist_shift=8)
        summary, keys = scene.cost_volume(vol, dims, c, labels=lab)
        assert cells == scene.cost_summary(summary, {7: "Left", 8: "Right"}) and cells["cells"]["Left"]["grown"] > 1000 and cells["cells"]["Right"]["grown"] > 1000
        assert np.array_equal(ctx.read_cost_map(), keys)
        got = d.grow_from_seeds(ctx, ["Left", "Right"], contrast=9)
        by_cost, want = scene.spread_volume(vol, dims, scene.Spread(None, 0, (0, 255), CS.table(0), CS.table(7, 8), None, (1, 0xFFFFFFFF), dims=dims), lab, keys, c.box)
        assert got == scene.relabel_result_dict(want) and got["changed"] > 2000 and set(got["arrived"]) == {7, 8}
        assert np.array_equal(ctx.read_labels(), by_cost)
        # they differ, and as the scene says: in steps the segments meet halfway, in cost at the boundary of the densities
        assert not np.array_equal(by_steps, by_cost)
        assert (by_steps[block][:, :, 25:34] == 7).all() and (by_steps[block][:, :, 35:44] == 8).all()
        assert (by_cost[block][:, :, 25:40] == 7).all() and (by_cost[block][:, :, 40:44] == 8).all()


def test_simple_smart_wand_at_a_pixel(oracle, volym_lib):
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
        got = d.smart_wand_at(ctx, x, y, "Wand", 4, 120, over=over)
        value = got["relabel"]["label"]
        assert value not in (0, 2, 3, 4) and d._segment_name(value) == "Wand"
        c = scene.Cost(dims=dims, window=(1, 255), seed=CS.table(), through=CS.table(*over), step=1, contrast=4, max_cost=120, points=[p["texel"]])
        _, keys = scene.cost_volume(vol, dims, c, labels=lab)
        want_labels, want = scene.spread_volume(vol, dims, scene.Spread(None, 0, (0, 255), CS.table(*over), None, np.full(256, value), dims=dims), lab, keys, c.box)
        res = dict(got["relabel"])
        res.pop("label")
        assert res == scene.relabel_result_dict(want) and res["changed"] >= 1
        assert np.array_equal(ctx.read_labels(), want_labels) and int(want_labels[p["texel"][2], p["texel"][1], p["texel"][0]]) == value


@pytest.mark.parametrize("cli", ["python", "native"])
@pytest.mark.parametrize("args", [["--grow-from-seeds", "Lobster"], ["--grow-from-seeds", "Lobster:12:5000"]])
def test_both_clis_grow_from_seeds(volym_lib, tmp_path, cli, args):
    """--grow-from-seeds on `run simple` with the built-in scene: how many texels joined which segment"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    head = [l for l in r.stdout.splitlines() if l.startswith("grow from seeds:")]
    assert len(head) == 1 and " texels joined " in head[0], r.stdout
    changed = int(head[0].split()[3])
    took = [l for l in r.stdout.splitlines() if l.startswith("  + ")]
    assert changed > 0 and len(took) >= 1 and sum(int(l.split()[-1]) for l in took) == changed, r.stdout


def test_both_clis_grow_the_same_texels(volym_lib, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    heads = []
    for cmd in ([sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")],
                [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]):
        r = subprocess.run(cmd + ["--grow-from-seeds", "Lobster:12:5000"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
        lines = [l.split() for l in r.stdout.splitlines() if l.startswith("grow from seeds:") or l.startswith("  + ")]
        heads.append([(l[-2].rstrip(":"), l[-1]) if l[0] == "+" else l[3] for l in lines])      # the texels in all, then (label, texels) per segment
    assert heads[0] == heads[1] and len(heads[0]) >= 2, heads


def test_the_python_cli_has_a_smart_wand(volym_lib, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png"), "--smart-wand-at", "80,45:Wand:4:200"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    head = [l for l in r.stdout.splitlines() if l.startswith("smart wand:")]
    assert len(head) == 1, r.stdout
