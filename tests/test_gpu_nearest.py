"""The nearest pass and the fill on the device (volym_nearest_pass and its reads, volym_fill_labels).

The expected results are scene.nearest_volume and scene.fill_volume, the host twins of the rules (pinned to an all-pairs minimum with
lexicographic ties, to the distance twin, to closed forms and to per-texel loops by tests/test_nearest_host.py), of the prepared
arrays the context was given and the cut state it was put in.  Every comparison is over all 4120 bytes of the summary, the whole site
map and the whole label map, and over the 4128 bytes of a fill's result and every label: the rules are integer and the ties
canonical, so there is no tolerance and nothing is left out.  After a fill the context is compared with one that was handed the edited
labels, as tests/test_gpu_relabel.py compares it.  The scenes and requests are those of tests/nearest_scenes.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import nearest_scenes as NS
from tests.test_gpu_crop_box import CANOPY, _bonsai, _ctx, _uniforms
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(what, got, want):
    if NS.as_bytes(got) == NS.as_bytes(want):
        return
    for k, name in ((1, "sites"), (2, "near labels")):
        assert got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (what, name + " [z, y, x]", len(bad), bad[:4].tolist(), got[k][got[k] != want[k]][:4].tolist(), want[k][got[k] != want[k]][:4].tolist())
    for k in ("n_solid", "n_present", "n_finite"):
        assert int(got[0][k]) == int(want[0][k]), (what, k, int(got[0][k]), int(want[0][k]))
    for k in ("cell", "cell_present"):
        bad = np.argwhere(got[0][k] != want[0][k])
        assert bad.size == 0, (what, k, bad[:4].tolist(), got[0][k][got[0][k] != want[0][k]][:4].tolist(), want[0][k][got[0][k] != want[0][k]][:4].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _read(ctx):
    return ctx.read_nearest(), ctx.read_nearest_sites(), ctx.read_nearest_labels()


def _run(ctx, d):
    """one pass and the three reads"""
    ctx.nearest_pass(d)
    return _read(ctx)


def _check(ctx, host, what, d, labels=True):
    want = NS.expect(host, d, labels)
    _same(what, _run(ctx, d), want)
    return want


# ---- 1. boxes, select tables, thresholds, weights and cuts, both scenes, both layouts -------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    """every box with rotating select tables, min_byte and the four weights before any cut; UNCUT; then a rotating subset after each
    edit of the cuts and each cut lifted, in a context that never had a view"""
    host = NS.scene_a() if which == "a" else NS.scene_b()
    finite = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.nearest_device_ptr() is None and ctx.nearest_sites_device_ptr() is None and ctx.nearest_labels_device_ptr() is None
        for turn in range(4):
            for name, d in NS.requests(0, turn):
                finite += int(_check(ctx, host, ("never cut", name), d)[0]["n_finite"])
        assert ctx.nearest_device_ptr() and ctx.nearest_sites_device_ptr() and ctx.nearest_labels_device_ptr()
        for name, d in NS.requests(NS.UNCUT)[::2]:
            _check(ctx, host, ("uncut, never cut", name), d)
        for turn, (step, box, plane, hidden) in enumerate(NS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for name, d in NS.requests(0, turn)[turn % 2::2]:
                finite += int(_check(ctx, host, (step, name), d)[0]["n_finite"])
            for name, d in NS.requests(NS.UNCUT, turn)[:3]:
                _check(ctx, host, (step, "uncut", name), d)
    assert finite > 100000


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: a row is swept in chunks of 64, and the nearest seed and its x are carried from chunk to chunk both
    ways"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    assert {b[1][0] - b[0][0] for b in NS.LONG_BOXES.values()} >= {64, 65, 97}
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for k, (name, box) in enumerate(NS.LONG_BOXES.items()):
            for min_byte, select, weight in ((4, None, (1, 1, 1)), (100, scene.surface_select([1, 5]), (4, 1, 9)), (150, scene.surface_select([2]), (64, 25, 1)),
                                             (3, scene.surface_select([0]), (1, 64, 4)))[k % 2::2]:
                d = scene.Distance(box, 0, min_byte, select, weight)
                want = scene.nearest_volume(vol, dims, d, labels=labels)
                assert int(want[0]["n_solid"]) > 100, (name, min_byte)
                _same((name, min_byte), _run(ctx, d), want)


@pytest.mark.parametrize("layout", [0, 1])
def test_the_constructed_and_the_tie_scenes(volym_lib, layout):
    """the mirrored seeds, an axis against a diagonal, the checkerboards, the full box, the empty set, the corners, the row and column
    ends, the extents of 1 and the distance tests' scenes: the twin, and the closed forms"""
    from volym_amd import scene
    with _ctx(layout) as ctx:
        for name, (dims, vol, lab, d, closed) in NS.constructed().items():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            got = _run(ctx, d)
            _same(name, got, scene.nearest_volume(vol, dims, d, labels=lab))
            NS.check_closed(name, got, closed, d)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_long_thin_volume(volym_lib, layout):
    """6 x 2049 x 5 with weight 64 on the long axis: columns of 2049 entries and the largest intermediates -- two seeds at the ends of
    the volume far apart, then noise that makes the stacks deep"""
    from volym_amd import scene
    dims = (6, 2049, 5)
    rng = np.random.default_rng(3)
    sparse = np.zeros(dims[::-1], np.uint8)
    sparse[0, 0, 0] = sparse[4, 2048, 5] = 9
    noise = np.where(rng.random(dims[::-1]) < 0.02, 200, 0).astype(np.uint8)
    lab = rng.integers(0, 256, 6 * 2049 * 5).astype(np.uint8)
    with _ctx(layout) as ctx:
        for vol in (sparse, noise):
            ctx.set_volume(vol.ravel(), dims, 0)
            ctx.set_labels(lab, dims)
            for weight in ((1, 64, 1), (64, 64, 64)):
                d = scene.Distance(None, 0, 1, None, weight, dims=dims)
                want = scene.nearest_volume(vol.ravel(), dims, d, labels=lab)
                _same(weight, _run(ctx, d), want)
        assert int(want[0]["n_finite"]) == 6 * 2049 * 5


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    host = NS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, d in NS.requests() + NS.requests(0, 1)[:4]:
            want = _check(ctx, host, ("no labels", name), d, labels=False)
            assert not want[2].any() and not want[0]["cell"][1:].any()
        host.set_cut(ctx, NS.BOX, NS.PLANE, None)
        for name, d in NS.requests(0, 2)[::2]:
            _check(ctx, host, ("no labels, cut", name), d, labels=False)
        other = (NS.NX + 1, NS.NY, NS.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, d in NS.requests(0, 3)[::2]:
            _check(ctx, host, ("labels of other dimensions", name), d, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = NS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.nearest_pass)
        _refused(_lib.E_STATE, ctx.nearest_pass, scene.Distance(NS.BOXES["whole"]))
        _refused(_lib.E_STATE, ctx.read_nearest)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Distance(dims=NS.DIMS))


# ---- 3. repeats, sub-boxes, snapshots, refusals ----------------------------------------------------------------------------------------
def test_the_same_request_three_times_gives_the_same_bytes(volym_lib):
    from volym_amd import scene
    host = NS.scene_b()
    with _ctx(1) as ctx:
        host.upload(ctx)
        d = scene.Distance(NS.BOXES["whole"], 0, 128, NS.selects()["mix"], (1, 4, 25))
        first = _run(ctx, d)
        for k in range(3):
            assert NS.as_bytes(_run(ctx, d)) == NS.as_bytes(first), k
        _same("whole", first, NS.expect(host, d))
        ctx.distance_pass(d)                                  # the distance pass's work arrays are there now, and large enough: they are borrowed
        dmap = ctx.read_distance_map()
        _same("beside a distance pass", _run(ctx, d), first)
        assert np.array_equal(ctx.read_distance_map(), dmap)   # (its map, a result, is left alone)
        assert np.array_equal(scene.nearest_d2(first[1], d.box, d.weight).astype(np.uint32), dmap)
        small = next(box for box in NS.BOXES.values() if 0 < np.prod(np.subtract(box[1], box[0])) < 50)
        t = scene.Distance(small)
        _same("a small box after the whole", _run(ctx, t), NS.expect(host, t))     # a second pass carries nothing of the first
        empty = ((3, 4, 5), (3, 9, 9))
        _same("empty after whole", _run(ctx, scene.Distance(empty)), scene.empty_nearest())
        _same("NULL", _run(ctx, None), NS.expect(host, scene.Distance(dims=NS.DIMS)))


@pytest.mark.parametrize("layout", [0, 1])
def test_the_maps_of_sub_boxes_and_single_texels(volym_lib, layout):
    from volym_amd import _lib, scene
    host = NS.scene_a()
    box = ((5, 3, 1), (30, 19, 18))
    d = scene.Distance(box, 0, 200, None, (1, 4, 9))
    (x0, y0, z0), (x1, y1, z1) = box
    w, h = x1 - x0, y1 - y0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        ctx.nearest_pass(d)
        summary, sites, near = NS.expect(host, d)
        d2 = scene.nearest_d2(sites, box, d.weight)
        assert len(np.unique(sites)) > 100 and len(np.unique(near)) == 5
        for lo, hi in ((box[0], box[1]), ((7, 4, 2), (19, 11, 9)), ((5, 3, 1), (30, 19, 2)), ((5, 3, 4), (30, 19, 9)), ((29, 18, 17), (30, 19, 18)), ((9, 5, 5), (9, 9, 9))):
            part = (slice(lo[2] - z0, hi[2] - z0), slice(lo[1] - y0, hi[1] - y0), slice(lo[0] - x0, hi[0] - x0))
            for got, want in ((ctx.read_nearest_sites((lo, hi)), sites[part]), (ctx.read_nearest_labels((lo, hi)), near[part])):
                assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (lo, hi)
        for x, y, z in ((5, 3, 1), (29, 18, 17), (17, 11, 9), (12, 4, 16)):
            s = int(sites[z - z0, y - y0, x - x0])
            want = {"at": (x0 + s % w, y0 + (s // w) % h, z0 + s // (w * h)), "d2": int(d2[z - z0, y - y0, x - x0]), "label": int(near[z - z0, y - y0, x - x0])}
            assert ctx.nearest_at(x, y, z) == want, (x, y, z)
        for t in ((4, 3, 1), (30, 3, 1), (5, 19, 1), (5, 3, 18), (5, 2, 1)):
            _refused(_lib.E_INVALID, ctx.nearest_at, *t)
        for read in (ctx.read_nearest_sites, ctx.read_nearest_labels):
            _refused(_lib.E_INVALID, read, ((4, 3, 1), (30, 19, 18)))
            _refused(_lib.E_INVALID, read, ((5, 3, 1), (31, 19, 18)))
            _refused(_lib.E_INVALID, read, ((9, 3, 1), (8, 19, 18)))
        ctx.nearest_pass(d.replace(select=np.zeros(256, np.int64)))                 # no solid texel: no site anywhere
        assert ctx.nearest_at(17, 11, 9) == {"at": None, "d2": None, "label": 0}


def test_the_reads_are_a_snapshot_and_a_new_volume_voids_it(volym_lib):
    from volym_amd import _lib, scene
    host = NS.scene_a()
    d = scene.Distance(NS.BOXES["rows"], 0, 128, None, (4, 1, 1))
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.nearest_pass)                                    # no volume
        for read in (ctx.read_nearest, ctx.read_nearest_sites, ctx.read_nearest_labels, lambda: ctx.nearest_at(0, 0, 0)):
            _refused(_lib.E_STATE, read)                                            # no pass
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_nearest)
        _refused(_lib.E_STATE, ctx.fill_labels, scene.Fill(dims=host.dims))
        want = _check(ctx, host, "before the edits", d)
        ctx.set_crop_box(*NS.BOX)                                                   # edits after the pass: the reads still give the snapshot
        ctx.set_segment_visibility(scene.visibility_mask(NS.HIDDEN))
        _same("after a crop", _read(ctx), want)
        ctx.edit_labels(scene.Relabel(dims=host.dims, to={0: 3, 1: 2, 2: 0}))
        _same("after an edit of the labels", _read(ctx), want)
        ctx.set_volume(host.vol, host.dims, 0)
        for read in (ctx.read_nearest, ctx.read_nearest_sites, ctx.read_nearest_labels, lambda: ctx.nearest_at(0, 5, 2)):
            _refused(_lib.E_STATE, read)
        _refused(_lib.E_STATE, ctx.fill_labels, scene.Fill(dims=host.dims))
        assert ctx.nearest_device_ptr() is None and ctx.nearest_sites_device_ptr() is None and ctx.nearest_labels_device_ptr() is None
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "after the new volume", d)               # (box and mask are reset)


def test_refusals_of_the_pass(volym_lib):
    from volym_amd import _lib, scene
    host = NS.scene_a()
    whole = scene.Distance(dims=NS.DIMS)
    with _ctx(0) as ctx:
        host.upload(ctx, labels=False)
        ctx.nearest_pass(whole)                                                     # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(NS.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.nearest_pass, scene.Distance(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(NS.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.nearest_pass, scene.Distance((tuple(lo), tuple(hi))))
            w = [1, 1, 1]; w[a] = 0
            _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(weight=tuple(w)))
            w[a] = 65
            _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(weight=tuple(w)))
        _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(flags=NS.INSIDE))
        _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(flags=NS.INSIDE | NS.UNCUT))
        _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(flags=4))
        _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(min_byte=0))
        _refused(_lib.E_INVALID, ctx.nearest_pass, whole.replace(min_byte=256))
        assert volym_lib.volym_nearest_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_nearest(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_nearest(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_nearest_sites(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_nearest_labels(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_nearest_sites(ctx.handle, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_nearest_labels(ctx.handle, None, None) == _lib.E_INVALID
        assert volym_lib.volym_nearest_at(None, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_nearest_at(ctx.handle, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_nearest_device_ptr(None) is None and volym_lib.volym_nearest_sites_device_ptr(None) is None
        assert volym_lib.volym_nearest_labels_device_ptr(None) is None
        _same("after the refusals", _read(ctx), NS.expect(host, whole, labels=False))      # the latest result stays usable


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
def test_a_frame_is_the_same_with_and_without_nearest_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        d = scene.Distance(((5, 3, 8), (60, 50, 64)), 0, 40, scene.surface_select([2, 3]), (1, 1, 4))
        want = scene.nearest_volume(vol, dims, d, labels=labels)
        assert int(want[0]["n_solid"]) > 1000 and int(want[0]["cell"][2]) > 1000 and int(want[0]["cell"][3]) > 1000
        _same("before any update", _run(ctx, d), want)            # before any volym_update or compute pass
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.nearest_pass(d)
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after the nearest pass"
        for k in range(3):                                        # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.nearest_pass(d)
            ctx.compute_pass()
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            _same(("nearest", k), _read(ctx), want)


# ---- 5. the fill -------------------------------------------------------------------------------------------------------------------------
def _fill(ctx, host, case, snap=None, passes=True):
    """run the pass `case` reads and the fill, compare the result with the twin's and take the twin's labels; returns the result"""
    if passes:
        ctx.nearest_pass(case.distance)
    new, want = NS.fill_expect(host, case, snap)
    got = ctx.fill_labels(case.fill)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not case.fill.flags & NS.FILL_DRY_RUN:
        host.labels = new
    return got


@pytest.mark.parametrize("layout", [0, 1])
def test_every_fill_before_any_cut(oracle, volym_lib, layout):
    host = NS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(NS.fill_cases()):
            if k:
                _hand_labels(ctx, host, original)
            got = _fill(ctx, host, case)
            assert (int(got["changed"]) == 0) == case.trivial, case.name
            if case.fill.flags & NS.FILL_DRY_RUN or case.trivial:
                assert np.array_equal(host.labels, original), case.name
            changed += int(got["changed"])
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 10000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_of_the_fills_after_each_cut(oracle, volym_lib, layout):
    host = NS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    cases = NS.fill_cases()[:8]
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(NS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in cases[step % 4::4]:
                _hand_labels(ctx, host, original)
                _fill(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_fill_into_and_out_of_a_hidden_label(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = NS.scene_a()
    uniforms = _frame_uniforms(oracle)
    seeds = scene.Distance(dims=host.dims, flags=NS.UNCUT, select=NS.table(1, 2, 3))
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [2])                             # hidden, with voxels: the seeds are read from the uncut copy
        into = NS.FillCase("into the hidden label", seeds, scene.Fill(dims=host.dims, flags=NS.FILL_UNCUT, give=NS.table(0, 4), take=NS.table(1, 2, 3)))
        got = _fill(ctx, host, into)
        assert int(got["arrived"][2]) > 500
        _look(ctx, host, ref, "filled into a hidden label", uniforms)
        out = NS.FillCase("out of the hidden label", scene.Distance(dims=host.dims, select=NS.table(1, 3)),
                          scene.Fill(dims=host.dims, flags=NS.FILL_UNCUT, give=NS.table(2), take=NS.table(1, 3), d2=(0, 9)))
        got = _fill(ctx, host, out)
        assert int(got["left"][2]) > 500
        _look(ctx, host, ref, "filled out of a hidden label", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "shown again", uniforms)
    host = NS.scene_a()
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:   # a hidden label without voxels, in a context that never cut
        host.upload(ctx)
        _hand_labels(ctx, host, np.where(host.labels == 3, 9, host.labels).astype(np.uint8))
        host.set_cut(ctx, None, None, [3])
        _hand_labels(ctx, host, np.where(host.labels == 9, 3, np.where(host.labels == 1, 0, host.labels)).astype(np.uint8))
        case = NS.FillCase("0 to 3 and 2", scene.Distance(dims=host.dims, flags=NS.UNCUT, select=NS.table(2, 3)),
                           scene.Fill(dims=host.dims, flags=NS.FILL_UNCUT, give=NS.table(0), take=NS.table(2, 3)))
        assert int(_fill(ctx, host, case)["arrived"][3]) > 200
        _look(ctx, host, ref, "moved into the hidden label", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "the label shown again", uniforms)


def test_a_snapshot_applied_twice_and_after_the_seeds_changed(oracle, volym_lib):
    from volym_amd import scene
    host = NS.scene_a()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in NS.fill_cases()}
    with _ctx(1) as ctx, Reference(1) as ref:
        host.upload(ctx)
        band = cases["0 within 2 of a seed"]
        snap = NS.expect(host, band.distance)
        first = int(_fill(ctx, host, band)["changed"])
        again = int(_fill(ctx, host, band, snap, passes=False)["changed"])         # the texels that went are no longer 0: nothing is left to give
        assert first > 1000 and again == 0
        wide = NS.FillCase("the same snapshot, a wider band", band.distance, band.fill.replace(d2=(0, 25)))
        assert int(_fill(ctx, host, wide, snap, passes=False)["changed"]) > 20      # (scene A's blocks are small: few texels of 0 lie further out)
        _look(ctx, host, ref, "one snapshot, three fills", uniforms)
        # a relabel moves the seeds' labels about: the snapshot's labels still decide, though no texel carries them where it says
        ctx.edit_labels(scene.Relabel(dims=host.dims, to={1: 2, 2: 3, 3: 1}))
        host.labels = np.array([0, 2, 3, 1, 4], np.uint8)[host.labels]
        stale = NS.FillCase("after the seeds changed", band.distance, scene.Fill(dims=host.dims, give=NS.table(0, 4), take=NS.table(1, 2, 3)))
        assert int(_fill(ctx, host, stale, snap, passes=False)["changed"]) > 1000
        _look(ctx, host, ref, "a fill by a stale snapshot", uniforms)
        assert not np.array_equal(NS.expect(host, band.distance)[2], snap[2])


@pytest.mark.parametrize("layout", [0, 1])
def test_fills_undone_and_redone(oracle, volym_lib, layout):
    from tests.test_gpu_label_history import Run
    from volym_amd import _lib, scene
    host = NS.scene_a()
    cases = [c for c in NS.fill_cases() if not c.trivial][:5]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, 64 << 20, bool(layout), ref, _frame_uniforms(oracle))
        states, edits = [host.labels.copy()], []
        for case in cases:
            old = host.labels.copy()
            edits.append(_fill(ctx, host, case))
            if not case.fill.flags & NS.FILL_DRY_RUN:
                run.twin.record(old, host.labels, box=case.fill.box)
            run.same_info(case.name)
            states.append(host.labels.copy())
        steps = run.twin.info()["undo_steps"]
        assert steps == len(cases) - 1                                  # (the dry run is no step)
        run.look("after the fills")
        for k in range(steps):
            run.swap(False, look=k == steps - 1)
        assert np.array_equal(host.labels, states[0])
        _refused(_lib.E_STATE, ctx.undo_labels)
        for k in range(steps):
            run.swap(True, look=k == steps - 1)
        assert np.array_equal(host.labels, states[-1])
        _refused(_lib.E_STATE, ctx.redo_labels)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_budget_one_record_short_gives_the_history_up(oracle, volym_lib, layout):
    from tests.test_gpu_label_history import Run
    from volym_amd import _lib, scene
    host = NS.scene_a()
    case = NS.fill_cases()[1]
    records = scene.label_chunks_changed(host.dims, host.labels, NS.fill_expect(host, case)[0], bool(layout))
    assert records > 100
    for budget, kept in ((20 * records, True), (20 * (records - 1), False)):
        host = NS.scene_a()
        with _ctx(layout) as ctx, Reference(layout) as ref:
            host.upload(ctx)
            run = Run(ctx, host, budget, bool(layout), ref, _frame_uniforms(oracle))
            old = host.labels.copy()
            _fill(ctx, host, case)                                      # returns OK either way, and its labels are right
            assert run.twin.record(old, host.labels, box=case.fill.box) == kept
            run.same_info(case.name)
            info = ctx.label_history_info()
            assert (info["undo_steps"], info["lost"], info["next_undo_records"]) == ((1, 0, records) if kept else (0, 1, 0))
            run.look(("budget", budget))
            if kept:
                run.swap(False)
            else:
                _refused(_lib.E_STATE, ctx.undo_labels)


def test_refusals_of_the_fill(volym_lib):
    from volym_amd import _lib, scene
    host = NS.scene_a()
    whole = scene.Fill(dims=host.dims, give=NS.table(0), take=NS.table(1, 2))
    inner = scene.Distance(NS.BOXES["x 5..30"], select=NS.table(1, 2))
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.fill_labels, whole)                              # no volume
        host.upload(ctx, labels=False)
        ctx.nearest_pass(inner)
        _refused(_lib.E_STATE, ctx.fill_labels, whole)                              # no labels
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        ctx.nearest_pass(inner)                                                     # (the pass above saw no labels: every near label is 0)
        _refused(_lib.E_INVALID, ctx.fill_labels, whole)                            # the box reaches outside the pass's box
        for a in range(3):
            lo, hi = list(inner.box[0]), list(inner.box[1])
            lo[a] -= 1
            _refused(_lib.E_INVALID, ctx.fill_labels, whole.replace(box=(tuple(lo), tuple(hi))))
            lo[a] += 1
            hi[a] += 1
            _refused(_lib.E_INVALID, ctx.fill_labels, whole.replace(box=(tuple(lo), tuple(hi))))
        part = whole.replace(box=inner.box)
        for bad in (dict(flags=4), dict(flags=16), dict(window=(9, 8)), dict(window=(0, 256)), dict(d2=(5, 4)), dict(box=((0, 0, 0), (NS.NX + 1, 1, 1))),
                    dict(box=((9, 0, 0), (8, 1, 1)))):
            _refused(_lib.E_INVALID, ctx.fill_labels, part.replace(**bad))
        assert volym_lib.volym_fill_labels(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_fill_labels(ctx.handle, None, None) == _lib.E_INVALID
        before = ctx.read_labels()
        assert np.array_equal(before.ravel(), host.labels)                          # no refusal wrote a label
        assert volym_lib.volym_fill_labels(ctx.handle, part.to_c(), None) == 0      # out may be NULL
        assert not np.array_equal(ctx.read_labels(), before)
        other = (NS.NX + 1, NS.NY, NS.NZ)
        ctx.set_labels(np.zeros(other[0] * other[1] * other[2], np.uint8), other)
        _refused(_lib.E_STATE, ctx.fill_labels, part)                               # labels of other dimensions
    with _ctx(0) as ctx:
        host.upload(ctx, labels_layout=1)
        _refused(_lib.E_STATE, ctx.fill_labels, whole)                              # labels in the other layout


# ---- 6. the Python callers and the CLIs --------------------------------------------------------------------------------------------------
SEGMENTS = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
            {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]


def _simple(ctx, raw, labels_raw, dims, segments):
    from volym_amd import demo, scene
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    return demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)


def test_simple_fills_three_segments_whose_margins_overlap(oracle, volym_lib):
    """the synthetic bonsai at 64^3: canopy, trunk and pot grow into the unlabelled matter at once, each texel to the nearest"""
    from tests import common
    from volym_amd import demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    with demo.GpuContext(160, 96, 0) as ctx:
        d = _simple(ctx, raw, labels_raw, dims, SEGMENTS)
        cells = d.nearest(ctx, ["Canopy", "Trunk", "Pot"], spacing=(1, 1, 2))
        request = scene.Distance(dims=dims, select=NS.table(2, 3, 4), weight=(1, 1, 4))
        summary, sites, near = scene.nearest_volume(vol, dims, request, labels=lab)
        assert cells["weights"] == (1, 1, 4) and cells["n_solid"] == int(summary["n_solid"]) > 1000
        assert {k: (c["texels"], c["fill"]) for k, c in cells["cells"].items()} == {name: (int(summary["cell"][l]), int(summary["cell_present"][l]))
                                                                                    for name, l in (("Canopy", 2), ("Trunk", 3), ("Pot", 4))}
        assert np.array_equal(ctx.read_nearest_sites(), sites) and np.array_equal(ctx.read_nearest_labels(), near)
        got = d.fill(ctx, ["Canopy", "Trunk", "Pot"], r=6, window=(1, 255), spacing=(1, 1, 2))
        want_labels, want = scene.fill_volume(vol, dims, scene.Fill(None, 0, (1, 255), NS.table(0), NS.table(2, 3, 4), (0, 36), dims=dims), lab, sites, near, request.box,
                                              request.weight)
        assert got == scene.relabel_result_dict(want) and got["changed"] > 1000 and len(got["arrived"]) == 3      # (the margins of all three took texels)
        assert np.array_equal(ctx.read_labels(), want_labels)
        # without names and without a limit: every label but those of `into` is a seed
        rest = d.fill(ctx, window=(1, 255))
        request = scene.Distance(dims=dims, select=1 - NS.table(0))
        _, sites, near = scene.nearest_volume(vol, dims, request, labels=want_labels.ravel())
        want_labels, want = scene.fill_volume(vol, dims, scene.Fill(None, 0, (1, 255), NS.table(0), 1 - NS.table(0), dims=dims), want_labels.ravel(), sites, near, request.box)
        assert rest == scene.relabel_result_dict(want) and np.array_equal(ctx.read_labels(), want_labels)
        present = vol.reshape(n, n, n) >= 1
        assert not (want_labels[present] == 0).any()                   # all the matter is handed out


@pytest.mark.parametrize("apart", [9, 10])
def test_simple_separates_two_touching_balls(oracle, volym_lib, apart):
    from tests.test_nearest_host import separate_by_twins
    dims, vol, labels = NS.two_balls(apart)
    segments = [{"id": "Segment_1", "name": "Balls", "label_value": 1, "importance": 255}]
    from volym_amd import demo, scene
    on_device, vol_dev = scene.prepare_volume(labels, dims, True).ravel(), scene.prepare_volume(vol, dims, True).ravel()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = _simple(ctx, vol, labels, dims, segments)
        pieces = d.separate(ctx, "Balls", 5)
        want, want_pieces = separate_by_twins(dims, vol_dev, on_device, 1, 5)
        assert [p["label"] for p in pieces] == want_pieces and [p["name"] for p in pieces] == ["Balls 1", "Balls 2"]
        assert np.array_equal(ctx.read_labels().ravel(), want)
        assert [p["texels"] for p in pieces] == [int((want == v).sum()) for v in want_pieces] and sum(p["texels"] for p in pieces) == int((on_device == 1).sum())
        assert d.separate(ctx, "Balls 1", 40) == []                     # no core that deep


@pytest.mark.parametrize("cli", ["python", "native"])
@pytest.mark.parametrize("args", [["--fill"], ["--fill", "Lobster:3"]])
def test_both_clis_fill(volym_lib, tmp_path, cli, args):
    """--fill on `run simple` with the built-in scene: how many texels joined which segment"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    head = [l for l in r.stdout.splitlines() if l.startswith("fill:")]
    assert len(head) == 1 and " texels joined the nearest of " in head[0], r.stdout
    changed = int(head[0].split()[1])
    took = [l for l in r.stdout.splitlines() if l.startswith("  + ")]
    assert changed > 0 and len(took) >= 1 and sum(int(l.split()[-1]) for l in took) == changed, r.stdout


def test_the_python_cli_separates(volym_lib, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png"), "--separate", "Lobster:2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    head = [l for l in r.stdout.splitlines() if l.startswith("separate:")]
    assert len(head) == 1 and " pieces" in head[0], r.stdout
