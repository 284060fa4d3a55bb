"""The distance pass on the device (volym_distance_pass and its reads).

The expected result is scene.distance_volume, the host twin of the rule (pinned to a brute-force all-pairs minimum, to scipy and to
closed forms by tests/test_distance_host.py), of the prepared arrays the context was given and the cut state it was put in.  Every
comparison is over all 6184 bytes of the summary and the whole map: the rule is integer and the ties canonical, so there is no
tolerance and nothing is left out.  The scenes and requests are those of tests/distance_scenes.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import distance_scenes as DS
from tests.test_gpu_crop_box import CANOPY, _bonsai, _uniforms, _ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(what, got, want):
    if DS.as_bytes(got) == DS.as_bytes(want):
        return
    assert got[1].shape == want[1].shape, (what, "map", got[1].shape, want[1].shape)
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (what, "map [z, y, x]", len(bad), bad[:4].tolist(), got[1][got[1] != want[1]][:4].tolist(), want[1][got[1] != want[1]][:4].tolist())
    for k in ("n_solid", "n_present", "n_finite", "max_d2"):
        assert int(got[0][k]) == int(want[0][k]), (what, k, int(got[0][k]), int(want[0][k]))
    assert got[0]["max_at"].tolist() == want[0]["max_at"].tolist(), (what, "max_at", got[0]["max_at"].tolist(), want[0]["max_at"].tolist())
    for k in ("near_d2", "near_at", "hist"):
        bad = np.argwhere(got[0][k] != want[0][k])
        assert bad.size == 0, (what, k, bad[:4].tolist(), got[0][k][got[0][k] != want[0][k]][:4].tolist(), want[0][k][got[0][k] != want[0][k]][:4].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _run(ctx, d):
    """one pass and the two reads"""
    ctx.distance_pass(d)
    return ctx.read_distance(), ctx.read_distance_map()


def _check(ctx, host, what, d, labels=True):
    want = DS.expect(host, d, labels)
    _same(what, _run(ctx, d), want)
    return want


def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


# ---- 1. boxes, select tables, thresholds, weights, flags and cuts, both scenes, both layouts ------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    """every box with rotating select tables, min_byte and weights under both flag values before any cut; then a rotating subset after
    each edit, without a volym_update, in a context that never had a view; and UNCUT"""
    host = DS.scene_a() if which == "a" else DS.scene_b()
    finite = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.distance_device_ptr() is None and ctx.distance_map_device_ptr() is None
        for flags in (0, DS.INSIDE):
            for turn in range(3):
                for name, d in DS.requests(flags, turn):
                    finite += int(_check(ctx, host, ("never cut", flags, name), d)[0]["n_finite"])
        assert ctx.distance_device_ptr() and ctx.distance_map_device_ptr()
        for name, d in DS.requests(DS.UNCUT)[::2]:
            _check(ctx, host, ("uncut, never cut", name), d)
        for turn, (step, box, plane, hidden) in enumerate(DS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for name, d in DS.requests(DS.INSIDE if turn % 2 else 0, turn)[turn % 2::2]:
                finite += int(_check(ctx, host, (step, name), d)[0]["n_finite"])
            for name, d in DS.requests(DS.UNCUT | (0 if turn % 2 else DS.INSIDE), turn)[:3]:
                _check(ctx, host, (step, "uncut", name), d)
    assert finite > 100000


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: a row is swept in chunks of 64, and the nearest seed is carried from chunk to chunk both ways"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for k, (name, box) in enumerate(DS.LONG_BOXES.items()):
            for min_byte, select, flags, weight in ((4, None, 0, (1, 1, 1)), (100, scene.surface_select([1, 5]), DS.INSIDE, (4, 1, 9)),
                                                    (150, scene.surface_select([2]), 0, (64, 25, 1)), (3, scene.surface_select([0]), DS.INSIDE, (1, 64, 4)))[k % 2::2]:
                d = scene.Distance(box, flags, min_byte, select, weight)
                want = scene.distance_volume(vol, dims, d, labels=labels)
                assert int(want[0]["n_solid"]) > 100, (name, min_byte)
                _same((name, min_byte, flags), _run(ctx, d), want)


@pytest.mark.parametrize("layout", [0, 1])
def test_the_constructed_scenes(volym_lib, layout):
    """the single texel, the ball, the slabs, the empty set, the full box, the row and column ends and the squares: the twin, and the
    closed forms"""
    from volym_amd import scene
    with _ctx(layout) as ctx:
        for name, (dims, vol, lab, d, closed) in DS.constructed().items():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            got = _run(ctx, d)
            _same(name, got, scene.distance_volume(vol, dims, d, labels=lab))
            DS.check_closed(name, got, closed)


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
    with _ctx(layout) as ctx:
        for vol in (sparse, noise):
            ctx.set_volume(vol.ravel(), dims, 0)
            for flags, weight in ((0, (1, 64, 1)), (0, (64, 64, 64)), (DS.INSIDE, (25, 64, 4))):
                d = scene.Distance(None, flags, 1, None, weight, dims=dims)
                want = scene.distance_volume(vol.ravel(), dims, d)
                _same((flags, weight), _run(ctx, d), want)
        assert int(want[0]["n_finite"]) == 6 * 2049 * 5
    d = scene.Distance(None, 0, 1, None, (64, 64, 64), dims=dims)
    assert int(scene.distance_volume(sparse.ravel(), dims, d)[0]["max_d2"]) >= 64 * 1024 ** 2


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    host = DS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, d in DS.requests() + DS.requests(DS.INSIDE, 1)[:4]:
            want = _check(ctx, host, ("no labels", name), d, labels=False)
            assert (want[0]["near_d2"][1:] == DS.NONE).all()
        host.set_cut(ctx, DS.BOX, DS.PLANE, None)
        for name, d in DS.requests(0, 2)[::2]:
            _check(ctx, host, ("no labels, cut", name), d, labels=False)
        other = (DS.NX + 1, DS.NY, DS.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, d in DS.requests(DS.INSIDE)[::2]:
            _check(ctx, host, ("labels of other dimensions", name), d, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = DS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.distance_pass)
        _refused(_lib.E_STATE, ctx.distance_pass, scene.Distance(DS.BOXES["whole"]))
        _refused(_lib.E_STATE, ctx.read_distance)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Distance(dims=DS.DIMS, flags=DS.INSIDE))


# ---- 3. repeats, sub-boxes, snapshots, refusals ----------------------------------------------------------------------------------------
def test_the_same_request_three_times_gives_the_same_bytes(volym_lib):
    from volym_amd import scene
    host = DS.scene_b()
    with _ctx(1) as ctx:
        host.upload(ctx)
        for flags in (0, DS.INSIDE):
            d = scene.Distance(DS.BOXES["whole"], flags, 128, DS.selects()["mix"], (1, 4, 25))
            first = _run(ctx, d)
            for k in range(3):
                assert DS.as_bytes(_run(ctx, d)) == DS.as_bytes(first), (flags, k)
            _same("whole", first, DS.expect(host, d))
        small = next(box for box in DS.BOXES.values() if 0 < np.prod(np.subtract(box[1], box[0])) < 50)
        t = scene.Distance(small)
        _same("a small box after the whole", _run(ctx, t), DS.expect(host, t))     # a second pass carries nothing of the first
        empty = ((3, 4, 5), (3, 9, 9))
        _same("empty after whole", _run(ctx, scene.Distance(empty)), scene.empty_distance())
        _same("NULL", _run(ctx, None), DS.expect(host, scene.Distance(dims=DS.DIMS)))


@pytest.mark.parametrize("layout", [0, 1])
def test_the_map_of_sub_boxes_and_of_single_texels(volym_lib, layout):
    from volym_amd import _lib, scene
    host = DS.scene_a()
    box = ((5, 3, 1), (30, 19, 18))
    assert all(h <= n for h, n in zip(box[1], DS.DIMS))
    d = scene.Distance(box, 0, 200, None, (1, 4, 9))
    (x0, y0, z0), (x1, y1, z1) = box
    with _ctx(layout) as ctx:
        host.upload(ctx)
        ctx.distance_pass(d)
        summary, dmap = DS.expect(host, d)
        assert len(np.unique(dmap)) > 8                      # (the map is no constant)
        for lo, hi in ((box[0], box[1]), ((7, 4, 2), (19, 11, 9)), ((5, 3, 1), (30, 19, 2)), ((29, 18, 17), (30, 19, 18)), ((9, 5, 5), (9, 9, 9))):
            want = dmap[lo[2] - z0:hi[2] - z0, lo[1] - y0:hi[1] - y0, lo[0] - x0:hi[0] - x0]
            got = ctx.read_distance_map((lo, hi))
            assert got.shape == want.shape and np.array_equal(got, want), (lo, hi)
        for x, y, z in ((5, 3, 1), (29, 18, 17), (17, 11, 9), tuple(int(v) for v in summary["max_at"])):
            assert ctx.distance_at(x, y, z) == int(dmap[z - z0, y - y0, x - x0])
        assert ctx.distance_at(*summary["max_at"].tolist()) == int(summary["max_d2"])
        for t in ((4, 3, 1), (30, 3, 1), (5, 19, 1), (5, 3, 18), (5, 2, 1)):
            _refused(_lib.E_INVALID, ctx.distance_at, *t)
        _refused(_lib.E_INVALID, ctx.read_distance_map, ((4, 3, 1), (30, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_distance_map, ((5, 3, 1), (31, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_distance_map, ((9, 3, 1), (8, 19, 18)))


def test_the_reads_are_a_snapshot_and_a_new_volume_voids_it(volym_lib):
    from volym_amd import _lib, scene
    host = DS.scene_a()
    d = scene.Distance(DS.BOXES["rows"], DS.INSIDE, 128, None, (4, 1, 1))
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.distance_pass)                                   # no volume
        for read in (ctx.read_distance, ctx.read_distance_map, lambda: ctx.distance_at(0, 0, 0)):
            _refused(_lib.E_STATE, read)                                            # no pass
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_distance)
        want = _check(ctx, host, "before the edits", d)
        ctx.set_crop_box(*DS.BOX)                                                   # edits after the pass: the reads still give the snapshot
        ctx.set_segment_visibility(scene.visibility_mask(DS.HIDDEN))
        _same("after a crop", (ctx.read_distance(), ctx.read_distance_map()), want)
        ctx.set_volume(host.vol, host.dims, 0)
        for read in (ctx.read_distance, ctx.read_distance_map, lambda: ctx.distance_at(0, 5, 2)):
            _refused(_lib.E_STATE, read)
        assert ctx.distance_device_ptr() is None and ctx.distance_map_device_ptr() is None
        _check(ctx, host, "after the new volume", d)               # (box and mask are reset; the labels stay)


def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = DS.scene_a()
    whole = scene.Distance(dims=DS.DIMS)
    with _ctx(0) as ctx:
        host.upload(ctx, labels=False)
        ctx.distance_pass(whole)                                                    # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(DS.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.distance_pass, scene.Distance(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(DS.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.distance_pass, scene.Distance((tuple(lo), tuple(hi))))
            w = [1, 1, 1]; w[a] = 0
            _refused(_lib.E_INVALID, ctx.distance_pass, whole.replace(weight=tuple(w)))
            w[a] = 65
            _refused(_lib.E_INVALID, ctx.distance_pass, whole.replace(weight=tuple(w)))
        _refused(_lib.E_INVALID, ctx.distance_pass, whole.replace(flags=4))
        _refused(_lib.E_INVALID, ctx.distance_pass, whole.replace(min_byte=0))
        _refused(_lib.E_INVALID, ctx.distance_pass, whole.replace(min_byte=256))
        assert volym_lib.volym_distance_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_distance(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_distance(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_distance_map(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_distance_at(None, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_distance_at(ctx.handle, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_distance_device_ptr(None) is None and volym_lib.volym_distance_map_device_ptr(None) is None
        _same("after the refusals", (ctx.read_distance(), ctx.read_distance_map()), DS.expect(host, whole, labels=False))      # the latest result stays usable


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
def test_a_frame_is_the_same_with_and_without_distance_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        d = scene.Distance(((5, 3, 8), (60, 50, 64)), DS.INSIDE, 40, scene.surface_select([2, 3]), (1, 1, 4))
        want = scene.distance_volume(vol, dims, d, labels=labels)
        assert int(want[0]["n_solid"]) > 1000 and int(want[0]["max_d2"]) > 4
        _same("before any update", _run(ctx, d), want)            # before any volym_update or compute pass
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.distance_pass(d)
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after the distance pass"
        for k in range(3):                                        # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.distance_pass(d)
            ctx.compute_pass()
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            _same(("distance", k), (ctx.read_distance(), ctx.read_distance_map()), want)


def test_a_sharded_context_maps_the_whole_volume(volym_lib):
    from volym_amd import scene
    with _ctx(0, w=160, h=96) as ctx:
        ctx.set_shard(1, 2)
        dims, vol, labels = _bonsai_scene(ctx)
        for d in (scene.Distance(dims=dims, min_byte=40), scene.Distance(((0, 10, 20), (64, 40, 50)), DS.INSIDE, 1, scene.surface_select([2, 4]), (4, 9, 1))):
            _same("sharded", _run(ctx, d), scene.distance_volume(vol, dims, d, labels=labels))


# ---- 5. the Python callers and the CLIs --------------------------------------------------------------------------------------------------
SEGMENTS = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
            {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]


def test_simple_measures_margins_thickness_and_clearance(oracle, volym_lib):
    from tests import common
    from volym_amd import _lib, demo, scene
    n = 32
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    twin = lambda values, flags, m=1, w=(1, 1, 1): scene.distance_volume(vol, dims, scene.Distance(None, flags, m, scene.surface_select(values), w, dims=dims), labels=lab)
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=SEGMENTS, dims=dims)
        got = d.distance(ctx, ["Canopy", 4], min_byte=30, spacing=(0.5, 0.5, 1.0))
        summary, dmap = twin([2, 4], 0, 30, (1, 1, 4))
        want = scene.distance_summary(summary, 0.5)
        assert got["weights"] == (1, 1, 4) and got["unit"] == 0.5 and got["n_solid"] == int(summary["n_solid"]) > 100
        assert {k: got[k] for k in ("n_present", "n_finite", "max_d2", "max_at", "max", "within")} == {k: want[k] for k in ("n_present", "n_finite", "max_d2", "max_at", "max", "within")}
        assert {l: (c["d2"], c["at"]) for l, c in got["clearance"].items()} == {l: (c["d2"], c["at"]) for l, c in want["clearance"].items()}
        assert got["clearance"][3]["segment"] == "Trunk" and got["clearance"][2]["d2"] == 0
        assert np.array_equal(ctx.read_distance_map(), dmap)
        # thickness: the deepest texel of the pot
        summary, dmap = twin([4], DS.INSIDE)
        t = d.thickness(ctx, "Pot")
        assert t["at"] == tuple(int(v) for v in summary["max_at"]) and t["d2"] == int(summary["max_d2"]) > 1 and t["solid"] == int(summary["n_solid"])
        assert t["radius"] == float(np.sqrt(t["d2"])) and t["thickness"] == 2.0 * t["radius"]
        assert d.thickness(ctx, "Trunk", min_byte=255) is None     # no texel that dense
        with pytest.raises(ValueError):
            d.thickness(ctx, "Pot", spacing=(1, 1, 1.5))
        # clearance: canopy to pot, both texels
        c = d.clearance(ctx, "Canopy", "Pot")
        from_a, from_b = twin([2], 0)[0], twin([4], 0)[0]
        assert c["d2"] == int(from_a["near_d2"][4]) == int(from_b["near_d2"][2]) > 0
        assert c["at_b"] == tuple(from_a["near_at"][4].tolist()) and c["at_a"] == tuple(from_b["near_at"][2].tolist())
        assert lab.reshape(n, n, n)[c["at_b"][::-1]] == 4 and lab.reshape(n, n, n)[c["at_a"][::-1]] == 2
        assert d.clearance(ctx, "Canopy", "Canopy") is None
        # the distance map of the segment under a pixel
        d.update_gpu_state(ctx, state)
        d.compute_pass(ctx)
        hits = 0
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (2, 2)):
            p = d.distance_at(ctx, x, y, inside=True)
            if p["status"] == "hit" and p["label"] is not None:
                hits += 1
                summary, dmap = twin([p["label"]], DS.INSIDE)
                tx, ty, tz = p["texel"]
                assert p["distance"]["d2_here"] == int(dmap[tz, ty, tx]) and p["distance"]["max_d2"] == int(summary["max_d2"]), (x, y)
            else:
                assert p["distance"] is None
        assert hits >= 1


@pytest.mark.parametrize("cli", ["python", "native"])
@pytest.mark.parametrize("args, inside", [(["--distance"], False), (["--distance", "Lobster:100", "--distance-inside"], True)])
def test_both_clis_print_the_distances(volym_lib, tmp_path, cli, args, inside):
    """--distance on `run simple` with the built-in teapot: n_solid, the deepest point and the clearance table; the Python CLI also
    writes the histogram"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    head = [l for l in r.stdout.splitlines() if l.startswith("distance:")]
    assert len(head) == 1 and " solid texels" in head[0] and "deepest (" in head[0] and ("inside" in head[0]) == inside, r.stdout
    assert int(head[0].split(" solid texels")[0].split()[-1]) > 100, head[0]
    near = [l for l in r.stdout.splitlines() if l.startswith("  nearest ")]
    assert len(near) >= (1 if inside else 2) and all(" at (" in l for l in near), r.stdout
    if cli == "python":
        doc = json.loads((tmp_path / "a_distance.json").read_text())
        assert len(doc["hist"]) == 256 and sum(doc["hist"]) == doc["n_finite"] > 0 and doc["inside"] == inside


# ---- 6. the workload's scale ---------------------------------------------------------------------------------------------------------
def test_the_canopy_of_the_bonsai_at_256(volym_lib):
    """one pass over 256^3 in the bricked layout against scipy's transform, squared (float64 is exact here: unit weights, distances
    below 2^26); the summary from the twin's own accounting of that map.  Without scipy, the twin itself."""
    from volym_amd import scene
    dims, vol, lab = _bonsai(256)
    d = scene.Distance(dims=dims, select=scene.surface_select([2]))
    try:
        from scipy import ndimage
    except ImportError:
        want = scene.distance_volume(vol, dims, d, labels=lab)
    else:
        b, l = vol.reshape(256, 256, 256), lab.reshape(256, 256, 256)
        solid = (b >= 1) & (l == 2)
        dmap = np.rint(ndimage.distance_transform_edt(~solid) ** 2).astype(np.uint32)
        want = scene.distance_map_summary(dmap, b, l, d), dmap
    assert int(want[0]["n_solid"]) > 1000000 and int(want[0]["max_d2"]) > 100 ** 2
    with _ctx(1) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(lab, dims)
        _same("canopy", _run(ctx, d), want)
