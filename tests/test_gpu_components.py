"""The components pass on the device (volym_components_pass and its reads).

The expected result is scene.components_volume, the host twin of the rule (pinned to a plain flood fill and to closed forms by
tests/test_components_host.py), of the prepared arrays the context was given and the cut state it was put in.  Every comparison is over
all 2072 bytes of the summary, every record of the table and the whole id volume: the rule is integer and the numbering canonical, so
there is no tolerance and nothing is left out.  The scenes and requests are those of tests/components_scenes.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import components_scenes as CS
from tests.test_gpu_crop_box import CANOPY, _bonsai, _uniforms, _ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(what, got, want):
    if CS.as_bytes(got) == CS.as_bytes(want):
        return
    for k in ("n_components", "n_solid", "recorded"):
        assert int(got[0][k]) == int(want[0][k]), (what, k, int(got[0][k]), int(want[0][k]))
    bad = np.flatnonzero(got[0]["per_label"] != want[0]["per_label"])
    assert bad.size == 0, (what, "per_label", bad[:6].tolist())
    assert got[2].shape == want[2].shape, (what, "ids", got[2].shape, want[2].shape)
    bad = np.argwhere(got[2] != want[2])
    assert bad.size == 0, (what, "ids [z, y, x]", len(bad), bad[:4].tolist(), got[2][got[2] != want[2]][:4].tolist(), want[2][got[2] != want[2]][:4].tolist())
    assert len(got[1]) == len(want[1]), (what, "records", len(got[1]), len(want[1]))
    bad = np.flatnonzero(got[1] != want[1])
    assert bad.size == 0, (what, "records", bad[:6].tolist(), got[1][bad[:3]].tolist(), want[1][bad[:3]].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _run(ctx, c):
    """one pass and the three reads"""
    ctx.components_pass(c)
    summary = ctx.read_components()
    return summary, ctx.read_component_table(summary["recorded"]), ctx.read_component_ids()


def _check(ctx, host, what, c, labels=True):
    want = CS.expect(host, c, labels)
    _same(what, _run(ctx, c), want)
    return want


def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


# ---- 1. boxes, select tables, thresholds, flags and cuts, both scenes, both layouts ---------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    """every box x select x min_byte with and without SPLIT_LABELS before any cut; then after each edit, without a volym_update, in a
    context that never had a view"""
    host = CS.scene_a() if which == "a" else CS.scene_b()
    found = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.components_device_ptr() is None and ctx.component_ids_device_ptr() is None and ctx.component_table_device_ptr() is None
        for flags in (0, CS.SPLIT):
            for name, c in CS.every_request(flags):
                found += int(_check(ctx, host, ("never cut", flags, name), c)[0]["n_components"])
        assert ctx.components_device_ptr() and ctx.component_ids_device_ptr() and ctx.component_table_device_ptr()
        for name, c in CS.requests(CS.UNCUT):
            _check(ctx, host, ("uncut, never cut", name), c)
        for step, box, plane, hidden in CS.CUTS:
            host.set_cut(ctx, box, plane, hidden)
            for name, c in CS.requests():
                found += int(_check(ctx, host, (step, name), c)[0]["n_components"])
            for name, c in CS.requests(CS.UNCUT | CS.SPLIT)[:4]:
                _check(ctx, host, (step, "uncut, split", name), c)
    assert found > 10000


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: a row is walked in chunks of 64, and a run is carried from one chunk into the next"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for name, box in CS.LONG_BOXES.items():
            for min_byte, select, flags in ((4, None, 0), (1, None, CS.SPLIT), (100, scene.surface_select([1, 5]), 0), (3, scene.surface_select([0]), 0)):
                c = scene.Components(box, flags, min_byte, select)
                want = scene.components_volume(vol, dims, c, labels=labels)
                assert int(want[0]["n_solid"]) > 1000, (name, min_byte)
                _same((name, min_byte, flags), _run(ctx, c), want)


@pytest.mark.parametrize("layout", [0, 1])
def test_the_constructed_scenes(volym_lib, layout):
    """the serpentine, the combs, the checkerboard, the slabs, the label blocks and the piece the box cuts: the twin, and the closed forms"""
    with _ctx(layout) as ctx:
        for name, (dims, vol, lab, c, closed) in CS.constructed().items():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            from volym_amd import scene
            got = _run(ctx, c)
            _same(name, got, scene.components_volume(vol, dims, c, labels=lab))
            assert int(got[0]["n_components"]) == closed["n_components"] and int(got[0]["n_solid"]) == closed["n_solid"], name
            assert got[1]["count"].tolist() == closed["counts"], name
            if "open" in closed:
                assert got[1]["flags"].tolist() == closed["open"], name


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    host = CS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, c in CS.requests() + CS.requests(CS.SPLIT)[:3]:
            want = _check(ctx, host, ("no labels", name), c, labels=False)
            assert int(want[0]["per_label"][1:].sum()) == 0
        host.set_cut(ctx, CS.BOX, CS.PLANE, None)
        for name, c in CS.requests():
            _check(ctx, host, ("no labels, cut", name), c, labels=False)
        other = (CS.NX + 1, CS.NY, CS.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, c in CS.requests(CS.SPLIT):
            _check(ctx, host, ("labels of other dimensions", name), c, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.components_pass)
        _refused(_lib.E_STATE, ctx.components_pass, scene.Components(CS.BOXES["texel"]))
        _refused(_lib.E_STATE, ctx.read_components)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Components(dims=CS.DIMS, flags=CS.SPLIT))


# ---- 3. capacity, repeats, sub-boxes, snapshots -------------------------------------------------------------------------------------
class _DeviceBytes:
    """`n` bytes of device memory at `ptr` for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("min_byte, at_least", [(128, 200), (200, 1000)])
def test_the_table_keeps_max_components_records_and_writes_nothing_behind_them(volym_lib, layout, min_byte, at_least):
    """percolation noise -- at byte 128 one large piece among 200 small ones, at 200 above a thousand small pieces: capacities of all,
    exactly n, one fewer and 1; the ids and the summary count every piece whatever the table keeps; the bytes behind the kept records
    are not touched"""
    from volym_amd import scene
    host = CS.scene_a()
    c = scene.Components(CS.BOXES["whole"], 0, min_byte)
    full = CS.expect(host, c)
    n = int(full[0]["n_components"])
    assert n > at_least and int(full[0]["recorded"]) == n
    with _ctx(layout) as ctx:
        host.upload(ctx)
        _same("default capacity", _run(ctx, c), full)
        table = torch.as_tensor(_DeviceBytes(ctx.component_table_device_ptr(), 24 * n), device="cuda")      # the context's buffer holds >= n records
        for cap in (n, n - 1, 1):
            table.fill_(0xA5)
            torch.cuda.synchronize()
            k = c.replace(max_components=cap)
            got = _run(ctx, k)
            want = CS.expect(host, k)
            _same(("capacity", cap), got, want)
            assert int(got[0]["recorded"]) == cap and int(got[0]["n_components"]) == n
            assert got[1].tobytes() == full[1][:cap].tobytes() and np.array_equal(got[2], full[2])
            raw = table.cpu().numpy()
            assert raw[:24 * cap].tobytes() == full[1][:cap].tobytes(), cap
            assert (raw[24 * cap:] == 0xA5).all(), ("written behind the capacity", cap)
        _refused(-1, ctx.read_component_table, 0)                 # room for fewer records than the pass kept


def test_the_same_request_three_times_gives_the_same_bytes(volym_lib):
    from volym_amd import scene
    host = CS.scene_b()
    with _ctx(1) as ctx:
        host.upload(ctx)
        for flags in (0, CS.SPLIT):
            c = scene.Components(CS.BOXES["x 5..30"], flags, 128)
            first = _run(ctx, c)
            for k in range(3):
                assert CS.as_bytes(_run(ctx, c)) == CS.as_bytes(first), (flags, k)
            _same("x 5..30", first, CS.expect(host, c))
        ctx.components_pass(scene.Components(CS.BOXES["whole"]))
        t = scene.Components(CS.BOXES["texel"])
        _same("texel after whole", _run(ctx, t), CS.expect(host, t))      # a second pass carries nothing of the first
        e = scene.Components(CS.BOXES["empty"])
        got = _run(ctx, e)
        _same("empty after whole", got, scene.empty_components())
        _same("NULL", _run(ctx, None), CS.expect(host, scene.Components(dims=CS.DIMS)))


@pytest.mark.parametrize("layout", [0, 1])
def test_ids_of_sub_boxes_and_of_single_texels(volym_lib, layout):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    box = CS.BOXES["x 5..30"]
    c = scene.Components(box, 0, 128)
    (x0, y0, z0), (x1, y1, z1) = box
    with _ctx(layout) as ctx:
        host.upload(ctx)
        ctx.components_pass(c)
        summary, table, ids = CS.expect(host, c)
        for lo, hi in ((box[0], box[1]), ((7, 4, 2), (19, 11, 9)), ((5, 3, 1), (30, 19, 2)), ((29, 18, 17), (30, 19, 18)), ((9, 5, 5), (9, 9, 9))):
            want = ids[lo[2] - z0:hi[2] - z0, lo[1] - y0:hi[1] - y0, lo[0] - x0:hi[0] - x0]
            got = ctx.read_component_ids((lo, hi))
            assert got.shape == want.shape and np.array_equal(got, want), (lo, hi)
        for k in (0, 1, len(table) // 2, len(table) - 1):        # record k's root texel carries id k
            assert ctx.component_of(int(table["x"][k]), int(table["y"][k]), int(table["z"][k])) == k
        air = np.argwhere(ids == _lib.COMPONENT_NONE)[:3]
        assert len(air) == 3
        for z, y, x in air.tolist():
            assert ctx.component_of(x + x0, y + y0, z + z0) == _lib.COMPONENT_NONE
        for t in ((4, 3, 1), (30, 3, 1), (5, 19, 1), (5, 3, 18), (5, 2, 1)):
            _refused(_lib.E_INVALID, ctx.component_of, *t)
        _refused(_lib.E_INVALID, ctx.read_component_ids, ((4, 3, 1), (30, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_component_ids, ((5, 3, 1), (31, 19, 18)))
        _refused(_lib.E_INVALID, ctx.read_component_ids, ((9, 3, 1), (8, 19, 18)))


def test_the_reads_are_a_snapshot_and_a_new_volume_voids_it(volym_lib):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    c = scene.Components(CS.BOXES["rows"], 0, 128)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.components_pass)                                # no volume
        for read in (ctx.read_components, ctx.read_component_table, ctx.read_component_ids, lambda: ctx.component_of(0, 0, 0)):
            _refused(_lib.E_STATE, read)                                            # no pass
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_components)
        want = _check(ctx, host, "before the edits", c)
        ctx.set_crop_box(*CS.BOX)                                                   # edits after the pass: the reads still give the snapshot
        ctx.set_segment_visibility(scene.visibility_mask(CS.HIDDEN))
        summary = ctx.read_components()
        _same("after a crop", (summary, ctx.read_component_table(summary["recorded"]), ctx.read_component_ids()), want)
        ctx.set_volume(host.vol, host.dims, 0)
        for read in (ctx.read_components, ctx.read_component_table, ctx.read_component_ids, lambda: ctx.component_of(0, 5, 2)):
            _refused(_lib.E_STATE, read)
        assert ctx.components_device_ptr() is None and ctx.component_ids_device_ptr() is None and ctx.component_table_device_ptr() is None
        _check(ctx, host, "after the new volume", c)               # (box and mask are reset; the labels stay)


def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = CS.scene_a()
    whole = scene.Components(dims=CS.DIMS)
    with _ctx(0) as ctx:
        host.upload(ctx, labels=False)
        ctx.components_pass(whole)                                                  # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(CS.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.components_pass, scene.Components(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(CS.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.components_pass, scene.Components((tuple(lo), tuple(hi))))
        _refused(_lib.E_INVALID, ctx.components_pass, whole.replace(flags=4))
        _refused(_lib.E_INVALID, ctx.components_pass, whole.replace(min_byte=0))
        _refused(_lib.E_INVALID, ctx.components_pass, whole.replace(min_byte=256))
        _refused(_lib.E_INVALID, ctx.components_pass, whole.replace(max_components=_lib.COMPONENTS_TABLE_MAX + 1))
        assert volym_lib.volym_components_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_components(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_components(None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_component_table(None, None, 0) == _lib.E_INVALID
        assert volym_lib.volym_read_component_ids(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_component_of(None, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_component_of(ctx.handle, 0, 0, 0, None) == _lib.E_INVALID
        assert volym_lib.volym_components_device_ptr(None) is None
        summary = ctx.read_components()                                             # a refused pass leaves the latest result usable
        _same("after the refusals", (summary, ctx.read_component_table(), ctx.read_component_ids()), CS.expect(host, whole, labels=False))


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
def test_a_frame_is_the_same_with_and_without_components_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        c = scene.Components(((5, 3, 8), (60, 50, 64)), CS.SPLIT, 40, scene.surface_select([2, 3]))
        want = scene.components_volume(vol, dims, c, labels=labels)
        assert int(want[0]["n_solid"]) > 1000 and (want[0]["per_label"] > 0).sum() == 2
        _same("before any update", _run(ctx, c), want)            # before any volym_update or compute pass
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.components_pass(c)
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after the components pass"
        for k in range(3):                                        # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.components_pass(c)
            ctx.compute_pass()
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            summary = ctx.read_components()
            _same(("components", k), (summary, ctx.read_component_table(summary["recorded"]), ctx.read_component_ids()), want)


def test_a_sharded_context_splits_the_whole_volume(volym_lib):
    from volym_amd import scene
    with _ctx(0, w=160, h=96) as ctx:
        ctx.set_shard(1, 2)
        dims, vol, labels = _bonsai_scene(ctx)
        for c in (scene.Components(dims=dims, min_byte=40), scene.Components(((0, 10, 20), (64, 40, 50)), CS.SPLIT, 1, scene.surface_select([2, 4]))):
            _same("sharded", _run(ctx, c), scene.components_volume(vol, dims, c, labels=labels))


# ---- 5. the Python callers and the CLIs --------------------------------------------------------------------------------------------------
def test_simple_splits_the_bonsai_into_its_pieces(oracle, volym_lib):
    from tests import common
    from volym_amd import _lib, demo, scene
    n = 32
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
                {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        alone = lambda l, m: scene.components_volume(vol, dims, scene.Components(dims=dims, min_byte=m, select=scene.surface_select([l])), labels=lab)
        got = d.components(ctx, ["Canopy", 4], min_byte=30)
        assert list(got) == ["Canopy", "Pot"]
        for name, l in (("Canopy", 2), ("Pot", 4)):
            summary, table, _ = alone(l, 30)
            want = scene.components_summary(summary, table)[l]
            assert {k: got[name][k] for k in want} == want, name
            assert got[name]["solid"] == int(summary["n_solid"]) and got[name]["pieces"] == int(summary["n_components"]) >= 1
            assert got[name]["top"][0] == want["largest"] and len(got[name]["top"]) == min(10, len(table))
        assert set(d.components(ctx)) >= {"Canopy", "Trunk", "Pot"}
        assert d.components(ctx, ["Trunk"], min_byte=255) == {}   # no texel that dense: no piece
        rec, _ = scene.measure_volume(vol, dims, scene.Measure(dims=dims), labels=lab)
        d.update_gpu_state(ctx, state)
        d.compute_pass(ctx)
        hits = 0
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (2, 2)):
            p = d.component_at(ctx, x, y)
            if p["status"] == "hit" and p["label"] is not None:
                summary, table, ids = alone(p["label"], 1)
                tx, ty, tz = p["texel"]
                k = int(ids[tz, ty, tx])
                if k == _lib.COMPONENT_NONE:
                    assert p["component"] is None
                    continue
                hits += 1
                want = scene.component_dict(table[k], k)
                want.update(pieces=int(summary["n_components"]), segment_count=int(rec["count"][p["label"]]))
                assert p["component"] == want, (x, y)
            else:
                assert p["component"] is None
        assert hits >= 1


@pytest.mark.parametrize("cli", ["python", "native"])
@pytest.mark.parametrize("arg, heads", [("", 3), ("Lobster:203", 1)])
def test_both_clis_print_the_pieces(volym_lib, tmp_path, cli, arg, heads):
    """--components on `run simple` with the built-in teapot: every segment (cup, ground and lobster at least), and the lobster alone
    from a byte that breaks it into pieces"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + ["--components"] + ([arg] if arg else []), capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if " piece" in l]
    head = [l for l in lines if not l.startswith("  piece")]
    assert len(head) >= heads and all("solid texels, largest" in l for l in head), r.stdout
    assert any(l.startswith("  piece") and "root (" in l and "box [" in l for l in lines), r.stdout
    if arg:
        assert len(head) == 1 and head[0].startswith("Lobster") and " 1 piece " not in head[0], r.stdout


# ---- 6. the workload's scale ---------------------------------------------------------------------------------------------------------
def test_the_canopy_of_the_bonsai_at_256(volym_lib):
    """one pass over 256^3 in the bricked layout: the scan spans workgroups and a piece has more than a million texels"""
    from volym_amd import scene
    dims, vol, lab = _bonsai(256)
    c = scene.Components(dims=dims, select=scene.surface_select([2]))
    want = scene.components_volume(vol, dims, c, labels=lab)
    assert int(want[0]["n_solid"]) > 1000000 and int(want[1]["count"].max()) > 1000000
    with _ctx(1) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(lab, dims)
        _same("canopy", _run(ctx, c), want)


# ---- 7. the offset scan's second level: more than 256 blocks of 256 rows ----------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_the_offset_scan_with_two_block_sums_per_thread(volym_lib, layout):
    """65792 rows are 257 blocks of the scan, so the one workgroup that scans the block sums owns two per thread: the number of every
    row's first root comes out of it.  The surface test's scene, box and request with SPLIT_LABELS, then no flags and every label."""
    from tests import surface_scenes as S
    dims, vol, labels = S.scan_scene()
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for split in (True, False):
            c, want = CS.scan_components(split)
            _same(("scan", split), _run(ctx, c), want)
