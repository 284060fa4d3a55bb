"""The interpolate pass (fill between slices) and the edit by it on the device (volym_interpolate_pass and its reads,
volym_interpolate_labels).

The expected results are scene.interpolate_volume and scene.interpolate_labels_volume, the host twins of the rules (pinned to a
per-texel restatement, to closed forms and to a case about the 64-bit comparison by tests/test_interpolate_host.py), of the prepared
arrays the context was given and the cut state it was put in.  Every comparison is over all 65592 bytes of the summary, the whole
signed map and the whole state map, and over the 4128 bytes of an edit's result and every label: the rule is integer, so there is no
tolerance and nothing is left out.  After an edit the context is compared with one that was handed the edited labels, as
tests/test_gpu_relabel.py compares it.  The scenes and requests are those of tests/interpolate_scenes.py.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import interpolate_scenes as IS
from tests.test_gpu_crop_box import _ctx
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(what, got, want):
    if IS.as_bytes(got) == IS.as_bytes(want):
        return
    for k, name in ((1, "signed map"), (2, "state")):
        assert got[k].shape == want[k].shape, (what, name, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (what, name + " [z, y, x]", len(bad), bad[:4].tolist(), got[k][got[k] != want[k]][:4].tolist(), want[k][got[k] != want[k]][:4].tolist())
    for k in ("n_slices", "n_keys", "n_gaps", "n_gap_slices", "n_refused", "reserved", "n_shape", "n_inside", "n_new", "n_stale"):
        assert int(got[0][k]) == int(want[0][k]), (what, k, int(got[0][k]), int(want[0][k]))
    for k in ("kind", "key_lo", "key_hi", "count"):
        g, w = got[0]["slice"][k], want[0]["slice"][k]
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, k, bad[:4].ravel().tolist(), g[g != w][:4].tolist(), w[g != w][:4].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _read(ctx):
    return ctx.read_interpolate(), ctx.read_interpolate_map(), ctx.read_interpolate_state()


def _run(ctx, q):
    """one pass and the three reads"""
    ctx.interpolate_pass(q)
    return _read(ctx)


def _check(ctx, host, what, q, labels=True):
    want = IS.expect(host, q, labels)
    _same(what, _run(ctx, q), want)
    return want


# ---- 1. every axis, boxes, selections, weights, max_gap, KEYS and cuts, both scenes, both layouts ---------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_request_under_every_cut(volym_lib, layout, which):
    host = IS.scene_a() if which == "a" else IS.scene_b()
    inside = gaps = refused = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.interpolate_device_ptr() is None and ctx.interpolate_map_device_ptr() is None and ctx.interpolate_state_device_ptr() is None
        for turn in range(3):
            for name, q in IS.requests(0, turn):
                s = _check(ctx, host, ("never cut", name), q)[0]
                inside, gaps, refused = inside + int(s["n_inside"]), gaps + int(s["n_gaps"]), refused + int(s["n_refused"])
        assert ctx.interpolate_device_ptr() and ctx.interpolate_map_device_ptr() and ctx.interpolate_state_device_ptr()
        for name, q in IS.requests(IS.UNCUT, 3)[::2]:
            _check(ctx, host, ("uncut, never cut", name), q)
        for turn, (step, box, plane, hidden) in enumerate(IS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for name, q in IS.requests(0, turn)[turn % 3::3]:
                inside += int(_check(ctx, host, (step, name), q)[0]["n_inside"])
            for name, q in IS.requests(IS.UNCUT, turn + 1)[:3]:
                _check(ctx, host, (step, "uncut", name), q)
    assert inside > 10000 and gaps > 20 and refused > 5, (inside, gaps, refused)


@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels(volym_lib, layout):
    host = IS.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, q in IS.requests(0, 1)[::2] + IS.requests(0, 3)[1::3]:
            _check(ctx, host, ("no labels", name), q, labels=False)
        host.set_cut(ctx, IS.BOX, IS.PLANE, None)
        for name, q in IS.requests(0, 2)[::3]:
            _check(ctx, host, ("no labels, cut", name), q, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_rows_longer_than_a_wave(volym_lib, layout):
    """97, 94, 66, 65 and 64 texels: a row is swept in chunks of 64, and the nearest seed of both maps is carried from chunk to chunk both
    ways; along x the slice counts go through the histogram in LDS"""
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    assert {b[1][0] - b[0][0] for b in IS.LONG_BOXES.values()} >= {64, 65, 97}
    inside = 0
    with _ctx(layout) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_labels(labels, dims)
        for k, (name, box) in enumerate(IS.LONG_BOXES.items()):
            for axis in range(3):
                lo, hi = box[0][axis], box[1][axis]
                keys = tuple(range(lo + 1 + k, hi, 9 + axis)) + (lo + 2 + k,)
                min_byte, select, weight = ((100, scene.surface_select([1, 5]), (4, 1, 9)), (150, scene.surface_select([2]), (64, 25, 1)), (3, None, (1, 64, 4)))[(k + axis) % 3]
                q = scene.Interpolate(box, IS.KEYS, min_byte, select, weight, axis, (0, 9)[k % 2], keys)
                want = scene.interpolate_volume(vol, dims, q, labels=labels)
                inside += int(want[0]["n_inside"])
                _same((name, axis), _run(ctx, q), want)
    assert inside > 10000


@pytest.mark.parametrize("layout", [0, 1])
def test_the_constructed_scenes(volym_lib, layout):
    """in-plane extents of 1; 1, 2 and 3 slices; adjacent keys; a gap at max_gap and one wider; one key and none; a key that is all
    SHAPE; a KEYS slice without SHAPE; the strips' ties; the case about 2^32; a box off the origin and off the brick grid"""
    from volym_amd import scene
    with _ctx(layout) as ctx:
        for name, (dims, vol, lab, q) in IS.constructed().items():
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            _same(name, _run(ctx, q), scene.interpolate_volume(vol, dims, q, labels=lab))


def test_sub_boxes_single_texels_and_repeats(volym_lib):
    from volym_amd import _lib, scene
    host = IS.scene_a()
    box = ((5, 3, 1), (30, 19, 18))
    q = scene.Interpolate(box, IS.KEYS, 128, None, (1, 4, 9), 1, 0, (3, 7, 8, 15, 18))
    (x0, y0, z0), _hi = box
    with _ctx(1) as ctx:
        host.upload(ctx)
        first = _run(ctx, q)
        summary, words, state = IS.expect(host, q)
        _same("first", first, (summary, words, state))
        assert IS.as_bytes(_run(ctx, q)) == IS.as_bytes(first)
        for lo, hi in ((box[0], box[1]), ((7, 4, 2), (19, 11, 9)), ((5, 3, 4), (30, 19, 9)), ((29, 18, 17), (30, 19, 18)), ((9, 5, 5), (9, 9, 9))):
            part = (slice(lo[2] - z0, hi[2] - z0), slice(lo[1] - y0, hi[1] - y0), slice(lo[0] - x0, hi[0] - x0))
            for got, want in ((ctx.read_interpolate_map((lo, hi)), words[part]), (ctx.read_interpolate_state((lo, hi)), state[part])):
                assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (lo, hi)
        for x, y, z in ((5, 3, 1), (29, 18, 17), (17, 11, 9), (12, 7, 16)):
            assert ctx.interpolate_at(x, y, z) == {"word": int(words[z - z0, y - y0, x - x0]), "state": int(state[z - z0, y - y0, x - x0])}, (x, y, z)
        for t in ((4, 3, 1), (30, 3, 1), (5, 19, 1), (5, 3, 18)):
            _refused(_lib.E_INVALID, ctx.interpolate_at, *t)
        for read in (ctx.read_interpolate_map, ctx.read_interpolate_state):
            _refused(_lib.E_INVALID, read, ((4, 3, 1), (30, 19, 18)))
            _refused(_lib.E_INVALID, read, ((9, 3, 1), (8, 19, 18)))
        small = scene.Interpolate(((17, 9, 11), (18, 10, 12)), 0, 1, None, (1, 1, 1), 2)
        _same("a small box after a larger", _run(ctx, small), IS.expect(host, small))
        _same("an empty box", _run(ctx, scene.Interpolate(((3, 4, 5), (3, 9, 9)))), scene.empty_interpolate())


def test_refusals_of_the_pass(volym_lib):
    from volym_amd import _lib, scene
    host = IS.scene_a()
    whole = scene.Interpolate(dims=IS.DIMS)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.interpolate_pass, whole)                          # no volume
        host.upload(ctx, labels=False)
        ctx.interpolate_pass(whole)
        for a in range(3):
            hi = list(IS.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.interpolate_pass, scene.Interpolate(((0, 0, 0), tuple(hi))))
            w = [1, 1, 1]; w[a] = 0
            _refused(_lib.E_INVALID, ctx.interpolate_pass, whole.replace(weight=tuple(w)))
            w[a] = 65
            _refused(_lib.E_INVALID, ctx.interpolate_pass, whole.replace(weight=tuple(w)))
        for bad in (dict(flags=4), dict(min_byte=256), dict(axis=3)):
            _refused(_lib.E_INVALID, ctx.interpolate_pass, whole.replace(**bad))
        assert volym_lib.volym_interpolate_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_interpolate_pass(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_interpolate(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_interpolate_at(ctx.handle, 0, 0, 0, None, None) == _lib.E_INVALID
        assert volym_lib.volym_interpolate_device_ptr(None) is None
        _same("after the refusals", _read(ctx), IS.expect(host, whole, labels=False))
    with _ctx(0) as ctx:
        host.upload(ctx, labels_layout=1)
        _refused(_lib.E_STATE, ctx.interpolate_pass, whole)                          # labels in the other layout


# ---- 2. the edit ---------------------------------------------------------------------------------------------------------------------------
def _edit(ctx, host, case, snap=None, passes=True):
    """run the pass `case` reads and the edit, compare the result with the twin's and take the twin's labels; returns the result"""
    from volym_amd import scene
    if passes:
        ctx.interpolate_pass(case.interpolate)
    if snap is None:
        snap = IS.expect(host, case.interpolate)
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, want = scene.interpolate_labels_volume(now, host.dims, case.edit, host.labels, snap[2], case.interpolate.box, uncut=host.vol if host.ever_cut else None)
    got = ctx.interpolate_labels(case.edit)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not case.edit.flags & IS.EDIT_DRY_RUN:
        host.labels = new.ravel()
    assert np.array_equal(ctx.read_labels().ravel(), host.labels), case.name
    return got


def _painted_host():
    """the edit's scene as the helpers of tests/test_gpu_relabel.py take a scene"""
    from tests.test_gpu_slice import Host
    dims, vol, labels = IS.edit_scene()
    host = Host(dims)
    host.vol, host.labels = vol, labels
    return host


@pytest.mark.parametrize("layout", [0, 1])
def test_every_edit_and_the_context_after_it(oracle, volym_lib, layout):
    host = _painted_host()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = {}
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(IS.edit_cases(host.dims)):
            if k:
                _hand_labels(ctx, host, original)
            changed[case.name] = int(_edit(ctx, host, case)["changed"])
            if case.edit.flags & IS.EDIT_DRY_RUN or case.name == "identity tables":
                assert np.array_equal(host.labels, original), case.name
            _look(ctx, host, ref, case.name, uniforms)
        host.set_cut(ctx, ((2, 1, 0), (17, 12, 17)), None, [7])
        for case in IS.edit_cases(host.dims)[2:5]:
            _hand_labels(ctx, host, original)
            _edit(ctx, host, case)
            _look(ctx, host, ref, ("cut", case.name), uniforms)
        uncut = IS.edit_cases(host.dims)[3]
        _hand_labels(ctx, host, original)
        _edit(ctx, host, IS.EditCase("UNCUT", uncut.interpolate.replace(flags=IS.KEYS | IS.UNCUT), uncut.edit.replace(flags=IS.EDIT_UNCUT)))
        _look(ctx, host, ref, "cut, UNCUT", uniforms)
    assert changed["identity tables"] == 0 and changed["both"] > changed["to alone"] > 200 and changed["out alone"] > 50, changed
    assert changed["a dry run"] == changed["to alone"] + changed["out alone"] > changed["a density window"] > 0 and changed["a sub-box"] > 0, changed


@pytest.mark.parametrize("layout", [0, 1])
def test_edits_undone_and_redone_and_a_journal_that_does_not_fit(oracle, volym_lib, layout):
    from tests.test_gpu_label_history import Run
    from volym_amd import _lib, scene
    cases = [c for c in IS.edit_cases(_painted_host().dims) if c.name in ("to alone", "out alone", "a dry run", "along x")]
    host = _painted_host()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, 64 << 20, bool(layout), ref, _frame_uniforms(oracle))
        states = [host.labels.copy()]
        for case in cases:
            old = host.labels.copy()
            _edit(ctx, host, case)
            if not case.edit.flags & IS.EDIT_DRY_RUN:
                run.twin.record(old, host.labels, box=case.edit.box)
            run.same_info(case.name)
            states.append(host.labels.copy())
        steps = run.twin.info()["undo_steps"]
        assert steps == len(cases) - 1                                  # each edit one step; the dry run none
        for k in range(steps):
            run.swap(False, look=k == steps - 1)
        assert np.array_equal(host.labels, states[0])
        for k in range(steps):
            run.swap(True, look=k == steps - 1)
        assert np.array_equal(host.labels, states[-1])
    case = cases[0]
    host = _painted_host()
    snap = IS.expect(host, case.interpolate)
    new = scene.interpolate_labels_volume(host.vol, host.dims, case.edit, host.labels, snap[2], case.interpolate.box)[0]
    records = scene.label_chunks_changed(host.dims, host.labels, new, bool(layout))
    assert records > 20
    for budget, kept in ((20 * records, True), (20 * (records - 1), False)):
        host = _painted_host()
        with _ctx(layout) as ctx, Reference(layout) as ref:
            host.upload(ctx)
            run = Run(ctx, host, budget, bool(layout), ref, _frame_uniforms(oracle))
            old = host.labels.copy()
            _edit(ctx, host, case)                                      # returns OK either way, and its labels are right
            assert run.twin.record(old, host.labels, box=case.edit.box) == kept
            run.same_info(case.name)
            info = ctx.label_history_info()
            assert (info["undo_steps"], info["lost"], info["next_undo_records"]) == ((1, 0, records) if kept else (0, 1, 0))
            if kept:
                run.swap(False)
            else:
                _refused(_lib.E_STATE, ctx.undo_labels)


# ---- 3. the snapshot's rules -----------------------------------------------------------------------------------------------------------------
def test_the_snapshot_outlives_edits_and_a_new_volume_voids_it(oracle, volym_lib):
    from volym_amd import _lib, scene
    host = _painted_host()
    case = IS.edit_cases(host.dims)[2]
    inner = scene.Interpolate(((2, 1, 1), (17, 13, 16)), IS.KEYS, 0, IS.table(5), (1, 1, 1), 2, 0, (2, 7, 8, 15))
    reads = lambda ctx: (ctx.read_interpolate, ctx.read_interpolate_map, ctx.read_interpolate_state, lambda: ctx.interpolate_at(3, 3, 3))
    with _ctx(0) as ctx, Reference(0) as ref:
        for read in reads(ctx):
            _refused(_lib.E_STATE, read)                                             # no pass
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_interpolate)
        _refused(_lib.E_STATE, ctx.interpolate_labels, case.edit)                    # no pass
        snap = _check(ctx, host, "the pass", inner)
        _refused(_lib.E_INVALID, ctx.interpolate_labels, case.edit)                  # the whole volume reaches outside the pass's box
        for bad in (dict(flags=4), dict(window=(9, 8)), dict(window=(0, 256)), dict(box=((0, 0, 0), (host.dims[0] + 1, 1, 1)))):
            _refused(_lib.E_INVALID, ctx.interpolate_labels, case.edit.replace(**bad))
        assert volym_lib.volym_interpolate_labels(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_interpolate_labels(ctx.handle, None, None) == _lib.E_INVALID
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)                # no refusal wrote a label
        # a brush on a key slice, a crop and new labels in between: the snapshot stays, and the edit by it follows the twin given the same
        dab = scene.Brush([(9, 6, 7)], 9, to={0: 5, 5: 0}, dims=host.dims)
        ctx.brush_labels(dab)
        host.labels = scene.brush_volume(host.vol, host.dims, dab, host.labels)[0].ravel()
        _same("after a brush", _read(ctx), snap)
        host.set_cut(ctx, ((1, 0, 0), (18, 13, 17)), None, None)
        _same("after a crop", _read(ctx), snap)
        _hand_labels(ctx, host, np.where(host.labels == 7, 0, host.labels).astype(np.uint8))
        _same("after new labels", _read(ctx), snap)
        assert IS.as_bytes(IS.expect(host, inner)) != IS.as_bytes(snap)              # (the scene has moved on)
        stale = IS.EditCase("by the stale snapshot", inner, case.edit.replace(box=inner.box))
        assert int(_edit(ctx, host, stale, snap, passes=False)["changed"]) > 200
        _look(ctx, host, ref, "an edit by a stale snapshot", _frame_uniforms(oracle))
        ctx.set_volume(host.vol, host.dims, 0)
        for read in reads(ctx):
            _refused(_lib.E_STATE, read)
        assert ctx.interpolate_device_ptr() is None and ctx.interpolate_map_device_ptr() is None and ctx.interpolate_state_device_ptr() is None
        ctx.set_labels(host.labels, host.dims)
        _refused(_lib.E_STATE, ctx.interpolate_labels, stale.edit)


# ---- 4. a session: fill, repaint a key, fill again with KEYS and `out`, and undo all of it --------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_a_short_session(oracle, volym_lib, layout):
    from volym_amd import scene
    host = _painted_host()
    host.labels = np.where(IS.turned(IS.painted(), 2), 5, 0).astype(np.uint8).ravel()       # the painted slices alone
    first = host.labels.copy()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        ctx.label_history(8 << 20)
        plain = IS.EditCase("the first fill", scene.Interpolate(None, 0, 0, IS.table(5), (1, 1, 1), 2, dims=host.dims), scene.InterpolateEdit(dims=host.dims, to={0: 5}))
        assert int(_edit(ctx, host, plain)["changed"]) > 200
        dab = scene.Brush([(13, 9, 15)], 16, to={0: 5}, dims=host.dims)                      # the key slice 15 repainted
        ctx.brush_labels(dab)
        host.labels = scene.brush_volume(host.vol, host.dims, dab, host.labels)[0].ravel()
        again = IS.EditCase("the fill again", plain.interpolate.replace(flags=IS.KEYS, keys=(2, 7, 8, 15)), scene.InterpolateEdit(dims=host.dims, to={0: 5}, out={5: 0}))
        got = _edit(ctx, host, again)
        assert int(got["arrived"][5]) > 0 and int(IS.expect(host, again.interpolate)[0]["n_stale"]) == 0      # the stale texels are gone
        _look(ctx, host, ref, "after the session", _frame_uniforms(oracle))
        assert ctx.label_history_info()["undo_steps"] == 3
        for _ in range(3):
            ctx.undo_labels()
        assert np.array_equal(ctx.read_labels().ravel(), first)
        host.labels = first
        _look(ctx, host, ref, "after the undos", _frame_uniforms(oracle))


def test_simple_fills_between_slices(oracle, volym_lib):
    """the synthetic bonsai at 64^3 with the canopy kept on every 8th slice: Simple.fill_between puts it back by the twins' rule"""
    from tests import common
    from volym_amd import demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    keys = tuple(range(0, n, 8))
    sparse = labels_raw.reshape(n, n, n).copy()
    keep = np.zeros(n, bool)
    keep[list(keys)] = True
    sparse[~keep] = np.where(sparse[~keep] == 2, 0, sparse[~keep])
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=sparse.ravel(), segments=segments, dims=dims)
        vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(sparse.ravel(), dims, True)
        (got,) = d.fill_between(ctx, ["Canopy"], "z", keys=keys, replace=True)
        q = scene.Interpolate(None, IS.KEYS, 0, IS.table(2), (1, 1, 1), 2, 0, keys, dims=dims)
        snap = scene.interpolate_volume(vol, dims, q, labels=lab)
        want_labels, want = scene.interpolate_labels_volume(vol, dims, scene.InterpolateEdit(dims=dims, to={0: 2}, out={2: 0}), lab, snap[2], q.box)
        assert got["relabel"] == scene.relabel_result_dict(want) and got["relabel"]["changed"] > 5000
        assert got["summary"] == scene.interpolate_summary(snap[0]) and got["summary"]["n_gaps"] >= 1
        assert np.array_equal(ctx.read_labels(), want_labels)


def _fill_between_line(stdout):
    """the numbers of the one line --fill-between prints per segment, by the word that follows each"""
    head = [l for l in stdout.splitlines() if l.startswith("fill between:")]
    assert len(head) == 1 and " key slices, " in head[0] and " texels joined, " in head[0], stdout
    m = re.search(r" label \d+, (\d+) key slices, (\d+) gaps of (\d+) slices filled, (\d+) refused: (\d+) texels joined, (\d+) left$", head[0])
    assert m, head[0]
    return dict(zip(("key", "gaps", "slices", "refused", "texels", "left"), (int(v) for v in m.groups())))


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_clis_fill_between_slices(volym_lib, tmp_path, cli):
    """--fill-between on `run simple` with the built-in scene, whose segment is on every slice it touches: keys without gaps, the same
    line from both CLIs"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + ["--fill-between", "Lobster:z:6"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    got = _fill_between_line(r.stdout)
    assert got["key"] > 3 and got["texels"] == 0 and got["left"] == 0, r.stdout
    bad = subprocess.run(cmd + ["--fill-between", "Lobster:w"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert bad.returncode != 0 and "--fill-between" in bad.stderr + bad.stdout, (bad.stdout, bad.stderr)


def test_the_python_cli_fills_between_named_keys(volym_lib, tmp_path):
    """--fill-between with --fill-between-keys: every fifth slice along z is kept, the rest is interpolated, and what the segment held
    outside the interpolated shape goes back to 0"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png"), "--fill-between", "Lobster:z:6",
           "--fill-between-keys", ",".join(str(z) for z in range(0, 4096, 5))]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _fill_between_line(r.stdout)
    assert got["gaps"] > 3 and got["texels"] + got["left"] > 0, r.stdout
