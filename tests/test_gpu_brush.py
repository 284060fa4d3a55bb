"""The brush on the device (volym_brush_labels).

The expected labels and result are scene.brush_volume's, the host twin of the rule (pinned to exact fractions and to a plain triple
loop by tests/test_brush_host.py).  The rule is integer: there is no tolerance anywhere and nothing is left out.  After every call the
result's 4128 bytes, the labels (whole and on a sub-box), the label counts and the state of the context are compared with the twin and
with a reference context that is handed the twin's labels (tests/test_gpu_relabel._look).  The scenes and strokes are those of
tests/brush_scenes.py, whose properties tests/test_brush_host.py asserts on the twin.
"""
import ctypes as C

import numpy as np
import pytest

from tests import brush_scenes as BS
from tests import label_history_scenes as LS
from tests import measure_scenes as MS
from tests.test_gpu_crop_box import _ctx
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu


def _brush(ctx, host, case, brush=None):
    """the stroke on the device, its result against the twin's; the twin's labels are taken; returns the result"""
    from volym_amd import _lib
    b = brush or case.brush
    new, want = BS.expect(host, case, b)
    got = ctx.brush_labels(b)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not b.flags & _lib.BRUSH_DRY_RUN:
        host.labels = new
    return got


# ---- 1. every stroke, both layouts, before any cut and under cuts -------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(BS.SCENES))
def test_every_stroke_before_any_cut(oracle, volym_lib, layout, which):
    host = BS.SCENES[which]()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(BS.cases(host.dims)):
            if k:
                _hand_labels(ctx, host, original)
            changed += int(_brush(ctx, host, case)["changed"])
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 1000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_after_each_cut(oracle, volym_lib, layout):
    host = BS.SCENES["a"]()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    cases = BS.cases()
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(MS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in cases[step % 4::4]:
                _hand_labels(ctx, host, original)
                _brush(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_strokes_on_top_of_each_other_then_cuts_that_move(oracle, volym_lib, layout):
    """cumulative strokes (no fresh labels in between), then masks and a crop that rewrite from the recomputed label boxes"""
    host = BS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in BS.cases()}
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        for name in ("capsule along x, r2 4", "two crossing capsules, 1 <-> 2", "the long diagonal, r2 6", "two crossing capsules, 1 <-> 2"):
            _brush(ctx, host, cases[name])
        _look(ctx, host, ref, "four strokes", uniforms)
        for hidden in ([7], [1, 2], None):
            host.set_cut(ctx, None, None, hidden)
            _look(ctx, host, ref, ("hidden", hidden), uniforms)
        host.set_cut(ctx, MS.BOX, MS.PLANE, [7])
        _brush(ctx, host, cases["256 points of a random walk"])
        _look(ctx, host, ref, "a stroke under all three cuts", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "all lifted", uniforms)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_brush_into_a_hidden_label_without_voxels_in_a_context_that_never_cut(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = BS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    case = BS.Case("everything -> 9", scene.Brush([(6, 6, 6), (30, 15, 13)], 20, to=BS.every(9), dims=host.dims))
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [9])                             # no voxel carries 9: no byte changes, no copy is made
        moved = int(_brush(ctx, host, case)["changed"])
        assert moved > 500
        _look(ctx, host, ref, "moved into the hidden label", uniforms)
        whole = scene.Measure(dims=host.dims)
        ctx.measure_pass(whole)
        assert int(ctx.read_measure()[0]["count"][9]) == 0              # the moved texels' density reads 0 ...
        ctx.measure_pass(whole.replace(flags=_lib.MEASURE_UNCUT))
        rec = ctx.read_measure()[0]
        assert int(rec["count"][9]) == moved and int(rec["min"][9]) >= 1    # ... and is kept in the uncut copy
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "the label shown again", uniforms)


# ---- 2. dry runs, no-ops and the surface pass -----------------------------------------------------------------------------------
def test_a_dry_run_changes_nothing_and_only_a_real_stroke_makes_a_surface_stale(oracle, volym_lib):
    from volym_amd import _lib, scene
    host = BS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in BS.cases()}
    with _ctx(1) as ctx, Reference(1, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, MS.BOX, None, [4])
        s = scene.Surface(dims=host.dims, min_byte=100)
        ctx.surface_pass(s)
        ctx.surface_faces_pass()
        total = int(ctx.read_surface()["total"])
        faces = ctx.read_surface_faces(total).tobytes()
        assert total > 100
        before = host.labels.copy()
        assert int(_brush(ctx, host, cases["dry run"])["changed"]) > 50 and np.array_equal(host.labels, before)
        for name in ("identity table", "empty box", "a box the hull misses"):
            assert int(_brush(ctx, host, cases[name])["changed"]) == 0
        _look(ctx, host, ref, "after a dry run and no-ops", uniforms)
        ctx.surface_faces_pass()                                        # still the surface of the scene as it stands
        assert ctx.read_surface_faces(total).tobytes() == faces
        real = cases["dry run"].brush.replace(flags=0)
        assert int(_brush(ctx, host, cases["dry run"], real)["changed"]) > 50
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        _look(ctx, host, ref, "after the real stroke", uniforms)


# ---- 3. the history -------------------------------------------------------------------------------------------------------------
class Run:
    """a context, the twin of its labels (host.labels) and the twin of its history, driven together"""

    def __init__(self, ctx, host, budget, bricked, ref=None, uniforms=None):
        from volym_amd import scene
        self.ctx, self.host, self.ref, self.uniforms, self.bricked = ctx, host, ref, uniforms, bricked
        self.twin = scene.LabelHistory(budget, host.dims, bricked)
        ctx.label_history(budget)
        self.same_info("switched on")

    def same_info(self, what):
        assert self.ctx.label_history_info() == self.twin.info(), (what, self.ctx.label_history_info(), self.twin.info())

    def look(self, what):
        if self.ref is not None:
            _look(self.ctx, self.host, self.ref, what, self.uniforms)

    def brush(self, case, look=True):
        from volym_amd import scene
        old = self.host.labels.copy()
        got = _brush(self.ctx, self.host, case)
        if not case.brush.flags & 16:
            self.twin.record(old, self.host.labels, box=scene.brush_box(case.brush, self.host.dims))
        self.same_info(case.name)
        if look:
            self.look(case.name)
        return got

    def swap(self, redo, look=True):
        what = "redo" if redo else "undo"
        labels, want = (self.twin.redo if redo else self.twin.undo)(self.host.labels)
        got = self.ctx.redo_labels() if redo else self.ctx.undo_labels()
        assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, what
        self.host.labels = labels
        self.same_info(what)
        if look:
            self.look(what)
        return got


HISTORY = ("the long diagonal, r2 6", "two crossing capsules, 1 <-> 2", "dry run", "256 points of a random walk", "a box the hull misses", "two whole rows, r2 0")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "ragged"])
def test_strokes_undone_and_redone(oracle, volym_lib, layout, which):
    from volym_amd import _lib
    host = BS.SCENES[which]()
    cases = {c.name: c for c in BS.cases(host.dims)}
    start = host.labels.copy()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        results = [run.brush(cases[name]) for name in HISTORY]
        steps = [r for r, name in zip(results, HISTORY) if int(r["changed"]) and name != "dry run"]
        assert len(steps) == 4 and ctx.label_history_info()["undo_steps"] == 4          # a dry run and a no-op are no steps
        for r in reversed(steps):
            assert run.swap(False).tobytes() == LS.swapped(r).tobytes()
        assert np.array_equal(host.labels, start)
        _refused(_lib.E_STATE, ctx.undo_labels)
        for r in steps:
            assert run.swap(True).tobytes() == r.tobytes()
        _refused(_lib.E_STATE, ctx.redo_labels)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_brush_after_two_undos_drops_the_redo_steps(oracle, volym_lib, layout):
    from volym_amd import _lib
    host = BS.SCENES["a"]()
    cases = {c.name: c for c in BS.cases()}
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        for name in ("capsule along x, r2 4", "the long diagonal, r2 6", "two crossing capsules, 1 <-> 2"):
            run.brush(cases[name], look=False)
        after_first = None
        run.swap(False, look=False)
        run.swap(False, look=False)
        after_first = host.labels.copy()
        assert ctx.label_history_info()["redo_steps"] == 2
        run.brush(cases["256 points of a random walk"])
        assert ctx.label_history_info()["redo_steps"] == 0 and ctx.label_history_info()["undo_steps"] == 2
        _refused(_lib.E_STATE, ctx.redo_labels)
        run.swap(False)
        assert np.array_equal(host.labels, after_first)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_budget_one_record_short_of_the_strokes_step_gives_the_history_up(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = BS.SCENES["a"]()
    cases = {c.name: c for c in BS.cases()}
    small, big = cases["ball of r2 25 at the origin"], cases["the long diagonal, r2 6"]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        run.brush(small, look=False)
        first = ctx.label_history_info()["next_undo_records"]
        records = scene.label_chunks_changed(host.dims, host.labels, BS.expect(host, big)[0], bool(layout))
        assert 0 < first < records - 1
        ctx.label_history(20 * (records - 1))                           # the first step still fits
        run.twin.set_budget(20 * (records - 1))
        run.same_info("a smaller budget")
        assert ctx.label_history_info()["undo_steps"] == 1
        run.brush(big)                                                  # carried out, and the whole history is given up
        info = ctx.label_history_info()
        assert info["lost"] == 1 and info["undo_steps"] == 0 and info["used_bytes"] == 0
        _refused(_lib.E_STATE, ctx.undo_labels)
    host = BS.SCENES["a"]()
    records = scene.label_chunks_changed(host.dims, host.labels, BS.expect(host, big)[0], bool(layout))
    with _ctx(layout) as ctx:
        host.upload(ctx)
        run = Run(ctx, host, 20 * records, bool(layout))                # one record more: the step is kept
        run.brush(big)
        assert ctx.label_history_info()["lost"] == 0 and ctx.label_history_info()["next_undo_records"] == records


@pytest.mark.parametrize("layout", [0, 1])
def test_a_volume_whose_chunks_span_rows_and_slices(volym_lib, layout):
    """5 x 3 x 9: a slice is smaller than a chunk, so a linear chunk spans up to four rows and two slices and the last one is partial.
    Every stroke with the history off and on, then one undo; result and all 135 labels against the twin after each call"""
    host = BS.scene_small()
    original = host.labels.copy()
    with _ctx(layout) as ctx:
        host.upload(ctx)
        for budget in (0, LS.BIG):
            ctx.label_history(budget)
            for case in BS.small_cases():
                _hand_labels(ctx, host, original)
                got = _brush(ctx, host, case)
                assert 0 < int(got["changed"]) < original.size, case.name
                assert np.array_equal(ctx.read_labels().ravel(), host.labels), (case.name, budget)
                if budget:
                    undone = ctx.undo_labels()
                    assert undone.tobytes() == LS.swapped(got).tobytes(), case.name
                    assert np.array_equal(ctx.read_labels().ravel(), original), case.name


# ---- 4. frames in flight --------------------------------------------------------------------------------------------------------
def test_a_brush_between_frames_with_two_frames_in_flight(oracle, volym_lib):
    from volym_amd import _lib
    host = BS.SCENES["a"]()
    cu, pu = _frame_uniforms(oracle)
    cases = {c.name: c for c in BS.cases()}
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)]) as ctx, Reference(0, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [4])
        ctx.update(cu, pu)
        for _ in range(3):
            ctx.compute_pass()
        before = ctx.read_rgba8()
        for name in ("the long diagonal, r2 6", "256 points of a random walk"):
            ctx.compute_pass()                                          # a frame in flight while the stroke arrives
            _brush(ctx, host, cases[name])
            frames = []
            for _ in range(3):                                          # both slots, with no update in between
                ctx.compute_pass()
                frames.append(ctx.read_rgba8())
            r = ref.at(host)
            r.update(cu, pu)
            r.compute_pass()
            want = r.read_rgba8()
            assert not np.array_equal(want, before), "the stroke must show"
            for k, f in enumerate(frames):
                assert np.array_equal(f, want), (name, "frame", k)
            before = want


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = BS.SCENES["a"]()
    ball = scene.Brush([(18, 10, 9)], 16, to=BS.every(7), dims=host.dims)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.brush_labels, ball)                  # no volume
        host.upload(ctx, labels=False)
        _refused(_lib.E_STATE, ctx.brush_labels, ball)                  # no labels
        other = (host.dims[0] + 1, host.dims[1], host.dims[2])
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)
        _refused(_lib.E_STATE, ctx.brush_labels, ball)                  # labels of other dimensions
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        dry = int(ctx.brush_labels(ball.replace(flags=_lib.BRUSH_DRY_RUN))["changed"])
        assert dry == int(scene.brush_mask(ball, host.dims).sum()) > 50
        for a in range(3):
            hi = list(host.dims); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.brush_labels, ball.replace(box=((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(host.dims); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.brush_labels, ball.replace(box=(tuple(lo), tuple(hi))))
            p = [1, 1, 1]; p[a] = host.dims[a]
            _refused(_lib.E_INVALID, ctx.brush_labels, ball.replace(points=[(1, 1, 1), tuple(p)]))
            for w in (0, 65):
                wt = [1, 1, 1]; wt[a] = w
                _refused(_lib.E_INVALID, ctx.brush_labels, ball.replace(weight=tuple(wt)))
        for bad in (dict(flags=2), dict(flags=32), dict(window=(9, 8)), dict(window=(0, 256)), dict(points=[]), dict(points=[(1, 1, 1, 2)])):
            _refused(_lib.E_INVALID, ctx.brush_labels, ball.replace(**bad))
        c = ball.to_c()
        c.n_points = 257
        assert volym_lib.volym_brush_labels(ctx.handle, C.byref(c), None) == _lib.E_INVALID
        assert volym_lib.volym_brush_labels(None, C.byref(ball.to_c()), None) == _lib.E_INVALID
        assert volym_lib.volym_brush_labels(ctx.handle, None, None) == _lib.E_INVALID
        # nothing above changed a label, and a NULL result is accepted
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)
        assert volym_lib.volym_brush_labels(ctx.handle, C.byref(ball.to_c()), None) == _lib.OK
        assert int((ctx.read_labels() == 7).sum()) == dry


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = BS.SCENES["a"]()
    ball = scene.Brush([(18, 10, 9)], 16, to=BS.every(7), dims=host.dims)
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.brush_labels, ball)
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)


# ---- 6. the Python callers ------------------------------------------------------------------------------------------------------
def test_simple_paints_the_bonsai(oracle, volym_lib):
    from tests import common
    from volym_amd import _lib, demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
                {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        d.compute_pass(ctx)
        d.history(ctx, 16)
        # a pixel that misses: nothing is painted, nothing is recorded
        miss = d.brush_at(ctx, 0, 0, "Moss", 3)
        assert miss["status"] != "hit" and miss["relabel"] is None and ctx.label_history_info()["undo_steps"] == 0
        # click to paint: a ball of radius 3 (round in a spacing of 1, 1, 2) over every label, a new segment
        hit = None
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (100, 40)):
            p = d.brush_at(ctx, x, y, "Moss", 3, over=None, spacing=(1, 1, 2))
            if p["relabel"] is not None:
                hit = p
                break
        assert hit is not None
        moss = next(s for s in d._segments if s["name"] == "Moss")["label_value"]
        assert moss not in (0, 2, 3, 4)
        want, res = scene.brush_volume(vol, dims, scene.Brush([hit["texel"]], 9, to=BS.every(moss), weight=(1, 1, 4), dims=dims), lab)
        assert hit["relabel"] == scene.relabel_result_dict(res) and hit["relabel"]["changed"] > 20
        assert np.array_equal(ctx.read_labels(), want)
        lab = want.ravel()
        # a drag over picked pixels and one that misses: one pick pass over their rect, a LIFT after the miss, one undo step
        pixels = [(x, y) for x in range(70, 91, 4)] + [(0, 0)] + [(80, 40), (84, 44)]
        ctx.pick_pass((0, 0, 91, 49), 0.5)
        rec = ctx.read_picks()
        points, lift = [], False
        for x, y in pixels:
            r = rec[y, x]
            if int(r["status"]) != _lib.PICK_HIT:
                lift = True
                continue
            points.append((int(r["x"]), int(r["y"]), int(r["z"]), 1 if lift and points else 0))
            lift = False
        got = d.stroke(ctx, pixels, None, 2, over=["Moss", "Canopy"])
        assert got["picked"] == len(points) and got["missed"] == len(pixels) - len(points) >= 1
        if points:
            to = {moss: 0, 2: 0}
            want, res = scene.brush_volume(vol, dims, scene.Brush(points, 4, to=to, dims=dims), lab)
            assert got["calls"] == 1 and got["relabel"] == scene.relabel_result_dict(res)
            assert np.array_equal(ctx.read_labels(), want)
            if int(res["changed"]):
                assert ctx.label_history_info()["undo_steps"] == 2
                assert d.undo(ctx)["changed"] == int(res["changed"])
                assert np.array_equal(ctx.read_labels().ravel(), lab)
        with pytest.raises(ValueError):
            d.stroke(ctx, [(160, 0)], "Moss", 2)
        with pytest.raises(ValueError):
            d.stroke(ctx, [], "Moss", 2)


def test_a_stroke_of_more_than_256_points_is_several_calls(volym_lib):
    from tests import common
    from volym_amd import demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=(n, n, n))
        d.compute_pass(ctx)
        d.history(ctx, 16)
        pixels = [(x, y) for y in range(16, 84, 2) for x in range(30, 130)]
        got = d.stroke(ctx, pixels, "Paint", 1, over=None)
        assert got["picked"] > 256 and got["calls"] == -(-(got["picked"] - 1) // 255)
        assert ctx.label_history_info()["undo_steps"] == got["calls"] and got["relabel"]["changed"] > 200
        paint = next(s for s in d._segments if s["name"] == "Paint")["label_value"]
        assert int((ctx.read_labels() == paint).sum()) == got["relabel"]["changed"] == got["relabel"]["arrived"][paint]


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_clis_brush_and_write_the_labels(volym_lib, tmp_path, cli):
    """--brush and --labels-out on `run simple` with the built-in teapot: the file holds the painted labels; --undo takes the stroke
    back; the Python CLI also drags the brush over pixels"""
    import json
    import os
    import subprocess
    import sys
    from volym_amd import scene, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    out = str(tmp_path / "labels.raw")
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(root, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + ["--brush", "100,128,128/140,120,130/140,150,130:Lobster:30", "--labels-out", out], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    dims = (256, 256, 256)
    raw, labels_raw = synth.synth_teapot()
    before = scene.prepare_volume(labels_raw, dims, True)
    stroke = scene.Brush([(100, 128, 128), (140, 120, 130), (140, 150, 130)], 30, to=np.full(256, 2), dims=dims)
    want, res = scene.brush_volume(scene.prepare_volume(raw, dims, True), dims, stroke, before)
    moved = int(res["changed"])
    assert moved > 1000
    saved = np.fromfile(out, np.uint8)
    assert saved.size == 256 ** 3 and np.array_equal(scene.prepare_volume(saved, dims, True), want.ravel())
    box = [int(v) for v in res["box"]]
    if cli == "native":
        line = [l for l in r.stdout.splitlines() if l.startswith("brush:")]
        assert len(line) == 1 and line[0].startswith("brush: %d texels changed, box [%d,%d,%d)..[%d,%d,%d)" % tuple([moved] + box)) and \
            "label 2: -0 +%d" % moved in line[0], r.stdout
    else:
        first = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"brush"')]
        assert len(first) == 1 and first[0]["brush"]["changed"] == moved and first[0]["brush"]["arrived"] == {"2": moved}
        assert first[0]["brush"]["box"] == [box[:3], box[3:]]
    # the stroke runs before --undo, which takes it back
    r = subprocess.run(cmd + ["--brush", "100,128,128/140,120,130/140,150,130:Lobster:30", "--undo", "1", "--labels-out", out], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(scene.prepare_volume(np.fromfile(out, np.uint8), dims, True), before)
    assert r.stdout.index("brush") < r.stdout.index("undo")
    # (a name no segment has is a new segment to the Python CLI, as for --split-at; the native one knows the table's names only)
    for bad in (["--brush", "1,2,3:Lobster"], ["--brush", "1,2:Lobster:4"], ["--brush", "300,2,3:Lobster:4"]) + ((["--brush", "1,2,3:Nobody:4"],) if cli == "native" else ()):
        r = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode != 0, (bad, r.stdout[-500:])
    if cli == "python":
        r = subprocess.run(cmd + ["--brush-at", "70,45/80,45/90,45/0,0:Picked:3"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        drag = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"brush_at"')]
        assert len(drag) == 1 and drag[0]["brush_at"] is not None
        assert drag[0]["brush_at"]["picked"] + drag[0]["brush_at"]["missed"] == 4 and drag[0]["brush_at"]["picked"] >= 1 and drag[0]["brush_at"]["changed"] > 0
