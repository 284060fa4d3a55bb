"""Undo and redo of label edits on the device (volym_label_history / volym_undo_labels / volym_redo_labels).

The expected labels, results and bookkeeping are scene.LabelHistory's, the host twin of the rule (pinned to a model of whole copies by
tests/test_label_history_host.py, which also asserts the conditions relied on here).  The rule is integer: there is no tolerance
anywhere and nothing is left out.  After every edit, undo and redo the result's 4128 bytes and the history's info are compared with
the twin, and the labels, the label counts and the state of the context with a reference context that is handed the twin's labels
(tests/test_gpu_relabel._look).  The edits and budgets are those of tests/label_history_scenes.py.
"""
import ctypes as C

import numpy as np
import pytest

from tests import label_history_scenes as LS
from tests import measure_scenes as MS
from tests import relabel_scenes as RS
from tests.test_gpu_crop_box import _ctx
from tests.test_gpu_relabel import Reference, _cut_to, _edit, _frame_uniforms, _look, _refused

pytestmark = pytest.mark.gpu


class Run:
    """a context, the twin of its labels (host.labels) and the twin of its history, driven together"""

    def __init__(self, ctx, host, budget, bricked, ref=None, uniforms=None):
        from volym_amd import scene
        self.ctx, self.host, self.ref, self.uniforms = ctx, host, ref, uniforms
        self.twin = scene.LabelHistory(budget, host.dims, bricked)
        ctx.label_history(budget)
        self.same_info("switched on")

    def same_info(self, what):
        assert self.ctx.label_history_info() == self.twin.info(), (what, self.ctx.label_history_info(), self.twin.info())

    def look(self, what):
        if self.ref is not None:
            _look(self.ctx, self.host, self.ref, what, self.uniforms)

    def edit(self, case, look=True):
        old = self.host.labels.copy()
        got = _edit(self.ctx, self.host, case)                          # (compares the result with the twin's and takes its labels)
        if not case.relabel.flags & 16:
            self.twin.record(old, self.host.labels, box=case.relabel.box)
        self.same_info(case.name)
        if look:
            self.look(case.name)
        return got

    def swap(self, redo, look=True):
        what = "redo" if redo else "undo"
        labels, want = (self.twin.redo if redo else self.twin.undo)(self.host.labels)
        got = self.ctx.redo_labels() if redo else self.ctx.undo_labels()
        for k in ("changed", "left", "arrived", "box"):
            assert np.array_equal(got[k], want[k]), (what, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
        assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, what
        self.host.labels = labels
        self.same_info(what)
        if look:
            self.look(what)
        return got


# ---- 1. cumulative edits, all undone, all redone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(LS.CHOSEN))
def test_edits_undone_and_redone(oracle, volym_lib, layout, which):
    host, cases = LS.chosen(which)
    labels, _ = LS.twin_steps(which)
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        edits = [run.edit(case) for case in cases]
        for k in range(len(cases), 0, -1):
            got = run.swap(False)
            assert got.tobytes() == LS.swapped(edits[k - 1]).tobytes()
            assert np.array_equal(host.labels, labels[k - 1])
        _refused(_lib().E_STATE, ctx.undo_labels)
        for k in range(len(cases)):
            got = run.swap(True)
            assert got.tobytes() == edits[k].tobytes()
            assert np.array_equal(host.labels, labels[k + 1])
        _refused(_lib().E_STATE, ctx.redo_labels)
        assert run.twin.info()["undo_steps"] == len(cases) and run.twin.info()["used_bytes"] == 20 * sum(LS.records(which, bool(layout)))


def _lib():
    from volym_amd import _lib
    return _lib


# ---- 2. a new edit drops the redo steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_a_new_edit_after_two_undos_drops_the_redo_steps(oracle, volym_lib, layout):
    host, cases = LS.chosen("a")
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        for case in cases[:3]:
            run.edit(case, look=False)
        run.swap(False, look=False)
        run.swap(False, look=False)
        assert ctx.label_history_info()["redo_steps"] == 2
        run.edit(cases[3])                                             # on the labels after the first edit alone
        assert ctx.label_history_info()["redo_steps"] == 0 and ctx.label_history_info()["undo_steps"] == 2
        _refused(_lib().E_STATE, ctx.redo_labels)
        run.swap(False)
        run.swap(False)
        assert np.array_equal(host.labels, LS.twin_steps("a")[0][0])


# ---- 3. cuts that move between an edit and its undo -------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_cuts_that_move_between_an_edit_and_its_undo(oracle, volym_lib, layout):
    host = RS.scene_a()
    cases = {c.name: c for c in RS.cases_a()}
    name, box, plane, _ = MS.CUTS[7]
    assert name == "all three"
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        host.set_cut(ctx, box, plane, None)
        run.edit(cases["table, x 3..8"], look=False)                   # 0, 1 -> 9 and 4 -> 2 in a narrow box
        run.edit(cases["merge 1, 2 -> 4, whole"])                      # labels 1 and 2 are gone
        assert int((host.labels == 1).sum()) == 0
        host.set_cut(ctx, ((5, 0, 3), (36, 22, 12)), plane, [1, 4, 9])  # another box; 1 has no voxels now, 4 and 9 have
        run.swap(False)                                                # texels go back into 1 (hidden) and 2, and leave 4 (hidden)
        assert int((host.labels == 1).sum()) > 50
        run.swap(False, look=False)                                    # ... and leave 9 (hidden) for 0, 1 (hidden) and 4 (hidden)
        host.set_cut(ctx, None, None, None)
        run.look("all lifted")
        run.swap(True, look=False)
        host.set_cut(ctx, None, MS.PLANE, [9])
        run.swap(True)                                                 # redone under a plane and a mask


@pytest.mark.parametrize("layout", [0, 1])
def test_undo_into_a_hidden_label_without_voxels_in_a_context_that_never_cut(oracle, volym_lib, layout):
    """nothing has made the uncut copies: the undo makes them, as an edit into such a label does"""
    from volym_amd import scene
    host = RS.scene_a()
    cases = {c.name: c for c in RS.cases_a()}
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        run.edit(cases["merge 1, 2 -> 4, whole"], look=False)
        host.set_cut(ctx, None, None, [1])                             # no voxel carries 1: no byte changes, no copy is made
        moved = int(run.swap(False)["arrived"][1])
        assert moved > 500
        whole = scene.Measure(dims=host.dims)
        ctx.measure_pass(whole)
        assert int(ctx.read_measure()[0]["count"][1]) == 0              # the restored texels' density reads 0 ...
        ctx.measure_pass(whole.replace(flags=_lib().MEASURE_UNCUT))
        assert int(ctx.read_measure()[0]["count"][1]) == moved          # ... and is kept in the uncut copy
        host.set_cut(ctx, None, None, None)
        run.look("the label shown again")
        host.set_cut(ctx, None, None, [4])
        run.swap(True)                                                 # and the redo sends them into the hidden 4


# ---- 4. the budget ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_the_small_budget_evicts_the_oldest_step(oracle, volym_lib, layout):
    host, cases = LS.chosen("a")
    labels, _ = LS.twin_steps("a")
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.small_budget(bool(layout)), bool(layout), ref, _frame_uniforms(oracle))
        for case in cases:
            run.edit(case, look=False)
        info = ctx.label_history_info()
        assert info["dropped_steps"] == 1 and info["undo_steps"] == 3 and info["lost"] == 0 and info["used_bytes"] <= info["budget_bytes"]
        for _ in range(3):
            run.swap(False, look=False)
        _refused(_lib().E_STATE, ctx.undo_labels)                       # one step early: the first edit stays
        assert np.array_equal(host.labels, labels[1])
        run.look("three of four undone")
        # a budget that holds only the nearest redo step: the two that would be redone last go
        rec = LS.records("a", bool(layout))
        ctx.label_history(20 * rec[1])
        run.twin.set_budget(20 * rec[1])
        run.same_info("a smaller budget")
        assert ctx.label_history_info()["redo_steps"] == 1 and ctx.label_history_info()["dropped_steps"] == 3
        run.swap(True)
        assert np.array_equal(host.labels, labels[2])


@pytest.mark.parametrize("layout", [0, 1])
def test_an_edit_that_does_not_fit_gives_the_history_up(oracle, volym_lib, layout):
    host, cases = LS.chosen("a")
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.overflow_budget(bool(layout)), bool(layout), ref, _frame_uniforms(oracle))
        run.edit(cases[0], look=False)
        assert ctx.label_history_info()["undo_steps"] == 1
        run.edit(cases[1])                                             # returns OK, and its labels are right (_edit, _look)
        info = ctx.label_history_info()
        assert info["lost"] == 1 and info["undo_steps"] == 0 and info["redo_steps"] == 0 and info["used_bytes"] == 0
        _refused(_lib().E_STATE, ctx.undo_labels)
        run.edit(cases[2], look=False)                                 # the history goes on with the steps that fit
        assert ctx.label_history_info()["undo_steps"] == 1
        run.swap(False)


# ---- 5. defaults and refusals ---------------------------------------------------------------------------------------------------------
def test_defaults_clearing_and_refusals(oracle, volym_lib):
    from volym_amd import _lib, scene
    host, cases = LS.chosen("a")
    by_name = {c.name: c for c in RS.cases_a()}
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.undo_labels)                         # off, and no volume
        host.upload(ctx)
        assert set(ctx.label_history_info().values()) == {0}
        _edit(ctx, host, cases[0])
        _refused(_lib.E_STATE, ctx.undo_labels)                         # off by default: the edit recorded nothing
        _refused(_lib.E_STATE, ctx.redo_labels)
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)
        run = Run(ctx, host, LS.BIG, False)
        _refused(_lib.E_STATE, ctx.undo_labels)                         # on, nothing to undo
        # a dry run, an identity table and an empty box record no step
        dry = RS.Case("dry", cases[1].relabel.replace(flags=_lib.RELABEL_DRY_RUN))
        assert int(run.edit(dry)["changed"]) > 50
        for name in ("identity", "empty box"):
            assert int(run.edit(by_name[name])["changed"]) == 0
        assert ctx.label_history_info()["undo_steps"] == 0
        run.edit(cases[1])
        run.edit(cases[2])
        assert ctx.label_history_info()["undo_steps"] == 2
        # label_history(0) frees the steps; on again starts empty
        ctx.label_history(0)
        assert set(ctx.label_history_info().values()) == {0}
        _refused(_lib.E_STATE, ctx.undo_labels)
        # set_labels, set_volume and set_importances each clear the steps and keep the budget
        for clear in (lambda: (ctx.set_labels(host.labels, host.dims), ctx.set_segment_importances(host.table)),
                      lambda: ctx.set_volume(host.vol, host.dims, 0),
                      lambda: (ctx.set_importances(host.table[host.labels], host.dims), ctx.set_labels(host.labels, host.dims),
                               ctx.set_segment_importances(host.table))):
            run = Run(ctx, host, LS.BIG, False)
            run.edit(cases[3])
            run.swap(False)
            assert (ctx.label_history_info()["undo_steps"], ctx.label_history_info()["redo_steps"]) == (0, 1)
            clear()
            run.twin.clear()
            run.same_info("cleared")
            assert ctx.label_history_info()["budget_bytes"] == LS.BIG and ctx.label_history_info()["redo_steps"] == 0
            _refused(_lib.E_STATE, ctx.redo_labels)
        # a refused undo leaves a surface pass valid for the faces pass; a successful one makes it stale
        run = Run(ctx, host, LS.BIG, False)
        run.edit(cases[3])
        s = scene.Surface(dims=host.dims, min_byte=100)
        ctx.surface_pass(s)
        ctx.surface_faces_pass()
        _refused(_lib.E_STATE, ctx.redo_labels)
        ctx.surface_faces_pass()
        run.swap(False)
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        ctx.surface_pass(s)
        ctx.surface_faces_pass()
        # no labels of the volume's dimensions: the states volym_edit_labels refuses
        ctx.set_importances(host.table[host.labels], host.dims)          # (drops the labels and clears the steps)
        _refused(_lib.E_STATE, ctx.undo_labels)
        # NULL ctx and NULL output through the raw library
        assert volym_lib.volym_label_history(None, 1 << 20) == _lib.E_INVALID
        assert volym_lib.volym_undo_labels(None, None) == _lib.E_INVALID
        assert volym_lib.volym_redo_labels(None, None) == _lib.E_INVALID
        assert volym_lib.volym_label_history_info(None, None) == _lib.E_INVALID
        assert volym_lib.volym_label_history_info(ctx.handle, None) == _lib.E_INVALID
        assert C.sizeof(_lib.LabelHistoryInfo) == 56
        # a NULL result is accepted
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, False)
        run.edit(cases[3])
        assert volym_lib.volym_undo_labels(ctx.handle, None) == _lib.OK and volym_lib.volym_redo_labels(ctx.handle, None) == _lib.OK
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)


# ---- 6. frames in flight --------------------------------------------------------------------------------------------------------------
def test_an_undo_between_frames_with_two_frames_in_flight(oracle, volym_lib):
    from volym_amd import _lib
    host, cases = LS.chosen("a")
    cu, pu = _frame_uniforms(oracle)
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)]) as ctx, Reference(0, reuse=False) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, False)
        host.set_cut(ctx, None, None, [4])
        run.edit(cases[1])
        run.edit(cases[3])
        ctx.update(cu, pu)
        for _ in range(3):
            ctx.compute_pass()
        before = ctx.read_rgba8()
        for redo in (False, False, True):
            ctx.compute_pass()                                          # a frame in flight while the undo arrives
            run.swap(redo)
            frames = []
            for _ in range(3):                                          # both slots, with no update in between
                ctx.compute_pass()
                frames.append(ctx.read_rgba8())
            r = ref.at(host)
            r.update(cu, pu)
            r.compute_pass()
            want = r.read_rgba8()
            assert not np.array_equal(want, before), "the swap must show"
            for k, f in enumerate(frames):
                assert np.array_equal(f, want), ("redo" if redo else "undo", "frame", k)
            before = want


# ---- 7. the Python callers --------------------------------------------------------------------------------------------------------------
def test_simple_undoes_and_redoes_on_the_bonsai(oracle, volym_lib, tmp_path):
    from tests import common
    from volym_amd import _lib, demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab0 = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
                {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    whole = ((0, 0, 0), dims)
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        assert d.undo(ctx) is None and d.redo(ctx) is None              # history off: nothing to take back
        d.history(ctx, budget_mb=8)
        assert ctx.label_history_info()["budget_bytes"] == 8 << 20 and d.undo(ctx) is None
        dist = scene.distance_volume(vol, dims, scene.Distance(dims=dims, select=scene.surface_select([2])), labels=lab0)
        lab1, res1 = scene.relabel_volume(vol, dims, scene.Relabel(dims=dims, flags=_lib.RELABEL_DISTANCE, to={0: 2}, d2=(0, 4)), lab0, dmap=dist[1], dmap_box=whole)
        grown = d.grow(ctx, "Canopy", 2)
        assert grown["changed"] == int(res1["changed"]) > 50 and np.array_equal(ctx.read_labels(), lab1)
        dist = scene.distance_volume(vol, dims, scene.Distance(dims=dims, flags=_lib.DISTANCE_INSIDE, select=scene.surface_select([2])), labels=lab1.ravel())
        lab2, res2 = scene.relabel_volume(vol, dims, scene.Relabel(dims=dims, flags=_lib.RELABEL_DISTANCE, to={2: 0}, d2=(0, 1)), lab1.ravel(), dmap=dist[1], dmap_box=whole)
        shrunk = d.shrink(ctx, "Canopy", 1)
        assert shrunk["changed"] == int(res2["changed"]) > 50 and np.array_equal(ctx.read_labels(), lab2)
        twin = scene.LabelHistory(8 << 20, dims, False)
        twin.record(lab0, lab1)
        twin.record(lab1, lab2)
        assert ctx.label_history_info() == twin.info()
        back = d.undo(ctx)
        assert back == dict(shrunk, left=shrunk["arrived"], arrived=shrunk["left"]) and np.array_equal(ctx.read_labels(), lab1)
        back = d.undo(ctx)
        assert back == dict(grown, left=grown["arrived"], arrived=grown["left"]) and np.array_equal(ctx.read_labels().ravel(), lab0)
        assert d.undo(ctx) is None
        path = str(tmp_path / "labels.raw")
        assert d.save_labels(ctx, path) == n ** 3
        assert np.array_equal(scene.prepare_volume(np.fromfile(path, np.uint8), dims, True), np.asarray(lab0).ravel())
        assert d.redo(ctx) == grown and np.array_equal(ctx.read_labels(), lab1)
        assert d.save_labels(ctx, path) == n ** 3
        assert np.array_equal(scene.prepare_volume(np.fromfile(path, np.uint8), dims, True), lab1.ravel())
        assert ctx.label_history_info()["undo_steps"] == 1 and ctx.label_history_info()["redo_steps"] == 1


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_clis_undo_a_relabel_and_write_the_original_labels(volym_lib, tmp_path, cli):
    """--relabel, --undo 1 and --labels-out on `run simple` with the built-in teapot: the file holds the labels as they were read"""
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
    r = subprocess.run(cmd + ["--relabel", "Cup,4:Lobster", "--undo", "1", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    dims = (256, 256, 256)
    _, labels_raw = synth.synth_teapot()
    before = scene.prepare_volume(labels_raw, dims, True)
    moved = int(((before == 3) | (before == 4)).sum())
    assert moved > 1000
    saved = np.fromfile(out, np.uint8)
    assert saved.size == 256 ** 3 and np.array_equal(scene.prepare_volume(saved, dims, True), before)
    if cli == "native":
        lines = [l for l in r.stdout.splitlines() if l.startswith(("relabel:", "undo:"))]
        assert len(lines) == 2 and lines[0].startswith("relabel: %d texels changed, box [" % moved) and "label 2: -0 +%d" % moved in lines[0], r.stdout
        assert lines[1].startswith("undo: %d texels changed, box [" % moved) and "label 2: -%d +0" % moved in lines[1], r.stdout
        assert lines[1].split(";")[0][len("undo"):] == lines[0].split(";")[0][len("relabel"):]
        return
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [list(l)[0] for l in lines] == ["relabel", "undo"], r.stdout
    edit, undo = lines[0]["relabel"], lines[1]["undo"]
    assert edit["changed"] == moved and undo == dict(edit, left=edit["arrived"], arrived=edit["left"])
