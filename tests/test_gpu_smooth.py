"""The smoothing on the device (volym_smooth_labels).

The expected labels and result are scene.smooth_volume's, the host twin of the rule (pinned to a plain triple loop by
tests/test_smooth_host.py).  The rule is integer: there is no tolerance anywhere and nothing is left out.  After every call the
result's 4128 bytes, the labels (whole and on a sub-box), the label counts and the state of the context are compared with the twin and
with a reference context that is handed the twin's labels (tests/test_gpu_relabel._look).  The scenes and requests are those of
tests/smooth_scenes.py, whose properties tests/test_smooth_host.py asserts on the twin.
"""
import ctypes as C

import numpy as np
import pytest

from tests import label_history_scenes as LS
from tests import measure_scenes as MS
from tests import smooth_scenes as SS
from tests.test_gpu_crop_box import _ctx
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu


def _smooth(ctx, host, case, smooth=None):
    """the pass on the device, its result against the twin's; the twin's labels are taken; returns the result"""
    from volym_amd import _lib
    s = smooth or case.smooth
    new, want = SS.expect(host, case, s)
    got = ctx.smooth_labels(s)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not s.flags & _lib.SMOOTH_DRY_RUN:
        host.labels = new
    return got


# ---- 1. every case, both layouts, before any cut and under cuts ----------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(SS.SCENES))
def test_every_case_before_any_cut(oracle, volym_lib, layout, which):
    host = SS.SCENES[which]()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(SS.cases(host.dims)):
            if k:
                _hand_labels(ctx, host, original)
            changed += int(_smooth(ctx, host, case)["changed"])
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 1000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_after_each_cut(oracle, volym_lib, layout):
    host = SS.SCENES["a"]()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    cases = SS.cases()
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(MS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in cases[step % 4::4]:
                _hand_labels(ctx, host, original)
                _smooth(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_three_passes_on_top_of_each_other_then_cuts_that_move(oracle, volym_lib, layout):
    """cumulative passes (what `iterations` does), then masks and a crop that rewrite from the recomputed label boxes"""
    host = SS.SCENES["b"]()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in SS.cases()}
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        moved = [int(_smooth(ctx, host, cases["joint, radius 1"])["changed"]) for _ in range(3)]
        assert moved[0] > moved[1] > moved[2] > 100                    # the passes converge
        _look(ctx, host, ref, "three passes", uniforms)
        for hidden in ([7], [1, 2], None):
            host.set_cut(ctx, None, None, hidden)
            _look(ctx, host, ref, ("hidden", hidden), uniforms)
        host.set_cut(ctx, MS.BOX, MS.PLANE, [7])
        _smooth(ctx, host, cases["joint, radius 0, 2, 1"])
        _look(ctx, host, ref, "a pass under all three cuts", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "all lifted", uniforms)


@pytest.mark.parametrize("layout", [0, 1])
def test_smoothing_into_and_out_of_a_hidden_label_in_a_context_that_never_cut(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = SS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    case = {c.name: c for c in SS.cases()}["joint, radius 2"]
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [2])                             # label 2 has voxels: the first cut of this context
        got = _smooth(ctx, host, case)
        assert int(got["left"][2]) > 50 and int(got["arrived"][2]) > 50
        _look(ctx, host, ref, "texels moved into and out of the hidden label", uniforms)
        whole = scene.Measure(dims=host.dims)
        ctx.measure_pass(whole)
        assert int(ctx.read_measure()[0]["count"][2]) == 0              # what carries 2 now reads 0 ...
        ctx.measure_pass(whole.replace(flags=_lib.MEASURE_UNCUT))
        assert int(ctx.read_measure()[0]["count"][2]) == int((host.labels == 2).sum())    # ... and is kept in the uncut copy
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "the label shown again", uniforms)
    # ... and into a hidden label WITHOUT voxels: only label 9 takes, nothing carries it, so nothing moves and nothing breaks
    host = SS.SCENES["a"]()
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [9])
        none = SS.Case("only 9 takes", scene.Smooth(2, take=SS.table(9), dims=host.dims))
        assert int(_smooth(ctx, host, none)["changed"]) == 0
        _look(ctx, host, ref, "nothing moved", uniforms)


# ---- 2. dry runs, no-ops and the surface pass -----------------------------------------------------------------------------------
def test_a_dry_run_changes_nothing_and_only_a_real_pass_makes_a_surface_stale(oracle, volym_lib):
    from volym_amd import _lib, scene
    host = SS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in SS.cases()}
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
        assert int(_smooth(ctx, host, cases["dry run"])["changed"]) > 50 and np.array_equal(host.labels, before)
        for name in ("joint, inside slices", "empty box", "single texel"):
            assert int(_smooth(ctx, host, cases[name])["changed"]) == 0
        _look(ctx, host, ref, "after a dry run and no-ops", uniforms)
        ctx.surface_faces_pass()                                        # still the surface of the scene as it stands
        assert ctx.read_surface_faces(total).tobytes() == faces
        real = cases["dry run"].smooth.replace(flags=0)
        assert int(_smooth(ctx, host, cases["dry run"], real)["changed"]) > 50
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        _look(ctx, host, ref, "after the real pass", uniforms)


# ---- 3. the staging area: one launch, and a second with room for what the first counted ---------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("budget", [0, LS.BIG])
def test_a_pass_that_overruns_the_staging_area_and_one_that_does_not(volym_lib, layout, budget):
    """Scene B changes most of its chunks but has fewer of them than the staging area's floor; the same kind of labels over the ragged
    volume changes more than twice what the first launch has room for (tests/test_smooth_host.py asserts both on the twin).  The
    outcome is the twin's either way, and the step is one of the history."""
    from volym_amd import scene
    first = SS.cases()[0]
    for host in (SS.scene_overflow(), SS.SCENES["b"](), SS.SCENES["ragged"]()):
        case = SS.Case(first.name, first.smooth.replace(box=((0, 0, 0), host.dims)))
        start = host.labels.copy()
        with _ctx(layout) as ctx:
            host.upload(ctx)
            ctx.label_history(budget)
            got = _smooth(ctx, host, case)
            assert np.array_equal(ctx.read_labels().ravel(), host.labels)
            assert ctx.label_counts().tolist() == np.bincount(host.labels, minlength=256).tolist()
            if budget:
                records = scene.label_chunks_changed(host.dims, start, host.labels, bool(layout))
                info = ctx.label_history_info()
                assert info["undo_steps"] == 1 and info["next_undo_records"] == records and info["lost"] == 0
                assert ctx.undo_labels().tobytes() == LS.swapped(got).tobytes()
                assert np.array_equal(ctx.read_labels().ravel(), start)
                assert ctx.redo_labels().tobytes() == got.tobytes()
                assert np.array_equal(ctx.read_labels().ravel(), host.labels)


# ---- 4. the history -------------------------------------------------------------------------------------------------------------
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

    def smooth(self, case, look=True):
        old = self.host.labels.copy()
        got = _smooth(self.ctx, self.host, case)
        if not case.smooth.flags & 16:
            self.twin.record(old, self.host.labels, box=case.smooth.box)
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


HISTORY = ("joint, radius 2, x 5..30", "take leaves out 0 and 2", "dry run", "joint, radius 1", "empty box", "only 1 gives, radius 2")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_passes_undone_and_redone(oracle, volym_lib, layout, which):
    from volym_amd import _lib
    host = SS.SCENES[which]()
    cases = {c.name: c for c in SS.cases(host.dims)}
    start = host.labels.copy()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        results = [run.smooth(cases[name]) for name in HISTORY]
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
def test_a_pass_after_two_undos_drops_the_redo_steps(oracle, volym_lib, layout):
    from volym_amd import _lib
    host = SS.SCENES["a"]()
    cases = {c.name: c for c in SS.cases()}
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        for name in ("joint, radius 1", "joint, radius 2, rows", "only 1 gives, radius 2"):
            run.smooth(cases[name], look=False)
        run.swap(False, look=False)
        run.swap(False, look=False)
        after_first = host.labels.copy()
        assert ctx.label_history_info()["redo_steps"] == 2
        run.smooth(cases["joint, radius 3"])
        assert ctx.label_history_info()["redo_steps"] == 0 and ctx.label_history_info()["undo_steps"] == 2
        _refused(_lib.E_STATE, ctx.redo_labels)
        run.swap(False)
        assert np.array_equal(host.labels, after_first)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_budget_one_record_short_of_the_passes_step_gives_the_history_up(oracle, volym_lib, layout):
    from volym_amd import scene
    from volym_amd import _lib
    host = SS.SCENES["a"]()
    cases = {c.name: c for c in SS.cases()}
    small, big = cases["joint, radius 1"], cases["joint, radius 2"]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LS.BIG, bool(layout), ref, _frame_uniforms(oracle))
        run.smooth(small, look=False)
        first = ctx.label_history_info()["next_undo_records"]
        records = scene.label_chunks_changed(host.dims, host.labels, SS.expect(host, big)[0], bool(layout))
        assert 0 < first < records - 1
        ctx.label_history(20 * (records - 1))                           # the first step still fits
        run.twin.set_budget(20 * (records - 1))
        run.same_info("a smaller budget")
        assert ctx.label_history_info()["undo_steps"] == 1
        run.smooth(big)                                                 # carried out, and the whole history is given up
        info = ctx.label_history_info()
        assert info["lost"] == 1 and info["undo_steps"] == 0 and info["used_bytes"] == 0
        _refused(_lib.E_STATE, ctx.undo_labels)
    host = SS.SCENES["a"]()
    records = scene.label_chunks_changed(host.dims, host.labels, SS.expect(host, big)[0], bool(layout))
    with _ctx(layout) as ctx:
        host.upload(ctx)
        run = Run(ctx, host, 20 * records, bool(layout))                # one record more: the step is kept
        run.smooth(big)
        assert ctx.label_history_info()["lost"] == 0 and ctx.label_history_info()["next_undo_records"] == records


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("dims", SS.SMALL_DIMS)
def test_volumes_whose_chunks_span_rows_and_slices(volym_lib, layout, dims):
    """7 x 5 x 3 and 5 x 3 x 9: a linear chunk spans several rows (and slices) and the last one is partial; a brick row has two bricks.
    Every flag and radius with the history off and on, then one undo; result and all labels against the twin after each call"""
    from volym_amd import scene
    host = SS.scene_small(dims)
    original = host.labels.copy()
    with _ctx(layout) as ctx:
        host.upload(ctx)
        host.set_cut(ctx, ((1, 0, 0), dims), None, None)                # a crop, so that UNCUT reads other bytes
        for budget in (0, LS.BIG):
            ctx.label_history(budget)
            for name, r in SS.small_requests(dims):
                _hand_labels(ctx, host, original)
                got = _smooth(ctx, host, SS.Case(name, r))
                assert 0 < int(got["changed"]) < original.size, name
                assert np.array_equal(ctx.read_labels().ravel(), host.labels), (name, budget)
                if budget and not r.flags & 16:
                    undone = ctx.undo_labels()
                    assert undone.tobytes() == LS.swapped(got).tobytes(), name
                    assert np.array_equal(ctx.read_labels().ravel(), original), name


# ---- 5. frames in flight --------------------------------------------------------------------------------------------------------
def test_a_pass_between_frames_with_two_frames_in_flight(oracle, volym_lib):
    from volym_amd import _lib
    host = SS.SCENES["b"]()
    cu, pu = _frame_uniforms(oracle)
    cases = {c.name: c for c in SS.cases()}
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)]) as ctx, Reference(0, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [4])
        ctx.update(cu, pu)
        for _ in range(3):
            ctx.compute_pass()
        before = ctx.read_rgba8()
        for name in ("joint, radius 1", "joint, radius 2"):
            ctx.compute_pass()                                          # a frame in flight while the pass arrives
            _smooth(ctx, host, cases[name])
            frames = []
            for _ in range(3):                                          # both slots, with no update in between
                ctx.compute_pass()
                frames.append(ctx.read_rgba8())
            r = ref.at(host)
            r.update(cu, pu)
            r.compute_pass()
            want = r.read_rgba8()
            assert not np.array_equal(want, before), "the pass must show"
            for k, f in enumerate(frames):
                assert np.array_equal(f, want), (name, "frame", k)
            before = want


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = SS.SCENES["b"]()
    one = scene.Smooth(1, dims=host.dims)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.smooth_labels, one)                  # no volume
        host.upload(ctx, labels=False)
        _refused(_lib.E_STATE, ctx.smooth_labels, one)                  # no labels
        other = (host.dims[0] + 1, host.dims[1], host.dims[2])
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)
        _refused(_lib.E_STATE, ctx.smooth_labels, one)                  # labels of other dimensions
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        dry = int(ctx.smooth_labels(one.replace(flags=_lib.SMOOTH_DRY_RUN))["changed"])
        assert dry == SS.TEXELS["b", (1, 1, 1)]
        for a in range(3):
            hi = list(host.dims); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.smooth_labels, one.replace(box=((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(host.dims); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.smooth_labels, one.replace(box=(tuple(lo), tuple(hi))))
            r = [1, 1, 1]; r[a] = 4
            _refused(_lib.E_INVALID, ctx.smooth_labels, one.replace(radius=tuple(r)))
        for bad in (dict(flags=2), dict(flags=32), dict(window=(9, 8)), dict(window=(0, 256)), dict(radius=(0, 0, 0))):
            _refused(_lib.E_INVALID, ctx.smooth_labels, one.replace(**bad))
        assert volym_lib.volym_smooth_labels(None, C.byref(one.to_c()), None) == _lib.E_INVALID
        assert volym_lib.volym_smooth_labels(ctx.handle, None, None) == _lib.E_INVALID
        # nothing above changed a label, and a NULL result is accepted
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)
        assert volym_lib.volym_smooth_labels(ctx.handle, C.byref(one.to_c()), None) == _lib.OK
        assert int((ctx.read_labels().ravel() != host.labels).sum()) == dry


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = SS.SCENES["a"]()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.smooth_labels, scene.Smooth(1, dims=host.dims))
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)


# ---- 7. the Python callers ------------------------------------------------------------------------------------------------------
def test_simple_smooths_the_bonsai(oracle, volym_lib):
    from tests import common
    from volym_amd import demo, scene
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
        # a pixel that misses: nothing is smoothed, nothing is recorded
        miss = d.smooth_at(ctx, 0, 0)
        assert miss["status"] != "hit" and miss["smooth"] is None and ctx.label_history_info()["undo_steps"] == 0
        # joint, three passes: each the twin's, each an undo step
        got = d.smooth(ctx, None, 1, 3)
        assert len(got) == 3
        for res in got:
            want, r = scene.smooth_volume(vol, dims, scene.Smooth(1, dims=dims), lab)
            assert res == scene.relabel_result_dict(r) and res["changed"] > 20
            lab = want.ravel()
        assert np.array_equal(ctx.read_labels().ravel(), lab) and ctx.label_history_info()["undo_steps"] == 3
        # one segment against label 0, inside slices
        pair = scene.smooth_table([0, 2])
        want, r = scene.smooth_volume(vol, dims, scene.Smooth((2, 2, 0), give=pair, take=pair, dims=dims), lab)
        assert d.smooth(ctx, ["Canopy"], (2, 2, 0)) == [scene.relabel_result_dict(r)] and int(r["changed"]) > 20
        assert np.array_equal(ctx.read_labels(), want)
        lab = want.ravel()
        # click to smooth: the segment under the pixel against label 0 (a pixel may show unlabelled density: label 0 against itself)
        hits = []
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (100, 40)):
            p = d.smooth_at(ctx, x, y, 2)
            if p["smooth"] is None:
                continue
            hits.append(p["label"])
            pair = scene.smooth_table([0, p["label"]])
            want, r = scene.smooth_volume(vol, dims, scene.Smooth(2, give=pair, take=pair, dims=dims), lab)
            assert p["smooth"] == [scene.relabel_result_dict(r)], (x, y, p["label"])
            assert np.array_equal(ctx.read_labels(), want)
            lab = want.ravel()
        assert hits
        with pytest.raises(ValueError):
            d.smooth(ctx, None, 4)
        with pytest.raises(ValueError):
            d.smooth(ctx, ["Nobody"])


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_clis_smooth_and_write_the_labels(volym_lib, tmp_path, cli):
    """--smooth and --labels-out on `run simple` with the built-in teapot: the file holds the smoothed labels; --undo takes the pass
    back; the Python CLI also iterates"""
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
    r = subprocess.run(cmd + ["--smooth", "2:2,2,1", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    dims = (256, 256, 256)
    raw, labels_raw = synth.synth_teapot()
    before = scene.prepare_volume(labels_raw, dims, True)
    pair = scene.smooth_table([0, 2])
    want, res = scene.smooth_volume(scene.prepare_volume(raw, dims, True), dims, scene.Smooth((2, 2, 1), give=pair, take=pair, dims=dims), before)
    moved = int(res["changed"])
    assert moved > 100
    saved = np.fromfile(out, np.uint8)
    assert saved.size == 256 ** 3 and np.array_equal(scene.prepare_volume(saved, dims, True), want.ravel())
    box = [int(v) for v in res["box"]]
    if cli == "native":
        line = [l for l in r.stdout.splitlines() if l.startswith("smooth:")]
        assert len(line) == 1 and line[0].startswith("smooth: %d texels changed, box [%d,%d,%d)..[%d,%d,%d)" % tuple([moved] + box)), r.stdout
    else:
        first = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"smooth"')]
        assert len(first) == 1 and len(first[0]["smooth"]) == 1 and first[0]["smooth"][0]["changed"] == moved
        assert first[0]["smooth"][0]["box"] == [box[:3], box[3:]]
    # the pass runs before --undo, which takes it back
    r = subprocess.run(cmd + ["--smooth", "2:2,2,1", "--undo", "1", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(scene.prepare_volume(np.fromfile(out, np.uint8), dims, True), before)
    assert r.stdout.index("smooth") < r.stdout.index("undo")
    for bad in (["--smooth", "2:4"], ["--smooth", "2:1,1"], ["--smooth", "2:x"]) + ((["--smooth", "Nobody:1"],) if cli == "native" else ()):
        r = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode != 0, (bad, r.stdout[-500:])
    if cli == "python":
        r = subprocess.run(cmd + ["--smooth", "--smooth-iterations", "2"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        both = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"smooth"')]
        assert len(both) == 1 and len(both[0]["smooth"]) == 2 and both[0]["smooth"][0]["changed"] > both[0]["smooth"][1]["changed"] > 0
