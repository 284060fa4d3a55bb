"""The lasso on the device (volym_lasso_labels, volym_read_lasso_mask).

The expected labels and result are scene.lasso_volume's, the host twin of the rule, which has no cull (pinned to exact fractions and
to a plain triple loop by tests/test_lasso_host.py).  The rule is integer: there is no tolerance anywhere and nothing is left out.
After every call the result's 4128 bytes, the polygon's bit plane (every word), the labels (whole and on a sub-box), the label counts
and the state of the context are compared with the twin and with a reference context that is handed the twin's labels
(tests/test_gpu_relabel._look).  The scenes, views, polygons and requests are those of tests/lasso_scenes.py, whose properties
tests/test_lasso_host.py asserts on the twin.
"""
import ctypes as C

import numpy as np
import pytest

from tests import label_history_scenes as LH
from tests import lasso_scenes as LS
from tests import measure_scenes as MS
from tests.test_gpu_crop_box import _ctx
from tests.test_gpu_relabel import Reference, _frame_uniforms, _hand_labels, _look, _refused

pytestmark = pytest.mark.gpu

_cases = {}


def cases(oracle, dims=LS.DIMS):
    """the requests of tests/lasso_scenes.py for `dims`, built once"""
    if dims not in _cases:
        _cases[dims] = LS.cases(oracle, dims)
    return _cases[dims]


def _lasso(ctx, host, case, lasso=None):
    """the lasso on the device, its result and its mask against the twin's; the twin's labels are taken; returns the result"""
    from volym_amd import _lib, scene
    l = lasso or case.lasso
    new, want = LS.expect(host, case, l)
    got = ctx.lasso_labels(l)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    rect, words = ctx.read_lasso_mask()
    want_rect, want_words = scene.lasso_mask_words(l.points, l.view.width, l.view.height)
    assert rect == want_rect and np.array_equal(words, want_words), (case.name, "mask", rect, want_rect)
    if not l.flags & _lib.LASSO_DRY_RUN:
        host.labels = new
    return got


# ---- 1. every request, both layouts, before any cut and under cuts ----------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(LS.SCENES))
def test_every_lasso_before_any_cut(oracle, volym_lib, layout, which):
    host = LS.SCENES[which]()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(cases(oracle, host.dims)):
            if k:
                _hand_labels(ctx, host, original)
            got = int(_lasso(ctx, host, case)["changed"])
            assert which != "a" or got == case.count, case.name         # (the counts are scene A's)
            changed += got
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 1000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_after_each_cut(oracle, volym_lib, layout):
    host = LS.SCENES["a"]()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    all_cases = cases(oracle)
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(MS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in all_cases[step % 5::5]:
                _hand_labels(ctx, host, original)
                _lasso(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(all_cases)


@pytest.mark.parametrize("layout", [0, 1])
def test_lassos_on_top_of_each_other_then_cuts_that_move(oracle, volym_lib, layout):
    """cumulative lassos (no fresh labels in between), then masks and a crop that rewrite from the recomputed label boxes"""
    host = LS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    by_name = {c.name: c for c in cases(oracle)}
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        for name in ("bow-tie", "star, 1 <-> 2", "rect, the front half", "star, 1 <-> 2", "walk, eye inside, outside"):
            _lasso(ctx, host, by_name[name])
        _look(ctx, host, ref, "five lassos", uniforms)
        for hidden in ([7], [1, 2], None):
            host.set_cut(ctx, None, None, hidden)
            _look(ctx, host, ref, ("hidden", hidden), uniforms)
        host.set_cut(ctx, MS.BOX, MS.PLANE, [7])
        _lasso(ctx, host, by_name["rect into the label the cuts hide"])
        _lasso(ctx, host, by_name["1024-vertex walk"])
        _look(ctx, host, ref, "lassos under all three cuts", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "all lifted", uniforms)


def test_the_mask_read_back_is_the_twins_in_every_word(oracle, volym_lib):
    """the plane of every polygon (the helper above compares every word after every call), the refusals of the read, and a rect that
    shrinks: the plane is the latest call's"""
    from volym_amd import _lib, scene
    host = LS.SCENES["a"]()
    view = LS.view(oracle, "pose", host.dims)
    with _ctx(0) as ctx:
        host.upload(ctx)
        _refused(_lib.E_STATE, ctx.read_lasso_mask)                     # no lasso yet
        dry = _lib.LASSO_DRY_RUN
        for name, points in LS.POLYGONS.items():
            l = scene.Lasso(points or LS.walk(), view, flags=dry, to=LS.every(7), dims=host.dims)
            _lasso(ctx, host, LS.Case(name, l, None))
            rect, words = ctx.read_lasso_mask()
            assert rect == scene.lasso_rect(l)
            if name in ("sliver", "off screen"):
                assert not words.any()
        # wide frames: more than one wave per row, a last word that is partly past the rect, vertices far off screen
        wide = view.replace(width=1000, height=40)
        for points in ([(3, 1), (997, 5), (500, 39)], [(-100000, -7), (70, 20), (130, 10), (1000000, 900), (200, 39), (64, 39)], [(0, 0), (65, 0), (65, 40), (0, 40)]):
            _lasso(ctx, host, LS.Case("wide", scene.Lasso(points, wide, flags=dry, to=LS.every(7), dims=host.dims), None))
        rect = (C.c_uint32 * 4)()
        few = (C.c_uint32 * 4)()
        assert volym_lib.volym_read_lasso_mask(ctx.handle, rect, few, 4) == _lib.E_INVALID          # too small
        assert volym_lib.volym_read_lasso_mask(ctx.handle, None, None, 0) == _lib.E_INVALID
        assert volym_lib.volym_read_lasso_mask(None, rect, None, 0) == _lib.E_INVALID
        assert volym_lib.volym_read_lasso_mask(ctx.handle, rect, None, 0) == _lib.OK and tuple(rect) == (0, 0, 65, 40)
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)


# ---- 2. dry runs, no-ops and the surface pass -----------------------------------------------------------------------------------
def test_a_dry_run_changes_nothing_and_only_a_real_lasso_makes_a_surface_stale(oracle, volym_lib):
    from volym_amd import _lib, scene
    host = LS.SCENES["a"]()
    uniforms = _frame_uniforms(oracle)
    by_name = {c.name: c for c in cases(oracle)}
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
        assert int(_lasso(ctx, host, by_name["star, dry run"])["changed"]) > 50 and np.array_equal(host.labels, before)
        for name in ("identity table", "empty box", "sliver (empty mask)", "off screen", "frame, in front of the volume"):
            assert int(_lasso(ctx, host, by_name[name])["changed"]) == 0
        _look(ctx, host, ref, "after a dry run and no-ops", uniforms)
        ctx.surface_faces_pass()                                        # still the surface of the scene as it stands
        assert ctx.read_surface_faces(total).tobytes() == faces
        real = by_name["star, dry run"].lasso.replace(flags=0)
        assert int(_lasso(ctx, host, by_name["star, dry run"], real)["changed"]) > 50
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        _look(ctx, host, ref, "after the real lasso", uniforms)


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

    def lasso(self, case, look=True):
        old = self.host.labels.copy()
        got = _lasso(self.ctx, self.host, case)
        if not case.lasso.flags & 16:
            self.twin.record(old, self.host.labels, box=case.lasso.box)
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


HISTORY = ("bow-tie", "star, 1 <-> 2", "star, dry run", "walk, eye inside, outside", "off screen", "star, a sub-box")


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "ragged"])
def test_lassos_undone_and_redone(oracle, volym_lib, layout, which):
    from volym_amd import _lib
    host = LS.SCENES[which]()
    by_name = {c.name: c for c in cases(oracle, host.dims)}
    start = host.labels.copy()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LH.BIG, bool(layout), ref, _frame_uniforms(oracle))
        results = [run.lasso(by_name[name]) for name in HISTORY]
        steps = [r for r, name in zip(results, HISTORY) if int(r["changed"]) and name != "star, dry run"]
        # a lasso that changes a texel is one step; a dry run and a no-op are none (the last lasso finds its sub-box cut already
        # where the one before it reached)
        assert len(steps) >= 3 and ctx.label_history_info()["undo_steps"] == len(steps)
        for r in reversed(steps):
            assert run.swap(False).tobytes() == LH.swapped(r).tobytes()
        assert np.array_equal(host.labels, start)
        _refused(_lib.E_STATE, ctx.undo_labels)
        for r in steps:
            assert run.swap(True).tobytes() == r.tobytes()
        _refused(_lib.E_STATE, ctx.redo_labels)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_budget_one_record_short_of_the_lassos_step_gives_the_history_up(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = LS.SCENES["a"]()
    by_name = {c.name: c for c in cases(oracle)}
    small, big = by_name["frame, a slab one texel thick"], by_name["star"]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        run = Run(ctx, host, LH.BIG, bool(layout), ref, _frame_uniforms(oracle))
        run.lasso(small, look=False)
        first = ctx.label_history_info()["next_undo_records"]
        records = scene.label_chunks_changed(host.dims, host.labels, LS.expect(host, big)[0], bool(layout))
        assert 0 < first < records - 1
        ctx.label_history(20 * (records - 1))                           # the first step still fits
        run.twin.set_budget(20 * (records - 1))
        run.same_info("a smaller budget")
        assert ctx.label_history_info()["undo_steps"] == 1
        run.lasso(big)                                                  # carried out, and the whole history is given up
        info = ctx.label_history_info()
        assert info["lost"] == 1 and info["undo_steps"] == 0 and info["used_bytes"] == 0
        _refused(_lib.E_STATE, ctx.undo_labels)
    host = LS.SCENES["a"]()
    records = scene.label_chunks_changed(host.dims, host.labels, LS.expect(host, big)[0], bool(layout))
    with _ctx(layout) as ctx:
        host.upload(ctx)
        run = Run(ctx, host, 20 * records, bool(layout))                # one record more: the step is kept
        run.lasso(big)
        assert ctx.label_history_info()["lost"] == 0 and ctx.label_history_info()["next_undo_records"] == records


@pytest.mark.parametrize("layout", [0, 1])
def test_a_volume_whose_chunks_span_rows_and_slices(volym_lib, layout):
    """5 x 3 x 9: a slice is smaller than a chunk, so a linear chunk spans up to four rows and two slices and the last one is partial.
    The triangle and its OUTSIDE twin with the history off and on, then one undo; result, mask and all 135 labels against the twin
    after each call"""
    host = LS.scene_small()
    original = host.labels.copy()
    with _ctx(layout) as ctx:
        host.upload(ctx)
        for budget in (0, LH.BIG):
            ctx.label_history(budget)
            for case in LS.small_cases():
                _hand_labels(ctx, host, original)
                got = _lasso(ctx, host, case)
                assert 0 < int(got["changed"]) < original.size, case.name
                assert np.array_equal(ctx.read_labels().ravel(), host.labels), (case.name, budget)
                if budget:
                    undone = ctx.undo_labels()
                    assert undone.tobytes() == LH.swapped(got).tobytes(), case.name
                    assert np.array_equal(ctx.read_labels().ravel(), original), case.name


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(oracle, volym_lib):
    from volym_amd import _lib, scene
    host = LS.SCENES["a"]()
    view = LS.view(oracle, "pose", host.dims)
    star = scene.Lasso(LS.STAR, view, to=LS.every(7), dims=host.dims)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.lasso_labels, star)                  # no volume
        host.upload(ctx, labels=False)
        _refused(_lib.E_STATE, ctx.lasso_labels, star)                  # no labels
        other = (host.dims[0] + 1, host.dims[1], host.dims[2])
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)
        _refused(_lib.E_STATE, ctx.lasso_labels, star)                  # labels of other dimensions
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        _refused(_lib.E_STATE, ctx.read_lasso_mask)                     # a refused call leaves no mask
        dry = int(ctx.lasso_labels(star.replace(flags=_lib.LASSO_DRY_RUN))["changed"])
        assert dry == LS.COUNTS["star"]
        for a in range(3):
            hi = list(host.dims); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.lasso_labels, star.replace(box=((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(host.dims); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.lasso_labels, star.replace(box=(tuple(lo), tuple(hi))))
        for bad in (dict(flags=2), dict(flags=64), dict(window=(9, 8)), dict(window=(0, 256)), dict(points=LS.STAR[:2]), dict(points=LS.STAR[:3] + [(2 ** 20 + 1, 0)]),
                    dict(view=view.replace(depth=(0, 9))), dict(view=view.replace(depth=(9, 8))), dict(view=view.replace(width=0)), dict(view=view.replace(height=16385)),
                    dict(view=view.replace(c=(2 ** 46, 0, 1))), dict(view=view.replace(m=((1, 2, -2 ** 31), (0, 0, 0), (0, 0, 0))))):
            _refused(_lib.E_INVALID, ctx.lasso_labels, star.replace(**bad))
        c = star.to_c()
        c.n_points = 1025
        assert volym_lib.volym_lasso_labels(ctx.handle, C.byref(c), None) == _lib.E_INVALID
        assert volym_lib.volym_lasso_labels(None, C.byref(star.to_c()), None) == _lib.E_INVALID
        assert volym_lib.volym_lasso_labels(ctx.handle, None, None) == _lib.E_INVALID
        # nothing above changed a label, and a NULL result is accepted
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)
        assert volym_lib.volym_lasso_labels(ctx.handle, C.byref(star.to_c()), None) == _lib.OK
        assert int((ctx.read_labels() == 7).sum()) == dry


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = LS.SCENES["a"]()
    star = scene.Lasso(LS.STAR, LS.view(oracle, "pose", host.dims), to=LS.every(7), dims=host.dims)
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.lasso_labels, star)
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)


# ---- 5. the Python callers ------------------------------------------------------------------------------------------------------
def test_simple_cuts_the_bonsai(oracle, volym_lib):
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
    poly = [(60, 20), (110, 25), (100, 70), (55, 60)]
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        d.compute_pass(ctx)
        d.history(ctx, 16)
        view = scene.lasso_view(state.camera_uniforms(), 160, 96, dims)
        # the canopy under the polygon becomes a new segment: one step
        got = d.lasso(ctx, poly, "Cut", over=["Canopy"])
        cut = next(s for s in d._segments if s["name"] == "Cut")["label_value"]
        want, res = scene.lasso_volume(vol, dims, scene.Lasso(poly, view, to={2: cut}, dims=dims), lab)
        assert got == scene.relabel_result_dict(res) and got["changed"] > 200
        assert np.array_equal(ctx.read_labels(), want) and ctx.label_history_info()["undo_steps"] == 1
        lab = want.ravel()
        # keep only what is under the lasso: everything else is erased
        got = d.lasso_erase(ctx, poly, outside=True)
        want, res = scene.lasso_volume(vol, dims, scene.Lasso(poly, view, flags=_lib.LASSO_OUTSIDE, to=LS.every(0), dims=dims), lab)
        assert got == scene.relabel_result_dict(res) and got["changed"] > 200 and np.array_equal(ctx.read_labels(), want)
        assert d.undo(ctx)["changed"] == int(res["changed"]) and np.array_equal(ctx.read_labels().ravel(), lab)
        # a slab behind the surface under the first vertex
        hit = None
        for first in ((80, 48), (80, 30), (80, 60), (70, 40)):
            p = d.lasso_to_pick(ctx, [first, (120, 20), (120, 80), (40, 80), (40, 20)], "Slab", 6)
            if p["relabel"] is not None:
                hit = p
                break
        assert hit is not None and hit["relabel"]["changed"] > 20
        slab = next(s for s in d._segments if s["name"] == "Slab")["label_value"]
        t = [2 * v + 1 for v in hit["texel"]]
        front = (sum(view.m[2][a] * t[a] for a in range(3)) + view.c[2]) * 2.0 ** -view.scale_log2
        deep = scene.lasso_view_depth(view, front, front + 6.0 / 64)
        want, res = scene.lasso_volume(vol, dims, scene.Lasso([first, (120, 20), (120, 80), (40, 80), (40, 20)], deep, to=LS.every(slab), dims=dims), lab)
        assert hit["relabel"] == scene.relabel_result_dict(res) and np.array_equal(ctx.read_labels(), want)
        assert int(res["changed"]) < int((lab != slab).sum()) // 2                            # most of the volume lies behind the slab
        with pytest.raises(ValueError):
            d.lasso(ctx, poly[:2], "Cut")


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_clis_lasso_and_write_the_frame_and_the_labels(volym_lib, tmp_path, cli):
    """--lasso and --labels-out on `run simple` with the built-in teapot: the file holds the cut labels and the picture is written
    after the cut; --undo takes it back; the Python CLI also keeps only what is under the lasso"""
    import json
    import os
    import subprocess
    import sys
    from volym_amd import _lib, image, scene, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    out = str(tmp_path / "labels.raw")
    shot = str(tmp_path / ("a.png" if cli == "python" else "a.ppm"))
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", shot] if cli == "python" else \
          [os.path.join(root, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", shot]
    poly = [(50, 20), (82, 20), (82, 85), (50, 85)]
    arg = "50,20/82,20/82,85/50,85:2,3,4:0"
    r = subprocess.run(cmd + ["--lasso", arg, "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    assert os.path.getsize(shot) > 1000, "the picture is written after the cut"
    dims = (256, 256, 256)
    raw, labels_raw = synth.synth_teapot()
    before = scene.prepare_volume(labels_raw, dims, True)
    state = scene.State.with_parameters(160 / 90, scene.StateParameters())
    state.update()
    view = scene.lasso_view(state.camera_uniforms(), 160, 90, dims)
    want, res = scene.lasso_volume(scene.prepare_volume(raw, dims, True), dims, scene.Lasso(poly, view, to={2: 0, 3: 0, 4: 0}, dims=dims), before)
    moved = int(res["changed"])
    assert moved > 1000
    saved = np.fromfile(out, np.uint8)
    assert saved.size == 256 ** 3 and np.array_equal(scene.prepare_volume(saved, dims, True), want.ravel())
    box = [int(v) for v in res["box"]]
    if cli == "native":
        line = [l for l in r.stdout.splitlines() if l.startswith("lasso:")]
        assert len(line) == 1 and line[0].startswith("lasso: %d texels changed, box [%d,%d,%d)..[%d,%d,%d)" % tuple([moved] + box)) and \
            "label 0: -0 +%d" % moved in line[0], r.stdout
    else:
        first = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"lasso"')]
        assert len(first) == 1 and first[0]["lasso"]["changed"] == moved and first[0]["lasso"]["arrived"] == {"0": moved}
        assert first[0]["lasso"]["box"] == [box[:3], box[3:]]
    # the lasso runs before --undo, which takes it back
    r = subprocess.run(cmd + ["--lasso", arg, "--undo", "1", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(scene.prepare_volume(np.fromfile(out, np.uint8), dims, True), before)
    assert r.stdout.index("lasso") < r.stdout.index("undo")
    for bad in (["--lasso", "1,2/3,4:1:0"], ["--lasso", "1,2/3,4/5,6:1"], ["--lasso", "1,2/3,4/5:1:0"], ["--lasso", "1,2/3,4/5,6:Nobody:0"]):
        r = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode != 0, (bad, r.stdout[-500:])
    if cli == "python":
        r = subprocess.run(cmd + ["--lasso", arg, "--lasso-outside", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        want, res = scene.lasso_volume(scene.prepare_volume(raw, dims, True), dims, scene.Lasso(poly, view, flags=_lib.LASSO_OUTSIDE, to={2: 0, 3: 0, 4: 0}, dims=dims), before)
        assert int(res["changed"]) > 1000
        assert np.array_equal(scene.prepare_volume(np.fromfile(out, np.uint8), dims, True), want.ravel())
