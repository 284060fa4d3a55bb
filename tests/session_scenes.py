"""Editing sessions: one context, every label editor, the passes whose snapshots they read, cuts, undo and redo, in the order someone
segmenting a volume works in.  Shared by tests/test_session_host.py (which runs every script on the host model alone and asserts the
conditions the device test relies on) and tests/test_gpu_session.py (which drives a context beside the model).

A script is a list of Steps over one scene.  A Session drives the host model, and a context beside it when it is given one, as
tests/test_gpu_label_history.Run does for relabels.  The model is built only from what the project already pins to plain loops:
tests/test_gpu_slice.Host (volume, labels, table, cut state), scene.LabelHistory (the journal), the editors' twins through the
`expect` functions of their scene modules and the passes' twins for the snapshots.  A pass stores the twin's result of that moment;
a later edit that reads a map is given the stored one, stale or not, with the stored request's box.  Every request comes from the
pools of the editors' own scene modules, which the twins and the device agree on in isolation: a failure here is a failure of the
combination.

What each set-up call does to the history and the snapshots is include/volym_hip.h's: volym_set_labels clears the steps and keeps
budget, counters and every snapshot (it resets the mask, which the caller sends again); volym_set_segment_importances, the cuts and
the frames touch neither; volym_label_history(0) drops everything, counters included.

The hazards the hand-written scripts contain (hazards() states each as a predicate over a script's trace):
  1. a smoothing pass (not dry) that changes texels, straight before undos that reach a step of another kind; a dry smoothing pass
     straight before an undo of a step of another kind; a smoothing pass with the history off, then the history switched on and a
     journalled brush.  (An undo straight after a journalled smoothing pass takes back that pass: the step of another kind is the
     next undo's.  The dry pass leaves the vote's records in the staging area and no step, so the undo after it is another kind's.)
  2. an undo or redo of a step of each of the six kinds; an undo of a fill step and of a flood step under other cuts than those
     they were recorded under.
  3. a new edit of kind X after two undos of steps of kinds Y and Z, which drops the redo steps.
  4. a distance pass, then a nearest and a geodesic pass on boxes of other sizes (one larger, one smaller), then a distance-band
     relabel by the old map; a components pass, the other three passes, then a relabel by the old ids.
  5. the first edit into a hidden label without voxels, in a context that never cut: by a brush in one script, by a flood in
     another; the next step is an edit of another kind.
  6. a dry run of every kind between real edits.
  7. a fill or flood by a snapshot taken before an undo that changed the seeds' labels.
"""
import os

import numpy as np

from tests import brush_scenes as BS
from tests import components_scenes as CS
from tests import distance_scenes as DS
from tests import geodesic_scenes as GS
from tests import lasso_scenes as LS
from tests import measure_scenes as MS
from tests import nearest_scenes as NS
from tests import relabel_scenes as RS
from tests import smooth_scenes as SS

EDITORS = ("relabel", "brush", "lasso", "smooth", "fill", "flood")
PASSES = ("components", "distance", "nearest", "geodesic")
BIG = 1 << 20
SEEDS = [16, 62, 72] + [int(x) for x in os.environ.get("VOLYM_EXTRA_SEEDS", "").split()]
LIFTED = (None, None, None)


class Step:
    """one step of a script: op is "cut", "pass", "edit", "undo", "redo", "budget", "hand", "table", "frames" or "look"."""

    def __init__(self, op, *args, tag=None, noop=False, oracle=False):
        self.op, self.args, self.tag, self.noop, self.oracle = op, args, tag, noop, oracle
        self.derive = None              # a budget step: the function of the records it was derived by

    def describe(self):
        if self.op == "edit":
            return "edit %s: %s" % (self.args[0], self.args[1].name)
        if self.op == "pass":
            return "pass %s over %r" % (self.args[0], self.args[1].box)
        if self.op == "cut":
            return "cut box %r plane %r hidden %r" % self.args
        if self.op == "hand":
            return "hand labels: %s" % self.args[1]
        if self.op == "budget":
            return "budget %s" % (self.args[0] if isinstance(self.args[0], int) else "derived")
        if self.op == "frames":
            return "frames %d" % self.args[0]
        return self.op


def cut(box=None, plane=None, hidden=None):
    return Step("cut", box, plane, hidden)


def run_pass(kind, request):
    return Step("pass", kind, request)


def edit(kind, case, tag=None, noop=False):
    return Step("edit", kind, case, tag=tag, noop=noop)


def undo():
    return Step("undo")


def redo():
    return Step("redo")


def budget(b):
    """b: bytes, or a function of {tag: records of that edit in this layout} (resolved by Script.steps)"""
    return Step("budget", b)


def hand(fn, name):
    """set_labels again with fn(the labels as they stand)"""
    return Step("hand", fn, name)


def table(t):
    return Step("table", t)


def frames(n):
    return Step("frames", n)


def look(oracle=False):
    return Step("look", oracle=oracle)


class _NoContext:
    """stands in for the context in a run of the model alone: every call is accepted and does nothing"""

    def __getattr__(self, name):
        return lambda *a, **kw: None


def _inside(box, outer):
    return all(a >= b for a, b in zip(box[0], outer[0])) and all(a <= b for a, b in zip(box[1], outer[1]))


def _volume(box):
    return int(np.prod([max(0, b - a) for a, b in zip(*box)]))


def dry_flag(kind):
    from volym_amd import _lib
    return {"relabel": _lib.RELABEL_DRY_RUN, "brush": _lib.BRUSH_DRY_RUN, "lasso": _lib.LASSO_DRY_RUN, "smooth": _lib.SMOOTH_DRY_RUN,
            "fill": NS.FILL_DRY_RUN, "flood": GS.FLOOD_DRY_RUN}[kind]


def request_of(kind, case):
    return getattr(case, kind) if kind in ("relabel", "brush", "lasso", "smooth", "fill", "flood") else None


def snapshots_read(kind, case):
    """{snapshot kind: the pass request the case was written for} of an edit"""
    if kind == "relabel":
        return {k: getattr(case, k) for k in ("components", "distance") if getattr(case, k) is not None}
    if kind == "fill":
        return {"nearest": case.distance}
    if kind == "flood":
        return {"geodesic": case.geodesic}
    return {}


class Session:
    """the host model of one session, and the context driven beside it (ctx None: the model alone).  trace holds one record per
    step: what the hazards and the conditions of tests/test_session_host.py are stated over."""

    def __init__(self, host, bricked, ctx=None, ref=None, uniforms=None, oracle=None, in_flight=1, what=""):
        from volym_amd import scene
        self.host, self.bricked, self.ctx, self.ref, self.uniforms, self.oracle = host, bool(bricked), ctx, ref, uniforms, oracle
        self.in_flight, self.what = in_flight, what
        self.null = _NoContext()
        self.twin = scene.LabelHistory(0, host.dims, bricked)
        self.snaps = {}                             # kind -> (request, the twin's result, the step it was taken at)
        self.cut_now = LIFTED
        self.trace = []
        if ctx is not None and uniforms is not None:
            ctx.update(*uniforms)
            for _ in range(3 if in_flight > 1 else 0):      # both slots hold a frame before the first step
                ctx.compute_pass()

    # ---- the walk -------------------------------------------------------------------------------------------------------------------
    def run(self, steps, upto=None, each=None):
        for k, step in enumerate(steps if upto is None else steps[:upto + 1]):
            try:
                self.apply(step)
                if each is not None:
                    each(k, step)
            except Exception as e:                      # (the step, and how to run the script up to it alone)
                raise AssertionError("%s, step %d (%s); the prefix alone: VOLYM_SESSION_UPTO=%d; %s: %s" % (self.what, k, step.describe(), k, type(e).__name__, e)) from e
        return self

    def finish(self):
        """the end of every script: all cuts lifted, a look, then everything undone (the checks after every step compare the labels)"""
        tail = [cut(None, None, None), look()] if self.cut_now != LIFTED else [] if self.trace and self.trace[-1]["op"] == "look" else [look()]
        for step in tail + [undo()] * self.twin.info()["undo_steps"] + [undo()]:
            try:
                self.apply(step)
            except Exception as e:
                raise AssertionError("%s, after the script (%s); %s: %s" % (self.what, step.describe(), type(e).__name__, e)) from e
        assert self.trace[-1]["refused"] and self.twin.info()["undo_steps"] == 0
        return self

    def apply(self, step):
        rec = {"k": len(self.trace), "op": step.op, "kind": None, "tag": step.tag, "noop": step.noop, "changed": 0, "dry": False, "refused": False,
               "recorded": False, "records": 0, "reads": {}, "cut": self.cut_now}
        getattr(self, "_" + step.op)(rec, *step.args, **({"oracle": step.oracle} if step.op == "look" else {}))
        rec["info"] = self.twin.info()
        rec["labels"] = self.host.labels                    # (every edit replaces the array: this is the state after the step)
        self.trace.append(rec)
        if self.ctx is not None and step.op not in ("look", "frames"):
            self.cheap(step.describe())
            if self.in_flight > 1 and step.op in ("edit", "undo", "redo"):
                for _ in range(3):
                    self.ctx.compute_pass()
        return rec

    def cheap(self, what):
        """history info, every label and the label counts of the context against the model"""
        got, want = self.ctx.label_history_info(), self.twin.info()
        assert got == want, (what, "history info", got, want)
        nx, ny, nz = self.host.dims
        labels = self.ctx.read_labels()
        want = self.host.labels.reshape(nz, ny, nx)
        assert np.array_equal(labels, want), (what, "labels", int((labels != want).sum()), np.argwhere(labels != want)[:4].tolist())
        assert self.ctx.label_counts().tolist() == np.bincount(self.host.labels, minlength=256).tolist(), (what, "label counts")

    # ---- the steps ------------------------------------------------------------------------------------------------------------------
    def _cut(self, rec, box, plane, hidden):
        rec["never_cut"] = not self.host.ever_cut
        self.host.set_cut(self.ctx if self.ctx is not None else self.null, box, plane, hidden)
        self.cut_now = rec["cut"] = (box, plane, tuple(hidden) if hidden else None)

    def _pass(self, rec, kind, request):
        want = {"components": CS.expect, "distance": DS.expect, "nearest": NS.expect, "geodesic": GS.expect}[kind](self.host, request)
        self.snaps[kind] = (request, want, rec["k"])
        rec.update(kind=kind, box=request.box, request=request)
        if self.ctx is None:
            return
        before = self.ctx.read_rgba8() if self.in_flight > 1 else None
        if kind == "components":
            from tests.test_gpu_components import _run, _same
        elif kind == "distance":
            from tests.test_gpu_distance import _run, _same
        elif kind == "nearest":
            from tests.test_gpu_nearest import _run, _same
        else:
            from tests.test_gpu_geodesic import _run, _same
        _same((kind, request.box), _run(self.ctx, request), want)
        if before is not None:
            assert np.array_equal(self.ctx.read_rgba8(), before), "the frame read before the pass changed"

    def expect(self, kind, case):
        """the twin's (new labels [flat], result, request, the box its journal's staging area is sized by, {snapshot kind: step taken})"""
        from volym_amd import scene
        host, reads = self.host, {}
        stored = {}
        for k, written_for in snapshots_read(kind, case).items():
            assert k in self.snaps, "the script reads a %s snapshot that no pass has taken" % k
            stored[k] = self.snaps[k]
            reads[k] = stored[k][2]
            assert _inside(request_of(kind, case).box, stored[k][0].box), "the script's %s reaches outside the latest %s pass's box" % (kind, k)
        if kind == "relabel":
            c = RS.Case(case.name, case.relabel, components=stored["components"][0] if "components" in stored else None,
                        distance=stored["distance"][0] if "distance" in stored else None, pick=case.pick)
            new, want, r = RS.expect(host, c, {k: stored[k][1] if k in stored else None for k in ("components", "distance")})
            return new, want, r, r.box, reads
        if kind == "brush":
            new, want = BS.expect(host, case)
            return new, want, case.brush, scene.brush_box(case.brush, host.dims), reads
        if kind == "lasso":
            new, want = LS.expect(host, case)
            return new, want, case.lasso, case.lasso.box, reads
        if kind == "smooth":
            new, want = SS.expect(host, case)
            return new, want, case.smooth, case.smooth.box, reads
        if kind == "fill":
            new, want = NS.fill_expect(host, NS.FillCase(case.name, stored["nearest"][0], case.fill), stored["nearest"][1])
            return new, want, case.fill, case.fill.box, reads
        assert kind == "flood", kind
        new, want = GS.flood_expect(host, GS.FloodCase(case.name, stored["geodesic"][0], case.flood), stored["geodesic"][1])
        return new, want, case.flood, case.flood.box, reads

    def _edit(self, rec, kind, case):
        from volym_amd import scene
        old = self.host.labels
        new, want, request, box, reads = self.expect(kind, case)
        dry = bool(request.flags & dry_flag(kind))
        rec.update(kind=kind, name=case.name, dry=dry, reads=reads, would=int(want["changed"]), left=np.array(want["left"]), arrived=np.array(want["arrived"]))
        if self.ctx is not None:
            got = getattr(self.ctx, {"relabel": "edit_labels"}.get(kind, kind + "_labels"))(request)
            self.same_result(case.name, got, want)
            if kind == "lasso":                             # the polygon's bit plane, every word
                rect, words = self.ctx.read_lasso_mask()
                want_rect, want_words = scene.lasso_mask_words(request.points, request.view.width, request.view.height)
                assert rect == want_rect and np.array_equal(words, want_words), (case.name, "mask", rect, want_rect)
        if dry:                                             # (the labels a twin returns for a dry run are not taken)
            return
        new = np.ascontiguousarray(new, np.uint8)
        rec["changed"] = int((new != old).sum())
        assert rec["changed"] == int(want["changed"]), (case.name, "the twin's count and its labels disagree")
        rec["records"] = scene.label_chunks_changed(self.host.dims, old, new, self.bricked)
        rec["journal_box"] = box
        self.host.labels = new
        undoable = {id(st): st["kind"] for st in self.twin.steps[:self.twin.cursor]}
        rec["recorded"] = self.twin.record(old, new, box=box)
        rec["evicted"] = [kind for i, kind in undoable.items() if rec["recorded"] and i not in {id(st) for st in self.twin.steps}]
        if rec["recorded"]:
            self.twin.steps[self.twin.cursor - 1].update(kind=kind, cut=self.cut_now, k=rec["k"])

    @staticmethod
    def same_result(what, got, want):
        for k in ("changed", "left", "arrived", "box"):
            assert np.array_equal(got[k], want[k]), (what, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
        assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, what

    def _swap(self, rec, redo):
        from volym_amd import _lib
        what = "redo" if redo else "undo"
        try:
            labels, want = (self.twin.redo if redo else self.twin.undo)(self.host.labels)
        except ValueError:
            rec["refused"] = True
            if self.ctx is not None:
                try:
                    (self.ctx.redo_labels if redo else self.ctx.undo_labels)()
                except _lib.VolymError as e:
                    assert e.code == _lib.E_STATE, (what, "refused with", e.code)
                else:
                    raise AssertionError("%s: the twin refuses, the context does not" % what)
            return
        step = self.twin.steps[self.twin.cursor - 1 if redo else self.twin.cursor]
        rec.update(kind=step["kind"], of=step["k"], recorded_under=step["cut"], changed=int(want["changed"]), left=np.array(want["left"]),
                   arrived=np.array(want["arrived"]))
        if self.ctx is not None:
            self.same_result(what, self.ctx.redo_labels() if redo else self.ctx.undo_labels(), want)
        self.host.labels = labels

    def _undo(self, rec):
        self._swap(rec, False)

    def _redo(self, rec):
        self._swap(rec, True)

    def _budget(self, rec, b):
        assert isinstance(b, int), "Script.steps resolves the derived budgets"
        kept = {id(st): st["kind"] for st in self.twin.steps}
        self.twin.set_budget(b)
        rec["evicted"] = [kind for i, kind in kept.items() if b and i not in {id(st) for st in self.twin.steps}]
        if self.ctx is not None:
            self.ctx.label_history(b)

    def _hand(self, rec, fn, name):
        """as tests/test_gpu_relabel._hand_labels: a new label volume, the table and the mask again"""
        self.host.labels = np.ascontiguousarray(fn(self.host.labels), np.uint8).copy()
        self.twin.clear()
        if self.ctx is not None:
            self.ctx.set_labels(self.host.labels, self.host.dims)
            self.ctx.set_segment_importances(self.host.table)
            if self.host.cut is not None and not np.asarray(self.host.cut["visible"]).all():
                self.ctx.set_segment_visibility(self.host.cut["visible"])

    def _table(self, rec, t):
        self.host.table = np.ascontiguousarray(t, np.uint8)
        if self.ctx is not None:
            self.ctx.set_segment_importances(self.host.table)

    def _frames(self, rec, n):
        if self.ctx is not None:
            for _ in range(n):
                self.ctx.compute_pass()

    def _look(self, rec, oracle=False):
        if self.ctx is None:
            return
        from tests.test_gpu_relabel import _look
        what = (self.what, "look at step %d" % rec["k"])
        if self.in_flight > 1:
            shown = []
            for _ in range(3):                      # both slots, with no update in between
                self.ctx.compute_pass()
                shown.append(self.ctx.read_rgba8())
            r = self.ref.at(self.host)
            r.update(*self.uniforms)
            r.compute_pass()
            want = r.read_rgba8()
            for k, f in enumerate(shown):
                assert np.array_equal(f, want), (what, "frame", k, "differs from the context that was handed the labels")
        _look(self.ctx, self.host, self.ref, what, self.uniforms)
        if oracle and self.oracle is not None:
            self.against_oracle(self.ctx, what)
        if self.uniforms is not None:
            self.ctx.update(*self.uniforms)         # (the view the frames between the steps show)

    def against_oracle(self, ctx, what):
        """one frame each in density and in importance mode against oracle.render on the model's labels and cuts: the bar is
        tests/test_gpu_crop_box._near's, and three standing frames are bit-equal"""
        from tests.test_gpu_crop_box import H, PARAMS, W, _near, _three, _uniforms
        from tests.test_gpu_relabel import POSE
        from volym_amd import scene
        host = self.host
        vol = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
        imp = scene.cut_volume(host.table[host.labels], host.dims, host.cut, host.labels)
        for mode in ("base", "straight"):
            cam, par, cu, pu = _uniforms(self.oracle, W, H, POSE, **PARAMS[mode])
            got = _three(ctx, what + (mode,), cu, pu)
            f32, u8, _ = self.oracle.render(vol, imp, host.dims, host.lut, cam, par, W, H)
            _near(what + (mode, "oracle"), got, (f32, u8))


# ---- scripts -------------------------------------------------------------------------------------------------------------------------
class Script:
    """name, the scene, the steps as a function of the oracle module (the lasso's views are its cameras'), and what its description
    claims of the twin's counters: {"evictions": at least, "lost": exactly}"""

    def __init__(self, name, scene, build, claims):
        self.name, self.scene, self.build, self.claims = name, scene, build, claims
        self._steps = {}

    def host(self):
        return self.scene()

    def steps(self, O, bricked):
        """the steps with the derived budgets resolved for this layout: the records are those of a run of the model with a budget
        that holds everything (the host test asserts that the real run journals the same)"""
        bricked = bool(bricked)
        if bricked not in self._steps:
            raw = self.build(O)
            for k, st in enumerate(raw):                # one after the other: a budget may decide what later steps journal
                if st.op == "budget" and not isinstance(st.args[0], int):
                    plenty = [Step("budget", BIG) if s.op == "budget" and not isinstance(s.args[0], int) else s for s in raw]
                    trace = Session(self.host(), bricked).run(plenty).trace
                    raw[k] = Step("budget", int(st.args[0]({t["tag"]: t["records"] for t in trace if t["tag"] is not None})))
                    raw[k].derive = st.args[0]
            self._steps[bricked] = raw
        return self._steps[bricked]

    def model(self, O, bricked):
        """a run of the model alone"""
        return Session(self.host(), bricked, what=self.name).run(self.steps(O, bricked))


def _by_name(cases):
    return {c.name: c for c in cases}


def _pools(O, dims=MS.DIMS):
    return {"relabel": _by_name(RS.cases_a()), "brush": _by_name(BS.cases(dims)), "lasso": _by_name(LS.cases(O, dims)), "smooth": _by_name(SS.cases(dims)),
            "fill": _by_name(NS.fill_cases()), "flood": _by_name(GS.flood_cases())}


def _request(pool, name):
    return dict(pool)[name]


def working_day(O):
    """scene A, about 40 steps: every editor twice or more, every snapshot kind read, every hazard but the flood's half of 5.  The
    budget holds about four steps, so the oldest are evicted again and again, and steps of several kinds among them."""
    P = _pools(O)
    R, B, L, S, F, G = (P[k] for k in EDITORS)
    part, pieces = R["band 1..5 of a map over x 5..30, a box inside it"].distance, R["pieces 2..40 of 3 -> 6, rows"].components
    outside = R["grow 2 by 2"].distance
    seeds, flow = F["0 within 2 of a seed"].distance, G["0 within 2 steps of a seed"].geodesic
    small = _request(GS.requests(), "x 3..8 / tables 2")
    _, box, plane, hidden = MS.CUTS[7]                                  # all three
    fits = lambda r: 20 * (r["capsule"] + r["band"] + r["smooth 1"])    # noqa: E731 -- these three, or about four of the later steps
    return [
        budget(fits),
        run_pass("components", pieces),
        run_pass("distance", part),
        edit("relabel", R["table, x 3..8"], tag="table"),
        run_pass("nearest", seeds),                                     # the whole volume: larger than the distance pass's box
        run_pass("geodesic", small),                                    # x 3..8: smaller
        cut(None, None, [7]),                                           # no voxel carries 7: no byte changes, no copy is made
        edit("brush", B["capsule along x, r2 4"], tag="capsule"),       # hazard 5: into the hidden 7, in a context that never cut
        edit("relabel", R["band 1..5 of a map over x 5..30, a box inside it"], tag="band"),      # hazard 4, by the old map
        edit("brush", B["dry run"]),
        look(),
        edit("smooth", S["joint, radius 1"], tag="smooth 1"),
        undo(),                                                         # hazard 1: the pass itself ...
        undo(),                                                         # ... and the band, a relabel
        edit("lasso", L["star, a sub-box"], tag="lasso"),               # hazard 3: drops two redo steps
        edit("relabel", R["pieces 2..40 of 3 -> 6, rows"], tag="pieces"),        # hazard 4, by the old ids
        look(),
        edit("fill", F["0 within 2 of a seed"], tag="fill"),            # hazard 7: the snapshot is older than the undo of the band
        cut(box, plane, hidden),
        look(),
        undo(),                                                         # hazard 2: the fill, under cuts it was not recorded under
        edit("smooth", S["dry run"]),                                   # hazards 1 and 6: a dry vote, then an undo of a relabel
        undo(),
        redo(),
        look(),
        edit("lasso", L["star, dry run"]),
        edit("fill", F["dry run"]),
        run_pass("geodesic", flow),
        edit("flood", G["dry run"]),
        edit("flood", G["0 within 2 steps of a seed"], tag="flood"),
        cut(None, None, None),
        undo(),                                                         # hazard 2: the flood, under other cuts
        redo(),
        edit("fill", F["seeds give too"], tag="seeds give"),            # by the nearest snapshot of the session's beginning
        edit("flood", G["to renames: 1 -> 9, 2 -> 3"], tag="renames"),
        look(),
        run_pass("distance", outside),
        edit("relabel", R["pieces 0..9 of 3 within 3 of 2, dry run"]),
        edit("relabel", R["merge 1, 2 -> 4, whole"], tag="merge"),
        cut(None, None, [2]),                                           # no voxel carries 2: no byte changes
        edit("brush", B["paint the label the cuts hide"], tag="paint"), # hazard 5
        edit("smooth", S["joint, radius 2"], tag="smooth 2"),
        look(),
        budget(0),
        edit("smooth", S["joint, radius 1"]),                           # hazard 1: the history is off
        budget(fits),
        edit("brush", B["the long diagonal, r2 6"], tag="diagonal"),
        edit("lasso", L["rect, a window 100..180"], tag="rect"),
        undo(),
        undo(),
        redo(),
        table((np.arange(256) * 37 + 11) % 256),
        frames(2),
        look(),
        cut(None, None, None),
        look(oracle=True),
    ]


def give_up_and_go_on(O):
    """scene A: the budget is one record short of the large fill in the middle, which gives the history up (lost = 1); the edits of
    other kinds after it are journalled again and undone; the budget shrinks, goes to 0 and comes back, and the labels are handed
    again.  The flood's half of hazard 5 is here."""
    P = _pools(O)
    R, B, L, S, F, G = (P[k] for k in EDITORS)
    flow, seeds, inner = G["0 within 2 steps of a seed"].geodesic, F["0 and 4 to the nearest of 1, 2, 3"].distance, G["a box inside the pass's box"].geodesic
    return [
        budget(lambda r: 20 * (r["big"] - 1)),
        run_pass("geodesic", flow),
        edit("relabel", R["merge 1, 2 -> 4, whole"], tag="merge"),      # labels 1 and 2 are gone
        cut(None, None, [1]),                                           # no voxel carries 1
        edit("flood", G["0 within 2 steps of a seed"], tag="flood"),    # hazard 5: by the seeds that were, into the hidden 1
        edit("brush", B["ball of r2 25 at the origin"], tag="ball"),
        look(),
        run_pass("nearest", seeds),
        edit("fill", F["0 and 4 to the nearest of 1, 2, 3"], tag="big"),    # does not fit: the history is given up
        undo(),                                                         # refused
        edit("lasso", L["frame, a slab one texel thick"], tag="slab"),
        edit("smooth", S["joint, radius 1"], tag="smooth"),
        edit("brush", B["capsule along x, r2 4"], tag="capsule"),
        undo(),
        undo(),
        redo(),
        edit("relabel", R["swap 0 <-> 3, rows"], tag="swap"),           # drops the capsule's redo step
        redo(),                                                         # refused
        look(),
        budget(lambda r: 20 * (r["swap"] + r["smooth"])),               # shrinks: the lasso's step is evicted
        undo(),
        budget(0),
        undo(),                                                         # refused: off
        edit("brush", B["the long diagonal, r2 6"]),                    # not journalled
        budget(lambda r: 20 * (r["big"] - 1)),
        edit("smooth", S["joint, radius 2"], tag="smooth 2"),
        edit("lasso", L["bow-tie, rolled"], tag="bow-tie"),
        undo(),
        hand(lambda l: np.where(l == 7, 3, l), "7 becomes 3"),          # clears the steps
        undo(),                                                         # refused
        redo(),                                                         # refused
        run_pass("geodesic", inner),
        edit("flood", G["a box inside the pass's box"], tag="inner"),
        edit("brush", B["256 points of a random walk"], tag="walk"),
        undo(),
        undo(),
        cut(None, None, None),
        look(),
    ]


RAGGED_BOX = ((13, 3, 6), (87, 62, 70))          # aligned to 4 on no axis
RAGGED_PLANE = ((5, -3, 7), 420)


def ragged_scene():
    """relabel_scenes.scene_ragged() with the transfer function tests/test_gpu_crop_box.py renders it with against the oracle"""
    from volym_amd import scene
    host = RS.scene_ragged()
    host.lut = np.asarray(scene.default_lut(), np.uint8).reshape(-1, 4)
    return host


def ragged(O):
    """the cup scene, 97 x 80 x 71: one edit of each kind, two cuts, two undos, one redo, three looks, each against the oracle as
    well.  The fill and the flood work in scene A's dimensions, a box in the volume's first corner that holds air and shell."""
    dims = RS.RAGGED_DIMS
    R, B, L, S = _by_name(RS.cases_ragged()), _by_name(BS.cases(dims)), _by_name(LS.cases(O, dims)), _by_name(SS.cases(dims))
    F, G = _by_name(NS.fill_cases()), _by_name(GS.flood_cases())
    return [
        budget(lambda r: 20 * (r["shell"] + r["diagonal"] + r["fill"] + r["tie"])),
        edit("relabel", R["air and shell -> 3, x 40..57"], tag="shell"),
        edit("brush", B["the long diagonal, r2 6"], tag="diagonal"),
        run_pass("nearest", F["0 within 2 of a seed"].distance),
        edit("fill", F["0 within 2 of a seed"], tag="fill"),
        cut(RAGGED_BOX, None, None),
        look(oracle=True),
        edit("lasso", L["bow-tie"], tag="tie"),
        edit("smooth", S["joint, radius 1"], tag="smooth"),             # evicts the relabel
        undo(),
        undo(),
        redo(),
        cut(None, RAGGED_PLANE, [5]),
        look(oracle=True),
        run_pass("geodesic", G["0 and 4 to the seeds 1, 2, 3"].geodesic),
        edit("flood", G["0 and 4 to the seeds 1, 2, 3"], tag="flood"),  # drops the smoothing's redo step
        cut(None, None, None),
        look(oracle=True),
    ]


SCRIPTS = {}


def scripts():
    """name -> Script: the hand-written ones"""
    if not SCRIPTS:
        SCRIPTS["a working day"] = Script("a working day", RS.scene_a, working_day, {"evictions": 3, "lost": 0})
        SCRIPTS["give up and go on"] = Script("give up and go on", RS.scene_a, give_up_and_go_on, {"evictions": 1, "lost": 1})
        SCRIPTS["ragged"] = Script("ragged", ragged_scene, ragged, {"evictions": 1, "lost": 0})
    return SCRIPTS


# ---- generated scripts ---------------------------------------------------------------------------------------------------------------
def _pass_requests():
    """the pool of pass requests over scene A: those the editors' cases were written for, and the passes' own short lists"""
    out = {"components": [c.components for c in RS.cases_a() if c.components is not None] + [c for _, c in CS.requests()],
           "distance": [c.distance for c in RS.cases_a() if c.distance is not None] + [d for _, d in DS.requests()],
           "nearest": [c.distance for c in NS.fill_cases()] + [d for _, d in NS.requests()],
           "geodesic": [c.geodesic for c in GS.flood_cases()] + [g for _, g in GS.requests()]}
    return out


def generate(O, seed, n_steps=30):
    """a script over scene A drawn with numpy.random.default_rng(seed) from the pools: deterministic, and made with the host model
    alone (what has been taken, and over which box, decides where a pass must go in front of an edit; otherwise snapshots are left
    to go stale)"""
    rng = np.random.default_rng(seed)
    pools = {k: list(v.values()) for k, v in _pools(O).items()}
    busy = {k: [c for c in v if not getattr(c, "trivial", False)] for k, v in pools.items()}       # the no-ops are drawn less often
    original = RS.scene_a().labels
    passes = _pass_requests()
    budgets = [0, 20 * 300, 20 * 1200, 20 * 1200, BIG]
    cuts = [(box, plane, hidden) for _, box, plane, hidden in MS.CUTS] + [(None, None, [7]), (MS.BOX, None, [3])]
    taken = {}                                          # kind -> the box of the latest pass
    steps = [budget(20 * 1200)]
    ops = ["edit"] * 14 + ["undo"] * 4 + ["redo"] * 2 + ["cut"] * 2 + ["pass", "budget", "hand", "table", "frames"]
    while len(steps) < n_steps:
        op = ops[int(rng.integers(len(ops)))]
        if op == "edit":
            kind = EDITORS[int(rng.integers(len(EDITORS)))]
            pool = busy[kind] if rng.random() < 0.8 else pools[kind]
            case = pool[int(rng.integers(len(pool)))]
            for k, written_for in snapshots_read(kind, case).items():
                if k not in taken or not _inside(request_of(kind, case).box, taken[k]):
                    steps.append(run_pass(k, written_for))
                    taken[k] = written_for.box
            steps.append(edit(kind, case))
        elif op == "pass":
            kind = PASSES[int(rng.integers(len(PASSES)))]
            request = passes[kind][int(rng.integers(len(passes[kind])))]
            steps.append(run_pass(kind, request))
            taken[kind] = request.box
        elif op == "cut":
            steps.append(cut(*cuts[int(rng.integers(len(cuts)))]))
        elif op == "budget":
            steps.append(budget(budgets[int(rng.integers(len(budgets)))]))
        elif op == "hand":
            a, b = (int(v) for v in rng.integers(0, 8, 2))
            if a == b:
                steps.append(hand(lambda l: original, "the scene's own"))
            else:
                steps.append(hand(lambda l, a=a, b=b: np.where(l == a, b, l), "%d becomes %d" % (a, b)))
        elif op == "table":
            steps.append(table(rng.integers(0, 256, 256)))
        elif op == "frames":
            steps.append(frames(int(rng.integers(1, 4))))
        else:
            steps.append(Step(op))
    return steps


def generated(seed):
    return Script("generated, seed %d" % seed, RS.scene_a, lambda O: generate(O, seed), {})


# ---- the hazards as predicates over a trace --------------------------------------------------------------------------------------------
def _edits(trace, **kw):
    return [t for t in trace if t["op"] == "edit" and all(t.get(k) == v for k, v in kw.items())]


def _swaps(trace):
    return [t for t in trace if t["op"] in ("undo", "redo") and not t["refused"]]


def hazards(trace):
    """{hazard: True where the trace of one script contains it}; the keys are those of the module's docstring, split where a
    hazard has several parts"""
    out = {}
    after = lambda t, n=1: trace[t["k"] + n] if t["k"] + n < len(trace) else {"op": None, "kind": None, "refused": True}     # noqa: E731
    undo_of_other = lambda t: t["op"] == "undo" and not t["refused"] and t["kind"] != "smooth"                          # noqa: E731
    out["1 a pass, then undos that reach another kind"] = any(
        t["recorded"] and t["changed"] > 0 and after(t)["op"] == "undo" and after(t).get("of") == t["k"] and undo_of_other(after(t, 2))
        for t in _edits(trace, kind="smooth", dry=False))
    out["1 a dry pass, then an undo of another kind"] = any(t["would"] > 0 and undo_of_other(after(t)) for t in _edits(trace, kind="smooth", dry=True))
    out["1 a pass with the history off, then on and a journalled brush"] = any(
        t["changed"] > 0 and t["info"]["budget_bytes"] == 0 and after(t)["op"] == "budget" and after(t)["info"]["budget_bytes"] > 0
        and after(t, 2)["kind"] == "brush" and after(t, 2).get("recorded") for t in _edits(trace, kind="smooth", dry=False))
    for kind in EDITORS:
        out["2 a step of kind %s undone or redone" % kind] = any(t["kind"] == kind for t in _swaps(trace))
    for kind in ("fill", "flood"):
        out["2 a %s step undone under other cuts" % kind] = any(t["op"] == "undo" and t["kind"] == kind and t["recorded_under"] != t["cut"] for t in _swaps(trace))
    out["3 a new edit after two undos of other kinds"] = any(
        t["recorded"] and trace[t["k"] - 1]["op"] == trace[t["k"] - 2]["op"] == "undo" and not trace[t["k"] - 1]["refused"] and not trace[t["k"] - 2]["refused"]
        and len({t["kind"], trace[t["k"] - 1]["kind"], trace[t["k"] - 2]["kind"]}) == 3 and trace[t["k"] - 1]["info"]["redo_steps"] >= 2
        and t["info"]["redo_steps"] == 0 for t in _edits(trace, dry=False) if t["k"] >= 2)

    def old_snapshot(kind):
        others = [k for k in PASSES if k != kind]
        for t in _edits(trace, kind="relabel", dry=False):
            if kind not in t["reads"] or t["changed"] == 0:
                continue
            taken = trace[t["reads"][kind]]
            between = [p for p in trace[taken["k"] + 1:t["k"]] if p["op"] == "pass"]
            if kind == "distance":
                sizes = {p["kind"]: _volume(p["box"]) for p in between if p["kind"] in ("nearest", "geodesic")}
                if len(sizes) == 2 and min(sizes.values()) < _volume(taken["box"]) < max(sizes.values()):
                    return True
            elif {p["kind"] for p in between} >= set(others):
                return True
        return False

    out["4 a band of a distance map older than a larger and a smaller pass"] = old_snapshot("distance")
    out["4 ids older than the other three passes"] = old_snapshot("components")
    for kind in ("brush", "flood"):
        found = False
        for t in _edits(trace, kind=kind, dry=False):
            before = trace[t["k"] - 1]
            if before["op"] == "cut" and before.get("never_cut") and before["cut"][:2] == (None, None) and before["cut"][2]:
                counts = np.bincount(before["labels"], minlength=256)
                hidden = [l for l in before["cut"][2] if counts[l] == 0]
                nxt = after(t)
                found = found or (len(hidden) == len(before["cut"][2]) and int(t["arrived"][hidden].sum()) > 0 and nxt["op"] == "edit"
                                  and nxt["kind"] != kind and nxt["changed"] > 0)
        out["5 the first edit into a hidden label without voxels, by a %s" % kind] = found
    for kind in EDITORS:
        out["6 a dry run of kind %s between real edits" % kind] = any(
            t["would"] > 0 and any(e["changed"] for e in _edits(trace[:t["k"]], dry=False)) and any(e["changed"] for e in _edits(trace[t["k"]:], dry=False))
            for t in _edits(trace, kind=kind, dry=True))
    found = False
    for t in _edits(trace, dry=False):
        for snap, kind in (("nearest", "fill"), ("geodesic", "flood")):
            if t["kind"] == kind and t["changed"] > 0:
                taken = trace[t["reads"][snap]]
                seeds = np.flatnonzero(np.asarray(getattr(taken["request"], "select" if snap == "nearest" else "seed")))
                found = found or any(u["op"] == "undo" and int(u["left"][seeds].sum() + u["arrived"][seeds].sum()) > 0 for u in _swaps(trace[taken["k"]:t["k"]]))
    out["7 a fill or flood by a snapshot older than an undo that changed the seeds"] = found
    return out


# which hand-written script must contain which hazard: every hazard in "a working day" but the flood's half of 5
def required(name, hazard):
    if name == "a working day":
        return not hazard.endswith("by a flood")
    if name == "give up and go on":
        return hazard.endswith("by a flood")
    return False
