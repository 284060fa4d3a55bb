"""The editing sessions of tests/session_scenes.py on the host model alone: no GPU.

Every script, the committed generated ones included, is run on the model, and the conditions tests/test_gpu_session.py relies on are
asserted, so that a script cannot pass on the device for a trivial reason: the edits change texels, every hazard of the module's list
occurs (each stated as a predicate over the script's trace), and the journal's counters reach what the script's description claims.
Along every script the model's labels and step counts are compared with a second, independent model that keeps whole copies of the
labels per step (as tests/test_label_history_host.py does for relabels) and restates the budget's rule; the same model with a wrong
rule must disagree on every hand-written script, which shows that the scripts reach those rules.
"""
import numpy as np
import pytest

from tests import session_scenes as SN
from volym_amd import scene

HAND_WRITTEN = ["a working day", "give up and go on", "ragged"]
_runs = {}


def _run(oracle, name, bricked):
    """(script, steps, the model after the whole script), run once per script and layout"""
    if (name, bricked) not in _runs:
        script = SN.scripts()[name] if name in SN.scripts() else SN.generated(name)
        _runs[name, bricked] = (script, script.steps(oracle, bricked), script.model(oracle, bricked))
    return _runs[name, bricked]


class Whole:
    """undo and redo by whole copies, with the budget's rule restated: `past` holds (the labels before, chunks) of each undoable
    step, oldest first; `future` (the labels after, chunks) of each undone one, the next to be redone last.  keep_redo and
    evict_newest are the wrong rules of test_a_wrong_rule_disagrees_on_every_hand_written_script."""

    def __init__(self, dims, bricked, keep_redo=False, evict_newest=False):
        self.dims, self.bricked, self.keep_redo, self.evict_newest = dims, bricked, keep_redo, evict_newest
        self.budget, self.past, self.future, self.dropped, self.lost = 0, [], [], 0, 0

    def set_budget(self, b):
        if b == 0:
            self.budget, self.past, self.future, self.dropped, self.lost = 0, [], [], 0, 0
            return
        if self.budget == 0:
            self.dropped = self.lost = 0
        self.budget = b
        self.fit()

    def fit(self):
        while 20 * sum(c for _, c in self.past + self.future) > self.budget:
            if self.past:
                self.past.pop(-1 if self.evict_newest else 0)
            else:
                self.future.pop(0)
            self.dropped += 1

    def clear(self):
        self.past, self.future = [], []

    def record(self, old, new, box):
        if self.budget == 0 or np.array_equal(old, new):
            return
        if not self.keep_redo:
            self.future = []
        chunks = scene.label_chunks_changed(self.dims, old, new, self.bricked)
        if chunks > min(scene.relabel_slab_items(self.dims, box, self.bricked), self.budget // 20):
            self.past, self.future = [], []
            self.lost += 1
            return
        self.past.append((old.copy(), chunks))
        self.fit()

    def undo(self, labels):
        if self.budget == 0 or not self.past:
            return None
        before, chunks = self.past.pop()
        self.future.append((labels.copy(), chunks))
        return before

    def redo(self, labels):
        if self.budget == 0 or not self.future:
            return None
        after, chunks = self.future.pop()
        self.past.append((labels.copy(), chunks))
        return after

    def counts(self):
        return len(self.past), len(self.future), self.dropped, self.lost


def shadow(host, bricked, steps, trace, **wrong):
    """Whole driven along a trace of the model: (the first disagreement or None, the Whole at the end)"""
    whole = Whole(host.dims, bricked, **wrong)
    labels = host.labels
    for step, t in zip(steps, trace):
        if t["op"] == "edit" and not t["dry"]:
            whole.record(labels, t["labels"], t["journal_box"])
        elif t["op"] in ("undo", "redo"):
            got = (whole.undo if t["op"] == "undo" else whole.redo)(labels)
            if (got is None) != t["refused"]:
                return "step %d (%s): the model %s, the whole copies %s" % (t["k"], t["op"], "refuses" if t["refused"] else "swaps", "refuse" if got is None else "swap"), whole
            if got is not None and not np.array_equal(got, t["labels"]):
                return "step %d (%s): %d labels differ" % (t["k"], t["op"], int((got != t["labels"]).sum())), whole
        elif t["op"] == "budget":
            whole.set_budget(step.args[0])
        elif t["op"] == "hand":
            whole.clear()
        i = t["info"]
        if whole.counts() != (i["undo_steps"], i["redo_steps"], i["dropped_steps"], i["lost"]):
            return "step %d (%s): undo, redo, dropped, lost are %r, the whole copies' %r" % (t["k"], step.describe(), (i["undo_steps"], i["redo_steps"], i["dropped_steps"], i["lost"]),
                                                                                         whole.counts()), whole
        labels = t["labels"]
    return None, whole


def _evictions(trace):
    """steps evicted over the whole script (the counter starts again when the history is switched off)"""
    d = [0] + [t["info"]["dropped_steps"] for t in trace]
    return sum(max(0, b - a) for a, b in zip(d[:-1], d[1:]))


def _given_up(trace):
    d = [0] + [t["info"]["lost"] for t in trace]
    return sum(max(0, b - a) for a, b in zip(d[:-1], d[1:]))


# ---- 1. the hand-written scripts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bricked", [False, True])
@pytest.mark.parametrize("name", HAND_WRITTEN)
def test_the_conditions_the_device_test_relies_on(oracle, name, bricked):
    script, steps, s = _run(oracle, name, bricked)
    trace = s.trace
    edits = [t for t in trace if t["op"] == "edit"]
    # every real edit that is no deliberate no-op changes at least 50 texels; a dry run counts them and leaves everything as it was
    for t in edits:
        before = trace[t["k"] - 1]
        if t["dry"]:
            assert t["would"] >= 50 and t["labels"] is before["labels"] and t["info"] == before["info"] and not t["recorded"], (name, t["k"], t["name"])
        elif not t["noop"]:
            assert t["changed"] >= 50, (name, t["k"], t["name"], t["changed"])
    # the hazards
    found = SN.hazards(trace)
    for hazard, there in found.items():
        assert there or not SN.required(name, hazard), (name, "the script does not contain hazard", hazard)
    # the counters reach what the description claims, and the budgets were derived from the records this run journals
    assert _evictions(trace) >= script.claims["evictions"] and _given_up(trace) == script.claims["lost"], (name, _evictions(trace), _given_up(trace))
    assert max(t["info"]["undo_steps"] for t in trace) >= 2
    records = {t["tag"]: t["records"] for t in trace if t["tag"] is not None}
    derived = [st for st in steps if st.op == "budget" and st.derive is not None]
    assert derived and all(st.args[0] == st.derive(records) for st in derived), (name, "the budgets are not those of the records this run journals")
    evicted = [kind for t in trace for kind in t.get("evicted", [])]
    assert len(evicted) == _evictions(trace) and (name != "a working day" or len(set(evicted)) >= 3), (name, "steps of different kinds are evicted", evicted)


def test_what_the_scripts_hold(oracle):
    kinds = lambda steps, op: [st.args[0] for st in steps if st.op == op]                              # noqa: E731
    for bricked in (False, True):
        _, steps, s = _run(oracle, "a working day", bricked)
        real = [t["kind"] for t in s.trace if t["op"] == "edit" and not t["dry"] and t["changed"] > 0]
        assert len(steps) >= 40 and all(real.count(k) >= 2 for k in SN.EDITORS), real
        assert {k for t in s.trace for k in t["reads"]} == set(SN.PASSES)
        looks = [t for t in s.trace if t["op"] == "look"]
        assert 7 <= len(looks) <= 9 and any(all(c is not None for c in t["cut"]) for t in looks) and looks[-1]["cut"] == SN.LIFTED and s.host.ever_cut
        assert {"table", "frames"} <= {st.op for st in steps}
        _, steps, s = _run(oracle, "give up and go on", bricked)
        budgets = kinds(steps, "budget")
        off = budgets.index(0)
        assert 0 < off < len(budgets) - 1 and budgets[off + 1] > 0 and "hand" in {st.op for st in steps}
        lost_at = next(t["k"] for t in s.trace if t["info"]["lost"])
        assert s.trace[lost_at]["kind"] == "fill" and s.trace[lost_at]["changed"] > 5000
        later = [t for t in s.trace[lost_at:] if t["op"] == "undo" and not t["refused"]]
        assert len({t["kind"] for t in later}) >= 4, "the edits of other kinds after the give-up are journalled again and undone"
        assert sum(t["refused"] for t in s.trace) >= 5
        _, steps, s = _run(oracle, "ragged", bricked)
        assert sorted(kinds(steps, "edit")) == sorted(SN.EDITORS) and len(steps) <= 20
        ops = [st.op for st in steps]
        assert (ops.count("undo"), ops.count("redo"), ops.count("look")) == (2, 1, 3) and ops.count("cut") == 3      # (two cuts, and all lifted)
        assert all(st.oracle for st in steps if st.op == "look")
    assert all(st.op != "look" or not st.oracle for st in _run(oracle, "a working day", False)[1][:-1]) and _run(oracle, "a working day", False)[1][-1].oracle


@pytest.mark.parametrize("bricked", [False, True])
@pytest.mark.parametrize("name", HAND_WRITTEN + SN.SEEDS[:3])
def test_the_model_restores_what_whole_copies_restore(oracle, name, bricked):
    script, steps, s = _run(oracle, name, bricked)
    differs, whole = shadow(script.host(), bricked, steps, s.trace)
    assert differs is None, (name, differs)
    # undo everything that can be undone: the labels are the whole copy of the oldest kept step
    labels, n = s.host.labels, 0
    oldest = whole.past[0][0] if whole.past else None
    while s.twin.info()["undo_steps"]:
        labels, _ = s.twin.undo(labels)
        n += 1
    assert n == len(whole.past) and (oldest is None or np.array_equal(labels, oldest))
    while n:                                            # (and back: the model is shared with the other tests)
        labels, _ = s.twin.redo(labels)
        n -= 1
    assert np.array_equal(labels, s.host.labels)


@pytest.mark.parametrize("wrong", ["keep_redo", "evict_newest"])
@pytest.mark.parametrize("name", HAND_WRITTEN)
def test_a_wrong_rule_disagrees_on_every_hand_written_script(oracle, name, wrong):
    """a recorded edit that keeps the redo steps; an eviction that takes the newest step"""
    for bricked in (False, True):
        script, steps, s = _run(oracle, name, bricked)
        differs, _ = shadow(script.host(), bricked, steps, s.trace, **{wrong: True})
        assert differs is not None, (name, bricked, "the script does not reach the rule", wrong)


# ---- 2. the generated scripts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bricked", [False, True])
@pytest.mark.parametrize("seed", SN.SEEDS)
def test_a_generated_script_does_something(oracle, seed, bricked):
    """conditions, not measurements: a committed seed that misses them is replaced by another"""
    script, steps, s = _run(oracle, seed, bricked)
    assert len(steps) >= 30
    again = SN.generate(oracle, seed)
    assert [st.describe() for st in again] == [st.describe() for st in script.steps(oracle, bricked)], "the generator is deterministic"
    edits = [t for t in s.trace if t["op"] == "edit"]
    moved = [t for t in edits if (t["would"] if t["dry"] else t["changed"]) > 0]
    assert len(moved) >= 0.6 * len(edits), (seed, len(moved), len(edits))
    assert {t["kind"] for t in edits if t["changed"] > 0} == set(SN.EDITORS), seed
    assert any(t["op"] == "undo" and not t["refused"] for t in s.trace) and any(t["op"] == "redo" and not t["refused"] for t in s.trace), seed
