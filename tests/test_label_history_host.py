"""The host twin of the label history (scene.LabelHistory, scene.label_chunks_changed, scene.relabel_slab_items): no GPU.

The twin is pinned against a plain model that keeps a whole copy of the labels per step, over random sequences of record, undo and
redo on scene A of tests/relabel_scenes.py, and the chunk count against a brute-force loop over texels.  The conditions
tests/test_gpu_label_history.py relies on (tests/label_history_scenes.py) are asserted here on the twin.
"""
import numpy as np
import pytest

from tests import label_history_scenes as LS
from tests import measure_scenes as MS
from tests import relabel_scenes as RS
from volym_amd import scene


class Plain:
    """undo and redo by whole copies: `past` holds the labels before each undoable edit, `future` those after each undone one"""

    def __init__(self):
        self.past, self.future = [], []

    def record(self, old, new):
        if np.array_equal(old, new):
            return
        self.past.append(old.copy())
        self.future = []

    def undo(self, labels):
        self.future.append(labels.copy())
        return self.past.pop()

    def redo(self, labels):
        self.past.append(labels.copy())
        return self.future.pop()


def _random_edit(rng, host, labels):
    """a random request of the twin's rule over the labels as they stand: a table on a random box, sometimes an identity"""
    nx, ny, nz = host.dims
    lo = [int(rng.integers(0, n)) for n in host.dims]
    hi = [int(rng.integers(l + 1, n + 1)) for l, n in zip(lo, host.dims)]
    to = {int(l): int(rng.integers(0, 12)) for l in rng.integers(0, 12, 3)} if rng.random() > 0.15 else {}
    r = scene.Relabel((tuple(lo), tuple(hi)), window=(int(rng.integers(0, 100)), 255), to=to)
    new, _ = scene.relabel_volume(host.vol, host.dims, r, labels)
    return r, new.ravel()


@pytest.mark.parametrize("bricked", [False, True])
def test_the_twin_restores_what_a_model_with_whole_copies_restores(bricked):
    rng = np.random.default_rng(11 + int(bricked))
    host = RS.scene_a()
    labels = host.labels.copy()
    twin, plain = scene.LabelHistory(LS.BIG, host.dims, bricked), Plain()
    done = {"record": 0, "undo": 0, "redo": 0}
    for _ in range(120):
        op = rng.choice(["record", "undo", "undo", "redo"])
        if op == "record":
            r, new = _random_edit(rng, host, labels)
            twin.record(labels, new, box=r.box)
            plain.record(labels, new)
            labels = new
        elif op == "undo" and plain.past:
            want = plain.undo(labels)
            got, result = twin.undo(labels)
            assert int(result["changed"]) == int((want != labels).sum()) > 0
            assert np.array_equal(result["left"], np.bincount(labels[want != labels], minlength=256))
            assert np.array_equal(result["arrived"], np.bincount(want[want != labels], minlength=256))
            assert np.array_equal(got, want)
            labels = got
        elif op == "redo" and plain.future:
            want = plain.redo(labels)
            got, result = twin.redo(labels)
            assert int(result["changed"]) == int((want != labels).sum()) > 0
            assert np.array_equal(got, want)
            labels = got
        else:
            with pytest.raises(ValueError):
                (twin.undo if op == "undo" else twin.redo)(labels)
            continue
        done[op] += 1
        info = twin.info()
        assert (info["undo_steps"], info["redo_steps"]) == (len(plain.past), len(plain.future))
        assert info["used_bytes"] <= info["budget_bytes"] and info["dropped_steps"] == info["lost"] == 0
    assert min(done.values()) >= 10, done


@pytest.mark.parametrize("bricked", [False, True])
@pytest.mark.parametrize("dims", [(37, 22, 19), (8, 4, 3), (16, 5, 2)])
def test_chunks_changed_against_a_loop_over_texels(dims, bricked):
    rng = np.random.default_rng(5)
    nx, ny, nz = dims
    n = nx * ny * nz
    for density in (0.0, 0.002, 0.05, 1.0):
        old = rng.integers(0, 4, n).astype(np.uint8)
        new = np.where(rng.random(n) < density, old + 1, old).astype(np.uint8)
        seen = set()
        for z in range(nz):
            for y in range(ny):
                for x in range(nx):
                    i = x + nx * (y + ny * z)
                    if old[i] != new[i]:
                        seen.add((x // 4, y // 4, z) if bricked else i // 16)
        assert scene.label_chunks_changed(dims, old, new, bricked) == len(seen), (dims, bricked, density)


def test_slab_items_bound_the_chunks_an_edit_inside_the_box_can_change():
    """the staging area's worst case: an edit that changes every texel of the box journals no more chunks than the slab has items"""
    dims = MS.DIMS
    nx, ny, nz = dims
    old = np.zeros(nx * ny * nz, np.uint8)
    for name, box in list(MS.BOXES.items()) + [("slices", ((0, 0, 3), (nx, ny, 11))), ("one row", ((0, 7, 5), (nx, 8, 6)))]:
        (x0, y0, z0), (x1, y1, z1) = box
        new = old.reshape(nz, ny, nx).copy()
        new[z0:z1, y0:y1, x0:x1] = 1
        for bricked in (False, True):
            assert scene.label_chunks_changed(dims, old, new, bricked) <= scene.relabel_slab_items(dims, box, bricked), (name, bricked)
    assert scene.relabel_slab_items(dims, None, False) == (nx * ny * nz + 15) // 16 + 1
    assert scene.relabel_slab_items(dims, None, True) == 4 * 10 * 6 * 5


def test_the_conditions_the_device_test_relies_on():
    for which in LS.CHOSEN:
        host, cases = LS.chosen(which)
        labels, results = LS.twin_steps(which)
        assert len(cases) == (4 if which == "a" else 2)
        assert all(int(r["changed"]) > 50 for r in results), (which, [int(r["changed"]) for r in results])
        assert all(not c.relabel.flags & 16 and not c.trivial for c in cases)
    # chunks of the linear layout that hold changed texels of two rows: the walk of the swap kernel wraps there
    labels, _ = LS.twin_steps("a")
    assert max(RS.wrapping_chunks(MS.DIMS, a, b) for a, b in zip(labels[:-1], labels[1:])) > 100
    host, cases = LS.chosen("ragged")
    labels, _ = LS.twin_steps("ragged")
    assert cases[0].wraps and RS.wrapping_chunks(host.dims, labels[0], labels[1]) > 1000
    # ... and hold texels outside the request's box: the narrow box of the first edit
    (x0, _, _), (x1, _, _) = LS.chosen("a")[1][0].relabel.box
    assert x0 % 16 != 0 and x1 - x0 < 16
    for bricked in (False, True):
        dims = MS.DIMS
        rec = LS.records("a", bricked)
        cases = LS.chosen("a")[1]
        items = [scene.relabel_slab_items(dims, c.relabel.box, bricked) for c in cases]
        small, over = LS.small_budget(bricked), LS.overflow_budget(bricked)
        # the small budget: every single step fits (budget and staging area), all four do not
        assert all(r <= min(i, small // 20) for r, i in zip(rec, items)) and 20 * sum(rec) > small >= 20 * sum(rec[1:])
        twin = scene.LabelHistory(small, dims, bricked)
        labels, _ = LS.twin_steps("a")
        for c, a, b in zip(cases, labels[:-1], labels[1:]):
            assert twin.record(a, b, box=c.relabel.box)
        assert twin.info() == {"budget_bytes": small, "used_bytes": 20 * sum(rec[1:]), "undo_steps": 3, "redo_steps": 0, "next_undo_records": rec[3],
                               "next_redo_records": 0, "dropped_steps": 1, "lost": 0}
        # the overflow budget: the first step fits, the second has more records than the budget holds
        assert rec[0] <= over // 20 < rec[1]
        twin = scene.LabelHistory(over, dims, bricked)
        assert twin.record(labels[0], labels[1], box=cases[0].relabel.box) and not twin.record(labels[1], labels[2], box=cases[1].relabel.box)
        assert twin.info() == {"budget_bytes": over, "used_bytes": 0, "undo_steps": 0, "redo_steps": 0, "next_undo_records": 0, "next_redo_records": 0,
                               "dropped_steps": 0, "lost": 1}
        # the big budget holds every step of every scene
        assert all(20 * sum(LS.records(w, bricked)) <= LS.BIG for w in LS.CHOSEN)


def test_budget_changes_clear_and_switching_off():
    dims = MS.DIMS
    labels, _ = LS.twin_steps("a")
    rec = LS.records("a", False)
    twin = scene.LabelHistory(LS.BIG, dims, False)
    for a, b in zip(labels[:-1], labels[1:]):
        twin.record(a, b)
    assert not twin.record(labels[4], labels[4]) and twin.info()["undo_steps"] == 4          # an edit that changes nothing records nothing
    now, _ = twin.undo(labels[4])
    now, _ = twin.undo(now)
    assert np.array_equal(now, labels[2]) and (twin.info()["undo_steps"], twin.info()["redo_steps"]) == (2, 2)
    # a smaller budget: the oldest undoable steps go first, then the redo steps that would be redone last
    twin.set_budget(20 * (rec[1] + rec[2] + rec[3]))
    assert (twin.info()["undo_steps"], twin.info()["redo_steps"], twin.info()["dropped_steps"]) == (1, 2, 1)
    twin.set_budget(20 * rec[2])
    assert (twin.info()["undo_steps"], twin.info()["redo_steps"], twin.info()["dropped_steps"]) == (0, 1, 3)
    now, result = twin.redo(now)
    assert np.array_equal(now, labels[3]) and int(result["changed"]) == int((labels[2] != labels[3]).sum())
    # a recorded edit drops the redo steps; clear keeps budget and counters; 0 switches everything off
    twin.set_budget(LS.BIG)
    now, _ = twin.undo(now)
    assert twin.record(now, labels[0])
    assert (twin.info()["undo_steps"], twin.info()["redo_steps"]) == (1, 0)
    twin.clear()
    assert twin.info() == {"budget_bytes": LS.BIG, "used_bytes": 0, "undo_steps": 0, "redo_steps": 0, "next_undo_records": 0, "next_redo_records": 0,
                           "dropped_steps": 3, "lost": 0}
    twin.set_budget(0)
    assert not twin.record(labels[0], labels[1]) and set(twin.info().values()) == {0}
