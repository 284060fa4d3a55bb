"""The edits and budgets of the label history tests, shared by tests/test_label_history_host.py (which asserts on the host twin the
conditions the device tests rely on) and tests/test_gpu_label_history.py (which compares the device with the twin).

The scenes and requests are those of tests/relabel_scenes.py.  On scene A four edits are applied one after the other: a table on a
narrow box, a density window, pieces by their ids (all but the largest) and a distance band.  On scene B and on the ragged scene two.
"""
import numpy as np

from tests import relabel_scenes as RS

CHOSEN = {
    "a": ("table, x 3..8", "window 100..180, whole", "all but the largest piece of 3 and 4 -> 0", "grow 2 by 2"),
    "b": ("reversed, x 3..8", "window 50..99, all -> 0, x 5..30"),
    "ragged": ("air and shell -> 3, full rows", "core, window 198..203"),
}
SCENES = {"a": (RS.scene_a, RS.cases_a), "b": (RS.scene_b, RS.cases_b), "ragged": (RS.scene_ragged, RS.cases_ragged)}
BIG = 1 << 20           # a budget that holds every step of these scenes (97 * 80 * 71 / 16 chunks * 20 bytes is 689 KB)


def chosen(which):
    """(a new host, the chosen cases of scene `which` in order)"""
    make, cases = SCENES[which]
    by_name = {c.name: c for c in cases()}
    return make(), [by_name[n] for n in CHOSEN[which]]


def twin_steps(which):
    """The twin's run of the chosen edits, applied cumulatively with no cut: [L0, ..., Ln] (flat labels) and the results."""
    host, cases = chosen(which)
    labels, results = [host.labels.copy()], []
    for case in cases:
        new, result, _ = RS.expect(host, case)
        host.labels = new
        labels.append(new.copy())
        results.append(result)
    return labels, results


def records(which, bricked):
    """chunks each chosen edit journals in that layout"""
    from volym_amd import scene
    host, _ = chosen(which)
    labels, _ = twin_steps(which)
    return [scene.label_chunks_changed(host.dims, a, b, bricked) for a, b in zip(labels[:-1], labels[1:])]


def small_budget(bricked):
    """holds the last three steps of scene A exactly: recording the fourth evicts the first"""
    return 20 * sum(records("a", bricked)[1:])


def overflow_budget(bricked):
    """one record short of scene A's second step, the largest: the first step fits, the second does not"""
    return 20 * (records("a", bricked)[1] - 1)


def swapped(result):
    """an edit's result as its undo reports it: left and arrived exchanged"""
    out = np.frombuffer(result.tobytes(), result.dtype).copy()          # (a copy: the edit's result stays as it is)
    out["left"][0], out["arrived"][0] = np.array(result["arrived"]), np.array(result["left"])
    return out[0]
