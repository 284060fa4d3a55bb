"""Time the label history on the scene scripts/relabel_timing.py uses (seeded synthetic bonsai, default 1024^3, labels on the
device, the pot hidden), for the same three edits: the trunk renamed by the table alone (3 -> 9), the trunk's second piece split
off by the ids of one components pass (3 -> 9 for ids 1..1), the canopy grown by 3 texels by one distance map (0 -> 2 for D in 1..9).

  off   -- volym_edit_labels with the history off, each edit alternating with its inverse as in relabel_timing.py (run that
           script under this commit and its parent for the comparison between the two); the figure is that of the edit alone, not
           of its inverse, which is the direction the next column takes;
  on    -- the same edit with the history on (--budget-mb): the journalling kernel, the step copied out of the staging area;
  undo, redo -- volym_undo_labels and volym_redo_labels of that step: the swap kernel and the edit's follow-up;
  host  -- the path they replace: volym_read_labels of the whole volume before the edit (save), then volym_set_labels,
           volym_set_segment_importances and volym_set_segment_visibility to go back (restore).

A repetition with the history on is edit, undo, redo, undo, which ends where it began.  A figure is a host clock around the call,
ending in volym_sync; one warm-up repetition, then --reps: median, minimum and maximum.  --host-reps 0 leaves the host path out,
for a run under `rocprofv3 --kernel-trace --stats`, which splits a call into its kernels.

    python scripts/label_history_timing.py [--size 1024] [--reps 9] [--host-reps 2] [--budget-mb 256] [--out profiles/label_history.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from volym_amd import _lib, demo, scene, synth  # noqa: E402


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _fmt(s):
    return "%9.3f (%.3f .. %.3f)" % s


def _say(text):
    print(text, flush=True)


def _timed(ctx, call):
    t0 = time.perf_counter()
    out = call()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def run(n, reps, host_reps, budget_mb):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    del raw, labels
    table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}, {"label_value": 9, "importance": 128}])
    hidden = scene.visibility_mask((4,))
    R = scene.Relabel
    rows, host = [], None
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.set_segment_visibility(hidden)
        ctx.components_pass(scene.Components(dims=dims, min_byte=200, select=scene.surface_select([3])))
        ctx.distance_pass(scene.Distance(dims=dims, select=scene.surface_select([2])))
        ctx.sync()
        _say("scene of %d^3 on the device, passes done" % n)
        edits = [
            ("table: trunk 3 -> 9", R(dims=dims, to={3: 9}), R(dims=dims, to={9: 3})),
            ("ids 1..1: the trunk's second piece 3 -> 9", R(dims=dims, flags=_lib.RELABEL_IDS, to={3: 9}, ids=(1, 1)),
             R(dims=dims, flags=_lib.RELABEL_IDS, to={9: 3}, ids=(1, 1))),
            ("distance 1..9: the canopy grown by 3, 0 -> 2", R(dims=dims, flags=_lib.RELABEL_DISTANCE, to={0: 2}, d2=(1, 9)),
             R(dims=dims, flags=_lib.RELABEL_DISTANCE, to={2: 0}, d2=(1, 9))),
        ]
        for name, there, back in edits:
            ctx.label_history(0)
            changed = int(ctx.edit_labels(there)["changed"])
            ctx.edit_labels(back)                    # warm-up, and the state every repetition starts from
            ctx.sync()
            off = []
            for r in range(reps + reps % 2):          # (an even number: back to the labels of the start)
                off.append(_timed(ctx, lambda: ctx.edit_labels(there if r % 2 == 0 else back))[0])
            ctx.label_history(budget_mb << 20)
            on, undo, redo, records = [], [], [], 0
            for r in range(reps + 1):
                ms = [_timed(ctx, lambda: ctx.edit_labels(there))[0]]
                info = ctx.label_history_info()
                assert info["lost"] == 0 and info["undo_steps"] >= 1, info
                records = info["next_undo_records"]
                ms.append(_timed(ctx, ctx.undo_labels)[0])
                ms.append(_timed(ctx, ctx.redo_labels)[0])
                ms.append(_timed(ctx, ctx.undo_labels)[0])
                if r:                                # (the first repetition grows the staging area: warm-up)
                    on.append(ms[0]); undo += [ms[1], ms[3]]; redo.append(ms[2])
            off = off[0::2]                           # the direction the journalled edit takes: an edit and its inverse differ in cost
            rows.append((name, changed, records, _stats(off), _stats(on), _stats(undo), _stats(redo)))
            _say("%s: %d texels, %d records, off %.3f on %.3f undo %.3f redo %.3f ms" % (name, changed, records, rows[-1][3][0], rows[-1][4][0],
                                                                                      rows[-1][5][0], rows[-1][6][0]))
        ctx.label_history(0)
        if host_reps > 0:
            save, restore = [], []
            for r in range(host_reps + 1):
                ms, kept = _timed(ctx, ctx.read_labels)
                save.append(ms)

                def back_again():
                    ctx.set_labels(kept.ravel(), dims)
                    ctx.set_segment_importances(table)
                    ctx.set_segment_visibility(hidden)
                restore.append(_timed(ctx, back_again)[0])
            host = (_stats(save[1:]), _stats(restore[1:]))
        assert np.array_equal(ctx.read_labels().ravel(), lab), "every repetition must leave the labels as they were"
    return rows, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--budget-mb", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, host = run(a.size, a.reps, a.host_reps, a.budget_mb)
    lines = ["%d^3, labels on the device, the pot hidden, history budget %d MB; milliseconds per call, median (min .. max)" % (a.size, a.budget_mb)]
    for name, changed, records, off, on, undo, redo in rows:
        lines.append("%s: %d texels, %d records (%.1f MB)" % (name, changed, records, records * 20 / 1e6))
        lines.append("    volym_edit_labels, history off %s   history on %s   extra %.3f" % (_fmt(off), _fmt(on), on[0] - off[0]))
        lines.append("    volym_undo_labels %s   volym_redo_labels %s" % (_fmt(undo), _fmt(redo)))
    if host is not None:
        lines.append("host path: volym_read_labels of the whole volume %s   set_labels + table + mask %s" % (_fmt(host[0]), _fmt(host[1])))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
