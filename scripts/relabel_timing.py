"""Time label edits two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3):
  device -- volym_edit_labels: the relabel kernel over the request's box, the label statistics rescanned, importances (and, under
            a mask, density and macro cells) rewritten inside the hull of the changed texels, lists reset;
  host   -- the path the call replaces: read back the ids or the distance map the edit goes by (none for a table edit),
            np.where on the labels, then volym_set_labels, volym_set_segment_importances and volym_set_segment_visibility.
Edits: the trunk renamed by the table alone (3 <-> 9), the trunk's second piece split off by the ids of one components pass
(3 <-> 9 for ids 1..1), the canopy grown by 3 texels into the air by one distance map (0 <-> 2 for D in 1..9).  Each edit
alternates with its inverse, which goes by the same snapshot, so every repetition relabels the same texels.  The pot is hidden
throughout, so the host path has a mask to send again.  A figure is a host clock around the call(s), ending in volym_sync; one
warm-up edit, then --reps (device) or --host-reps (host) repetitions: median, minimum and maximum (--host-reps 0 leaves the host
path out, for a run under `rocprofv3 --kernel-trace --stats`).  The components and the distance pass are timed once each, on
their own: they are the analysis the edit acts on, not part of it.

    python scripts/relabel_timing.py [--size 1024] [--reps 9] [--host-reps 2] [--out profiles/relabel.txt]
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


def _say(text):
    print(text, flush=True)


def run(n, reps, host_reps):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    del raw, labels
    table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}, {"label_value": 9, "importance": 128}])
    hidden = scene.visibility_mask((4,))
    R = scene.Relabel
    rows, passes = [], {}
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.set_segment_visibility(hidden)
        ctx.sync()
        _say("scene of %d^3 on the device" % n)
        t0 = time.perf_counter()
        ctx.components_pass(scene.Components(dims=dims, min_byte=200, select=scene.surface_select([3])))
        ctx.sync()
        passes["components pass (trunk, min_byte 200)"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ctx.distance_pass(scene.Distance(dims=dims, select=scene.surface_select([2])))
        ctx.sync()
        passes["distance pass (canopy)"] = (time.perf_counter() - t0) * 1e3
        _say("passes done")
        edits = [
            ("table: trunk 3 <-> 9", R(dims=dims, to={3: 9}), R(dims=dims, to={9: 3}), None),
            ("ids 1..1: the trunk's second piece 3 <-> 9", R(dims=dims, flags=_lib.RELABEL_IDS, to={3: 9}, ids=(1, 1)),
             R(dims=dims, flags=_lib.RELABEL_IDS, to={9: 3}, ids=(1, 1)), "ids"),
            ("distance 1..9: the canopy grown by 3, 0 <-> 2", R(dims=dims, flags=_lib.RELABEL_DISTANCE, to={0: 2}, d2=(1, 9)),
             R(dims=dims, flags=_lib.RELABEL_DISTANCE, to={2: 0}, d2=(1, 9)), "map"),
        ]
        for name, there, back, snapshot in edits:
            changed = int(ctx.edit_labels(there)["changed"])
            ctx.edit_labels(back)                    # warm-up, and the state every repetition starts from
            ctx.sync()
            dev = []
            for r in range(reps):
                t0 = time.perf_counter()
                ctx.edit_labels(there if r % 2 == 0 else back)
                ctx.sync()
                dev.append((time.perf_counter() - t0) * 1e3)
            if reps % 2:
                ctx.edit_labels(back)
            rows.append([name, changed, _stats(dev), None, snapshot, there, back])
            _say("%s: %d texels, device %.3f ms" % (name, changed, _stats(dev)[0]))
        assert np.array_equal(ctx.read_labels().ravel(), lab), "the edits and their inverses must leave the labels as they were"
        for row in rows:
            if host_reps <= 0:
                break
            name, changed, _, _, snapshot, there, back = row
            now = lab
            host = []
            for r in range(host_reps + 1):
                req = there if r % 2 == 0 else back
                to = np.asarray(req.to, np.int64).astype(np.uint8)
                t0 = time.perf_counter()
                if snapshot == "ids":
                    ids = ctx.read_component_ids().ravel()
                    new = np.where((ids >= req.ids[0]) & (ids <= req.ids[1]), to[now], now)
                    del ids
                elif snapshot == "map":
                    dmap = ctx.read_distance_map().ravel()
                    new = np.where((dmap >= req.d2[0]) & (dmap <= req.d2[1]), to[now], now)
                    del dmap
                else:
                    new = to[now]
                ctx.set_labels(new, dims)
                ctx.set_segment_importances(table)
                ctx.set_segment_visibility(hidden)
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
                now = new
            row[3] = _stats(host[1:])
            if host_reps % 2 == 0:                   # (an odd number of edits so far: back to the labels of the start)
                ctx.set_labels(lab, dims)
                ctx.set_segment_importances(table)
                ctx.set_segment_visibility(hidden)
            _say("%s: host %.1f ms" % (name, row[3][0]))
    return passes, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    passes, rows = run(a.size, a.reps, a.host_reps)
    lines = ["%d^3, labels on the device, the pot hidden; milliseconds per edit, median (min .. max)" % a.size]
    lines += ["%s, once, with its first allocation: %.1f ms" % (k, v) for k, v in passes.items()]
    for name, changed, dev, host, _, _, _ in rows:
        head = "%-48s %10d texels   volym_edit_labels %9.3f (%.3f .. %.3f)" % (name, changed, dev[0], dev[1], dev[2])
        if host is not None:
            head += "   host read-back + np.where + re-upload %9.1f (%.1f .. %.1f)   %.0fx" % (host[0], host[1], host[2], host[0] / dev[0])
        lines.append(head)
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
