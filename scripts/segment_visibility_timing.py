"""Time segment-visibility edits two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3):
  device -- volym_set_segment_visibility: the texels inside the boxes of the labels that flipped rewritten on the device (only
            the 16-byte chunks that hold such a label), the macro cells those boxes touch rebuilt, lists reset;
  host   -- the only way without it: NumPy zeroing of density and importances (scene.hide_segments), then volym_set_volume and
            volym_set_importances of those bytes.
Edits: toggle the trunk (label 3: a small box), the canopy (label 2: the largest segment, a wide box), the pot (label 4), all
three at once, and the canopy while the near z half of the volume is cropped away.  Each edit alternates between hidden and
shown, so every repetition rewrites the same texels.  A figure is a host clock around the call(s), ending in volym_sync; one
warm-up edit, then --reps (device) or --host-reps (host) repetitions: median, minimum and maximum (--host-reps 0 leaves the host
path out, for a run under `rocprofv3 --kernel-trace --stats`).  The first hide of a context (which copies the uncropped
density) is timed on its own.

    python scripts/segment_visibility_timing.py [--size 1024] [--reps 9] [--host-reps 3] [--out profiles/segment_visibility.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from volym_amd import demo, scene, synth  # noqa: E402


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run(n, reps, host_reps):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    del raw, labels
    table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}])
    imp = table[lab]
    full = ((0, 0, 0), dims)
    half = ((0, 0, 0), (n, n, n // 2))
    edits = [
        ("trunk (label 3)", (3,), full),
        ("canopy (label 2)", (2,), full),
        ("pot (label 4)", (4,), full),
        ("trunk, canopy and pot", (2, 3, 4), full),
        ("canopy, near z half cropped", (2,), half),
    ]
    show = scene.visibility_mask(())
    rows = []
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.sync()
        counts = ctx.label_counts()
        t0 = time.perf_counter()
        ctx.set_segment_visibility(scene.visibility_mask((3,)))
        ctx.sync()
        first = (time.perf_counter() - t0) * 1e3
        ctx.set_segment_visibility(show)
        for name, hidden, box in edits:
            hide = scene.visibility_mask(hidden)
            ctx.set_crop_box(*box)
            ctx.set_segment_visibility(hide)
            ctx.set_segment_visibility(show)         # warm-up, and the state every repetition starts from
            ctx.sync()
            dev = []
            for r in range(reps):
                t0 = time.perf_counter()
                ctx.set_segment_visibility(hide if r % 2 == 0 else show)
                ctx.sync()
                dev.append((time.perf_counter() - t0) * 1e3)
            ctx.set_segment_visibility(show)
            ctx.set_crop_box(*full)
            rows.append([name, int(sum(int(counts[l]) for l in hidden)), _stats(dev), None])
        for row, (name, hidden, box) in zip(rows, edits):
            if host_reps <= 0:
                break
            hide = scene.visibility_mask(hidden)
            host = []
            for r in range(host_reps + 1):
                mask = hide if r % 2 == 0 else show
                t0 = time.perf_counter()
                ctx.set_volume(scene.crop_volume(scene.hide_segments(vol, lab, mask), dims, *box), dims, 0)
                ctx.set_importances(scene.crop_volume(scene.hide_segments(imp, lab, mask), dims, *box), dims)
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
            row[3] = _stats(host[1:])
    return first, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    first, rows = run(a.size, a.reps, a.host_reps)
    lines = ["%d^3, labels on the device; milliseconds per edit, median (min .. max)" % a.size,
             "first hide of the context (the trunk; copies the uncropped density): %.3f ms" % first]
    for name, voxels, dev, host in rows:
        head = "%-28s %10d voxels   volym_set_segment_visibility %8.3f (%.3f .. %.3f)" % (name, voxels, dev[0], dev[1], dev[2])
        if host is not None:
            head += "   host zeroing + re-upload %8.1f (%.1f .. %.1f)   %.0fx" % (host[0], host[1], host[2], host[0] / dev[0])
        lines.append(head)
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
