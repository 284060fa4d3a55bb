"""Time crop-box edits two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3):
  device -- volym_set_crop_box: the slabs between the old faces and the new ones rewritten on the device, the macro cells they
            touch rebuilt, lists reset;
  host   -- the only way without it: NumPy zeroing of density and importances (scene.crop_volume), then volym_set_volume and
            volym_set_importances of those bytes.
Edits: (a) one face moved by 8 texels (the far z face, and the far x face: the thin direction of both layouts), (b) all six
faces moved by 8, (c) the whole volume <-> its near z half.  Each edit alternates between two boxes, so every repetition moves
the same number of texels.  A figure is a host clock around the call(s), ending in volym_sync; one warm-up edit, then --reps
(device) or --host-reps (host) repetitions: median, minimum and maximum (--host-reps 0 leaves the host path out, for a run under
`rocprofv3 --kernel-trace --stats`).  The first crop of a context (which copies the uncropped
density) is timed on its own.

    python scripts/crop_edit_timing.py [--size 1024] [--reps 9] [--host-reps 3] [--out profiles/crop_box.txt]
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
    edits = [
        ("(a) far z face by 8", ((0, 0, 0), (n, n, n - 8)), ((0, 0, 0), (n, n, n - 16))),
        ("(a) far x face by 8", ((0, 0, 0), (n - 8, n, n)), ((0, 0, 0), (n - 16, n, n))),
        ("(b) six faces by 8", ((8, 8, 8), (n - 8, n - 8, n - 8)), ((16, 16, 16), (n - 16, n - 16, n - 16))),
        ("(c) full <-> near z half", ((0, 0, 0), (n, n, n // 2)), full),
    ]
    rows = []
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.set_crop_box((0, 0, 0), (n, n, n - 1))
        ctx.sync()
        first = (time.perf_counter() - t0) * 1e3
        ctx.set_crop_box(*full)
        for name, a, b in edits:
            ctx.set_crop_box(*b)
            ctx.set_crop_box(*a)                     # warm-up, and the state every repetition starts from
            ctx.sync()
            dev = []
            for r in range(reps):
                t0 = time.perf_counter()
                ctx.set_crop_box(*(b if r % 2 == 0 else a))
                ctx.sync()
                dev.append((time.perf_counter() - t0) * 1e3)
            ctx.set_crop_box(*full)
            rows.append([name, _stats(dev), None])
        for row, (name, a, b) in zip(rows, edits):
            if host_reps <= 0:
                break
            host = []
            for r in range(host_reps + 1):
                lo, hi = b if r % 2 == 0 else a
                t0 = time.perf_counter()
                ctx.set_volume(scene.crop_volume(vol, dims, lo, hi), dims, 0)
                ctx.set_importances(scene.crop_volume(imp, dims, lo, hi), dims)
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
            row[2] = _stats(host[1:])
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
             "first crop of the context (copies the uncropped density): %.3f ms" % first]
    for name, dev, host in rows:
        if host is None:
            lines.append("%-26s volym_set_crop_box %8.3f (%.3f .. %.3f)" % (name, dev[0], dev[1], dev[2]))
            continue
        lines.append("%-26s volym_set_crop_box %8.3f (%.3f .. %.3f)   host zeroing + re-upload %8.1f (%.1f .. %.1f)   %.0fx"
                     % (name, dev[0], dev[1], dev[2], host[0], host[1], host[2], host[0] / dev[0]))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
