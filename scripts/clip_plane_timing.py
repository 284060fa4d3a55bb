"""Time clip-plane edits two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3, bricked by
size):
  device -- volym_set_clip_plane: the chunks in which a texel changes side rewritten on the device, the macro cells the changed
            box touches rebuilt, lists reset;
  host   -- the only way without it: NumPy zeroing of density and importances (scene.clip_volume), then volym_set_volume and
            volym_set_importances of those bytes.
Edits: (a) an oblique plane moved by one step, d by 8 * max|n|; (b) a plane and its flip; (c) no plane <-> a diagonal half.  Each
edit alternates between two planes, so every repetition moves the same number of texels.  A figure is a host clock around the
call(s), ending in volym_sync; one warm-up edit, then --reps (device) or --host-reps (host) repetitions: median, minimum and
maximum (--host-reps 0 leaves the host path out, for a run under `rocprofv3 --kernel-trace --stats`).  The first cut of a
context (which copies the uncut density) is timed on its own.

    python scripts/clip_plane_timing.py [--size 1024] [--reps 9] [--host-reps 3] [--out profiles/clip_plane.txt]
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

NONE = ((0, 0, 0), 0)


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
    oblique = (3, -2, 5)
    d0 = 3 * n // 2 - n + 5 * n // 2
    edits = [
        ("(a) oblique plane by one step", (oblique, d0), (oblique, d0 + 8 * 5)),
        ("(b) a plane and its flip", (oblique, d0), (tuple(-v for v in oblique), -d0)),
        ("(c) no plane <-> diagonal half", ((1, 1, 1), 3 * n // 2), NONE),
    ]
    rows = []
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.set_clip_plane((0, 0, 1), n - 2)
        ctx.sync()
        first = (time.perf_counter() - t0) * 1e3
        ctx.set_clip_plane(*NONE)
        for name, a, b in edits:
            ctx.set_clip_plane(*b)
            ctx.set_clip_plane(*a)                   # warm-up, and the state every repetition starts from
            ctx.sync()
            dev = []
            for r in range(reps):
                t0 = time.perf_counter()
                ctx.set_clip_plane(*(b if r % 2 == 0 else a))
                ctx.sync()
                dev.append((time.perf_counter() - t0) * 1e3)
            ctx.set_clip_plane(*NONE)
            rows.append([name, _stats(dev), None])
        for row, (name, a, b) in zip(rows, edits):
            if host_reps <= 0:
                break
            host = []
            for r in range(host_reps + 1):
                plane = b if r % 2 == 0 else a
                t0 = time.perf_counter()
                ctx.set_volume(scene.clip_volume(vol, dims, *plane), dims, 0)
                ctx.set_importances(scene.clip_volume(imp, dims, *plane), dims)
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
             "first cut of the context (copies the uncut density): %.3f ms" % first]
    for name, dev, host in rows:
        if host is None:
            lines.append("%-32s volym_set_clip_plane %8.3f (%.3f .. %.3f)" % (name, dev[0], dev[1], dev[2]))
            continue
        lines.append("%-32s volym_set_clip_plane %8.3f (%.3f .. %.3f)   host zeroing + re-upload %8.1f (%.1f .. %.1f)   %.0fx"
                     % (name, dev[0], dev[1], dev[2], host[0], host[1], host[2], host[0] / dev[0]))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
