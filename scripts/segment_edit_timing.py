"""Time one segment-importance edit two ways, on seeded synthetic bonsai volumes (256^3 and 1024^3):
  host   -- volym_map_segments_to_importance over the raw labels, volym_prepare_volume, volym_set_importances
            (the reference's flow: map on the host, upload, re-brick, host scan for the important box);
  device -- volym_set_segment_importances on labels kept on the device by volym_set_labels.
Each figure is a host clock around the call, ending in volym_sync; median of --reps edits alternating two tables.
The map kernel alone (volym_segment_map_kernel) comes from a separate run under `rocprofv3 --kernel-trace --stats`.

    python scripts/segment_edit_timing.py [--sizes 256,1024] [--reps 5] [--out profiles/segment_importances.txt]
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


def run(n, reps):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    segs = [[{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}],
            [{"label_value": 3, "importance": 255}, {"label_value": 4, "importance": 200}]]
    tables = [scene.segment_table(s) for s in segs]
    out = {}
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        t0 = time.perf_counter()
        ctx.set_labels(lab, dims)
        ctx.sync()
        out["set_labels_ms"] = (time.perf_counter() - t0) * 1e3
        dev, host = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            ctx.set_segment_importances(tables[r % 2])
            ctx.sync()
            dev.append((time.perf_counter() - t0) * 1e3)
        for r in range(reps):
            t0 = time.perf_counter()
            imp = scene.prepare_volume(scene.map_segments_to_importance(labels, segs[r % 2]), dims, True)
            ctx.set_importances(imp, dims)
            ctx.sync()
            host.append((time.perf_counter() - t0) * 1e3)
        out["device_ms"] = float(np.median(dev[1:]))      # (the first edit allocates the importance volume)
        out["device_first_ms"] = dev[0]
        out["host_ms"] = float(np.median(host))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in (int(s) for s in a.sizes.split(",")):
        r = run(n, a.reps)
        lines.append("%d^3: set_segment_importances %.3f ms (first edit %.3f ms), host map + set_importances %.1f ms (%.0fx), "
                     "set_labels %.1f ms" % (n, r["device_ms"], r["device_first_ms"], r["host_ms"], r["host_ms"] / r["device_ms"],
                                             r["set_labels_ms"]))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
