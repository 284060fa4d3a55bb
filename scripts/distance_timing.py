"""What the distance pass costs (volym_distance_pass), on seeded synthetic bonsai volumes with their label maps on the
device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.

  the pass     one segment (the canopy, label 2) and every label, over the whole volume and over a box of one eighth (the middle half
               of every axis), without and with INSIDE.  HIP events around each of --reps passes after 5 warm-ups, inputs resident,
               --blocks blocks per case; minimum over all passes, median of the block medians, and their range (spread).  One pass is
               all its kernels: zeroing, rows, the two column sweeps, finish, pack.
  for scale    in the same session, on the same volume and box: volym_measure_pass and volym_components_pass; and at 256^3, on a
               ready-made host mask (no download counted), scipy.ndimage.distance_transform_edt where scipy is installed, whose square
               is compared with the pass's map.
  the kernels  --kernel-stats FILE... appends each kernel's share of the kernel time from kernel-statistics CSVs of profiler runs of
               this script, one per size (columns Name, TotalDurationNs): all cases together.

    python scripts/distance_timing.py [--sizes 256,1024] [--reps 30] [--blocks 3] [--out profiles/distance.txt] [--kernel-stats FILE...]
"""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from scripts.measure_timing import _timed  # noqa: E402
from volym_amd import _lib, demo, scene, synth  # noqa: E402


def _line(name, blocks):
    med = [float(np.median(b)) for b in blocks]
    return "    %-16s min %10.1f   median %10.1f   spread %7.1f" % (name, float(min(b.min() for b in blocks)), float(np.median(med)), max(med) - min(med))


def kernel_shares(path):
    """lines: the share of every distance kernel in the summed kernel time of a profiler's kernel-statistics CSV; the two column sweeps
    are launches of one kernel"""
    total = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"volym_distance_([a-z_]+?)_kernel", row.get("Name", ""))
            if m:
                total[m.group(1)] = total.get(m.group(1), 0.0) + float(row["TotalDurationNs"])
    whole = sum(total.values()) or 1.0
    return ["each kernel's share of the kernel time of the passes above (%s):" % os.path.basename(path)] + \
           ["    %-8s %5.1f %%" % (k, 100.0 * total.get(k, 0.0) / whole) for k in ("init", "rows", "columns", "finish", "pack")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--host-up-to", type=int, default=256, help="largest size at which scipy is timed on the host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    a = ap.parse_args()
    lines = ["distance pass, microseconds, HIP events around each of %d passes per block, %d blocks per case;" % (a.reps, a.blocks),
             "min = minimum over all passes, median = median of the block medians, spread = range of the block medians", ""]
    stream = torch.cuda.Stream()
    for n in (int(v) for v in a.sizes.split(",") if v):
        dims = (n, n, n)
        raw, labels = synth.synth_bonsai(n, with_labels=True)
        vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
        del raw, labels
        q = n // 4
        whole, eighth = ((0, 0, 0), dims), ((q, q, q), (n - q, n - q, n - q))
        canopy = scene.surface_select([2])
        with demo.GpuContext(640, 480, 0) as ctx:
            ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            lines.append("%d^3, %s layout, labels 0, 2, 3, 4 (%s texels)" % (n, "bricked" if n ** 3 > (64 << 20) else "linear", "{:,}".format(n ** 3)))
            for case, box, select in (("one segment (canopy)", whole, canopy), ("every label", whole, None), ("canopy, box of one eighth", eighth, canopy),
                                      ("every label, box of one eighth", eighth, None)):
                for flags in (0, _lib.DISTANCE_INSIDE):
                    d = scene.Distance(box, flags, 1, select)
                    ctx.distance_pass(d)                   # (the allocations)
                    passes = [_timed(stream, lambda: ctx.distance_pass(d), a.reps) for _ in range(a.blocks)]
                    summary = ctx.read_distance()
                    lines.append("  %s%s: %s texels in the box, %s solid, max d2 %d" % (
                        case, ", INSIDE" if flags else "", "{:,}".format(int(np.prod([h - l for l, h in zip(*box)]))), "{:,}".format(int(summary["n_solid"])),
                        int(summary["max_d2"])))
                    lines.append(_line("distance pass", passes))
                    if n <= a.host_up_to:
                        try:
                            from scipy import ndimage
                        except ImportError:
                            lines.append("    scipy.ndimage.distance_transform_edt: scipy is not installed")
                        else:
                            sub = (slice(box[0][2], box[1][2]), slice(box[0][1], box[1][1]), slice(box[0][0], box[1][0]))
                            solid = (vol.reshape(n, n, n)[sub] >= 1) & (np.asarray(d.select)[lab.reshape(n, n, n)[sub]] != 0)
                            mask = np.pad(solid, 1) if flags else ~solid
                            t0 = time.perf_counter()
                            edt = ndimage.distance_transform_edt(mask)
                            secs = time.perf_counter() - t0
                            if flags:
                                edt = edt[1:-1, 1:-1, 1:-1]
                            same = np.array_equal(np.rint(edt ** 2).astype(np.uint32), ctx.read_distance_map())
                            lines.append("    scipy.ndimage.distance_transform_edt on a ready-made mask: %.1f ms; its square %s the pass's map" % (
                                secs * 1e3, "equals" if same else "DIFFERS FROM"))
                measure = [_timed(stream, lambda: ctx.measure_pass(scene.Measure(box)), a.reps) for _ in range(a.blocks)]
                comps = [_timed(stream, lambda: ctx.components_pass(scene.Components(box, 0, 1, select)), a.reps) for _ in range(a.blocks)]
                lines += [_line("measure pass", measure), _line("components pass", comps)]
        lines.append("")
        print("\n".join(lines[-40:]), flush=True)
    for path in a.kernel_stats:
        lines += kernel_shares(path) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
