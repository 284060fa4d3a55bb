"""What the components pass costs (volym_components_pass), on seeded synthetic bonsai volumes with their label maps on
the device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.

  the pass     one segment (the canopy, label 2), every label (the solid density >= 1 as it links across segments), and the canopy
               inside a box of one eighth (the middle half of every axis).  HIP events around each of --reps passes after 5 warm-ups,
               inputs resident, --blocks blocks per case; minimum over all passes, median of the block medians, and their range
               (spread).  One pass is all its kernels: zeroing, rows, merge, flatten, the three scan kernels, number, relabel, pack.
  for scale    in the same session, on the same volume and box: volym_measure_pass and volym_surface_pass (the count pass and its
               scan); and at 256^3, on host copies (the download of the two volumes not counted), scene.components_volume, the NumPy
               twin, whose bytes are compared with the pass's, and scipy.ndimage.label with the 6-connected structure where scipy is
               installed.
  the kernels  --kernel-stats FILE... appends each kernel's share of the kernel time from kernel-statistics CSVs of profiler runs of
               this script, one per size (columns Name, TotalDurationNs): the three cases together, the scan kernels as one.

    python scripts/components_timing.py [--sizes 256,1024] [--reps 30] [--blocks 3] [--out profiles/components.txt] [--kernel-stats FILE...]
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
from volym_amd import demo, scene, synth  # noqa: E402


def _line(name, blocks):
    med = [float(np.median(b)) for b in blocks]
    return "    %-16s min %10.1f   median %10.1f   spread %7.1f" % (name, float(min(b.min() for b in blocks)), float(np.median(med)), max(med) - min(med))


def kernel_shares(path):
    """lines: the share of every components kernel in the summed kernel time of a profiler's kernel-statistics CSV"""
    total = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"volym_components_([a-z_]+?)_kernel", row.get("Name", ""))
            if m:
                step = "scan" if m.group(1).startswith("scan") else m.group(1)
                total[step] = total.get(step, 0.0) + float(row["TotalDurationNs"])
    whole = sum(total.values()) or 1.0
    order = ["init", "rows", "merge", "flatten", "scan", "number", "relabel", "pack"]
    return ["each kernel's share of the kernel time of the passes above (%s):" % os.path.basename(path)] + \
           ["    %-8s %5.1f %%" % (k, 100.0 * total.get(k, 0.0) / whole) for k in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--twin-up-to", type=int, default=256, help="largest size at which the NumPy twin and scipy are timed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    a = ap.parse_args()
    lines = ["components pass, microseconds, HIP events around each of %d passes per block, %d blocks per case;" % (a.reps, a.blocks),
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
            for case, box, select in (("one segment (canopy)", whole, canopy), ("every label", whole, None), ("canopy, box of one eighth", eighth, canopy)):
                c = scene.Components(box, 0, 1, select)
                ctx.components_pass(c)                  # (the allocations)
                passes = [_timed(stream, lambda: ctx.components_pass(c), a.reps) for _ in range(a.blocks)]
                summary = ctx.read_components()
                measure = [_timed(stream, lambda: ctx.measure_pass(scene.Measure(box)), a.reps) for _ in range(a.blocks)]
                surface = [_timed(stream, lambda: ctx.surface_pass(scene.Surface(box, 0, 1, select)), a.reps) for _ in range(a.blocks)]
                lines.append("  %s: %s texels in the box, %s solid, %s components" % (
                    case, "{:,}".format(int(np.prod([h - l for l, h in zip(*box)]))), "{:,}".format(int(summary["n_solid"])), "{:,}".format(int(summary["n_components"]))))
                lines += [_line("components pass", passes), _line("measure pass", measure), _line("surface count", surface)]
                if n <= a.twin_up_to:
                    got = summary, ctx.read_component_table(summary["recorded"]), ctx.read_component_ids()
                    t0 = time.perf_counter()
                    want = scene.components_volume(vol, dims, c, labels=lab)
                    secs = time.perf_counter() - t0
                    same = all(np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want))
                    lines.append("    NumPy twin on host copies: %.1f ms; summary, table and ids %s the pass's" % (secs * 1e3, "equal" if same else "DIFFER FROM"))
                    try:
                        from scipy import ndimage
                    except ImportError:
                        lines.append("    scipy.ndimage.label: scipy is not installed")
                    else:
                        solid = want[2] != 0xFFFFFFFF
                        t0 = time.perf_counter()
                        _, found = ndimage.label(solid, structure=ndimage.generate_binary_structure(3, 1))
                        lines.append("    scipy.ndimage.label on the solid mask: %.1f ms, %d components" % ((time.perf_counter() - t0) * 1e3, found))
        lines.append("")
        print("\n".join(lines[-24:]), flush=True)
    for path in a.kernel_stats:
        lines += kernel_shares(path) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
