"""What the nearest pass and the fill cost (volym_nearest_pass, volym_fill_labels), on seeded synthetic bonsai volumes
with their label maps on the device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.

  the pass     the cases of profiles/distance.txt without INSIDE -- one segment (the canopy, label 2) and every label, over the whole
               volume and over a box of one eighth -- each beside the distance pass on the same request, in alternating blocks of
               --reps passes (HIP events around each pass, 5 warm-ups, inputs resident, --blocks blocks each): minimum over all
               passes, median of the block medians, their range (spread), and the ratio of the two medians.  The distance pass's
               kernels are byte for byte the parent commit's (profiles/nearest_units_asm_equal.txt), so the library's own pass stands
               for the parent's.  One pass is all its kernels.
  the fill     a nearest pass from canopy, trunk and pot, then the unlabelled matter within 3 texels joins the nearest of them: a host
               clock around volym_fill_labels, ending in volym_sync, --edit-reps times; between two fills an edit by the distance map
               of the same seeds sends the texels back (not timed).  Beside it, the edit by the table alone of the same texels: they
               are given label 7 once (by that distance map), then 7 <-> 8 alternate, every one timed.
  the host     once, at sizes up to --host-up-to: volym_read_labels, scipy.ndimage.distance_transform_edt(return_indices=True) on
               the seeds' mask, the labels at the indices, np.where, volym_set_labels and the segment table again.
  the kernels  --kernel-stats FILE... appends each kernel's share of the kernel time from kernel-statistics CSVs of profiler runs of
               this script (columns Name, TotalDurationNs): all cases together.

    python scripts/nearest_timing.py [--sizes 256,1024] [--reps 30] [--blocks 3] [--edit-reps 7] [--out profiles/nearest.txt] [--kernel-stats FILE...]
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

from scripts.distance_timing import _line  # noqa: E402
from scripts.measure_timing import _timed  # noqa: E402
from volym_amd import _lib, demo, scene, synth  # noqa: E402


def kernel_shares(path):
    """lines: the share of every nearest kernel in the summed kernel time of a profiler's kernel-statistics CSV; the two column sweeps
    are launches of one kernel"""
    total = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"volym_nearest_([a-z_]+?)_kernel", row.get("Name", ""))
            if m:
                total[m.group(1)] = total.get(m.group(1), 0.0) + float(row["TotalDurationNs"])
    whole = sum(total.get(k, 0.0) for k in ("init", "rows", "columns", "resolve")) or 1.0
    return ["each kernel's share of the kernel time of the nearest passes above (%s):" % os.path.basename(path)] + \
           ["    %-8s %5.1f %%" % (k, 100.0 * total.get(k, 0.0) / whole) for k in ("init", "rows", "columns", "resolve")]


def _ms(values):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(values)), float(np.min(values)), float(np.max(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--edit-reps", type=int, default=7)
    ap.add_argument("--host-up-to", type=int, default=256, help="largest size at which the host route is timed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    a = ap.parse_args()
    lines = ["nearest pass beside the distance pass, microseconds, HIP events around each of %d passes per block, %d alternating blocks each per case;" % (a.reps, a.blocks),
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
        table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}])
        with demo.GpuContext(640, 480, 0) as ctx:
            ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
            ctx.set_volume(vol, dims, 0)
            ctx.set_transfer_function(scene.default_lut())
            ctx.set_labels(lab, dims)
            ctx.set_segment_importances(table)
            lines.append("%d^3, %s layout, labels 0, 2, 3, 4 (%s texels)" % (n, "bricked" if n ** 3 > (64 << 20) else "linear", "{:,}".format(n ** 3)))
            for case, box, select in (("one segment (canopy)", whole, canopy), ("every label", whole, None), ("canopy, box of one eighth", eighth, canopy),
                                      ("every label, box of one eighth", eighth, None)):
                d = scene.Distance(box, 0, 1, select)
                ctx.distance_pass(d)                       # (the allocations)
                ctx.nearest_pass(d)
                dist, near = [], []
                for _ in range(a.blocks):
                    dist.append(_timed(stream, lambda: ctx.distance_pass(d), a.reps))
                    near.append(_timed(stream, lambda: ctx.nearest_pass(d), a.reps))
                summary = ctx.read_nearest()
                ratio = float(np.median([np.median(b) for b in near])) / float(np.median([np.median(b) for b in dist]))
                lines.append("  %s: %s texels in the box, %s solid, %d labels with a cell" % (
                    case, "{:,}".format(int(np.prod([h - l for l, h in zip(*box)]))), "{:,}".format(int(summary["n_solid"])), int((summary["cell"] != 0).sum())))
                lines += [_line("distance pass", dist), _line("nearest pass", near), "    nearest / distance, medians: %.2f" % ratio]
            # the fill
            seeds = scene.Distance(whole, 0, 1, scene.surface_select([2, 3, 4]))
            ctx.nearest_pass(seeds)
            ctx.distance_pass(seeds)
            fill = scene.Fill(whole, 0, (1, 255), scene.smooth_table([0]), scene.smooth_table([2, 3, 4]), (1, 9))
            back = scene.Relabel(whole, _lib.RELABEL_DISTANCE, (1, 255), {2: 0, 3: 0, 4: 0}, d2=(1, 9))
            changed = int(ctx.fill_labels(fill)["changed"])
            assert int(ctx.edit_labels(back)["changed"]) == changed, "the edit by the distance map must send back the texels the fill moved"
            ctx.sync()
            fills = []
            for _ in range(a.edit_reps):
                t0 = time.perf_counter()
                ctx.fill_labels(fill)
                ctx.sync()
                fills.append((time.perf_counter() - t0) * 1e3)
                ctx.edit_labels(back)
                ctx.sync()
            assert int(ctx.edit_labels(scene.Relabel(whole, _lib.RELABEL_DISTANCE, (1, 255), {0: 7}, d2=(1, 9)))["changed"]) == changed
            tables = []
            for r in range(2 * (a.edit_reps // 2) + 2):
                t0 = time.perf_counter()
                ctx.edit_labels(scene.Relabel(whole, to={7: 8} if r % 2 == 0 else {8: 7}))
                ctx.sync()
                tables.append((time.perf_counter() - t0) * 1e3)
            ctx.edit_labels(scene.Relabel(whole, to={7: 0}))
            lines += ["  the fill: the unlabelled matter within 3 texels of canopy, trunk or pot joins the nearest, %s texels; milliseconds, median (min .. max)" % "{:,}".format(changed),
                      "    volym_fill_labels                          %s" % _ms(fills),
                      "    volym_edit_labels, table alone, same texels %s" % _ms(tables[1:])]
            if n <= a.host_up_to:
                try:
                    from scipy import ndimage
                except ImportError:
                    lines.append("    the host route: scipy is not installed")
                else:
                    t0 = time.perf_counter()
                    now = ctx.read_labels()
                    solid = (vol.reshape(n, n, n) >= 1) & np.isin(now, (2, 3, 4))
                    t1 = time.perf_counter()
                    d2f, (iz, iy, ix) = ndimage.distance_transform_edt(~solid, return_indices=True)
                    t2 = time.perf_counter()
                    d2i = np.rint(d2f ** 2).astype(np.int64)
                    new = np.where((now == 0) & (vol.reshape(n, n, n) >= 1) & (d2i >= 1) & (d2i <= 9), now[iz, iy, ix], now)
                    ctx.set_labels(new.ravel(), dims)
                    ctx.set_segment_importances(table)
                    ctx.sync()
                    t3 = time.perf_counter()
                    assert int((new != now).sum()) == changed, "the host route must move the texels the fill moves"
                    lines.append("    the host route, once: volym_read_labels %.1f ms, scipy.ndimage.distance_transform_edt(return_indices=True) %.1f ms, "
                                 "np.where and the re-upload %.1f ms: %.1f ms" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        lines.append("")
        print("\n".join(lines[-30:]), flush=True)
    for path in a.kernel_stats:
        lines += kernel_shares(path) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
