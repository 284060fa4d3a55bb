"""What the interpolate pass and the edit by it cost (volym_interpolate_pass, volym_interpolate_labels), on seeded
synthetic bonsai volumes with their label maps on the device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the
bricked one.  The canopy (label 2) is kept on every 8th slice along the case's axis and taken off the slices between, as a person who
paints key slices leaves it; the cases are that segment along z and along x.  volym_distance_pass of the same box and selection,
measured in the same run in alternating blocks, is the yardstick: what the planes, the second map and the decision cost is the ratio to it.

  the pass     HIP events around each of --reps passes per block, --blocks blocks per pass and case, interpolate and distance blocks
               alternating: minimum over all passes, median of the block medians, their range (spread), and the ratio of the medians.
  the edit     after the pass: a host clock around volym_interpolate_labels (the unlabelled texels the shape holds join the canopy),
               ending in volym_sync, --edit-reps times; between two the same snapshot sends them back.  Beside it volym_edit_labels
               with a table alone over the same texels.
  the host     once, at sizes up to --host-up-to: volym_read_labels, the NumPy twins, volym_set_labels and the table again.

    python scripts/interpolate_timing.py [--sizes 256,1024] [--reps 20] [--blocks 3] [--edit-reps 7] [--out profiles/interpolate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from scripts.distance_timing import _line  # noqa: E402
from scripts.measure_timing import _timed  # noqa: E402
from scripts.nearest_timing import _ms  # noqa: E402
from volym_amd import _lib, demo, scene, synth  # noqa: E402

EVERY = 8


def painted(lab, n, axis, label=2):
    """the labels with `label` kept on every 8th slice along `axis` and 0 on the slices between, and those key slices"""
    out = lab.reshape(n, n, n).copy()
    keys = tuple(range(0, n, EVERY))
    gap = np.ones(n, bool)
    gap[list(keys)] = False
    view = np.moveaxis(out, 2 - axis, 0)
    view[gap] = np.where(view[gap] == label, 0, view[gap])
    return out.ravel(), keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--edit-reps", type=int, default=7)
    ap.add_argument("--host-up-to", type=int, default=256, help="largest size at which the host route is timed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["interpolate pass beside the distance pass of the same box and selection, microseconds, HIP events around each of %d passes per block, "
             "%d alternating blocks each per case;" % (a.reps, a.blocks),
             "min = minimum over all passes, median = median of the block medians, spread = range of the block medians; ratio = interpolate median / distance median", ""]
    stream = torch.cuda.Stream()
    for n in (int(v) for v in a.sizes.split(",") if v):
        dims = (n, n, n)
        raw, labels = synth.synth_bonsai(n, with_labels=True)
        vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
        del raw, labels
        whole = ((0, 0, 0), dims)
        canopy = scene.surface_select([2])
        table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}])
        with demo.GpuContext(640, 480, 0) as ctx:
            ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
            ctx.set_volume(vol, dims, 0)
            ctx.set_transfer_function(scene.default_lut())
            lines.append("%d^3, %s layout, labels 0, 2, 3, 4 (%s texels), the canopy on every %dth slice" % (
                n, "bricked" if n ** 3 > (64 << 20) else "linear", "{:,}".format(n ** 3), EVERY))
            for axis in (2, 0):
                sparse, keys = painted(lab, n, axis)
                ctx.set_labels(sparse, dims)
                ctx.set_segment_importances(table)
                q = scene.Interpolate(whole, 0, 1, canopy, (1, 1, 1), axis)  # (min_byte 1, the least the distance pass takes: the same selection)
                d = scene.Distance(whole, 0, 1, canopy)
                ctx.distance_pass(d)                       # (the allocations)
                ctx.interpolate_pass(q)
                dist, inter = [], []
                for _ in range(a.blocks):
                    inter.append(_timed(stream, lambda: ctx.interpolate_pass(q), a.reps))
                    dist.append(_timed(stream, lambda: ctx.distance_pass(d), a.reps))
                s = ctx.read_interpolate()
                assert int(s["n_keys"]) <= len(keys) and int(s["n_gaps"]) >= 1, "the painted canopy must leave gaps between its keys"
                ratio = float(np.median([np.median(b) for b in inter])) / float(np.median([np.median(b) for b in dist]))
                lines.append("  the canopy along %s: %d key slices, %d gaps of %d slices, %s SHAPE texels, %s INSIDE on the gap slices" % (
                    "xyz"[axis], int(s["n_keys"]), int(s["n_gaps"]), int(s["n_gap_slices"]), "{:,}".format(int(s["n_shape"])), "{:,}".format(int(s["n_inside"]))))
                lines += [_line("interpolate pass", inter), _line("distance pass", dist), "    interpolate / distance, medians: %.2f" % ratio]
                # the edit, by the snapshot the passes above left
                fill = scene.InterpolateEdit(whole, to={0: 2})
                back = scene.InterpolateEdit(whole, to={2: 0})
                changed = int(ctx.interpolate_labels(fill)["changed"])
                assert 0 < changed <= int(s["n_new"]) and int(ctx.interpolate_labels(back)["changed"]) == changed, "the same snapshot must send the texels back"
                ctx.sync()
                fills = []
                for _ in range(a.edit_reps):
                    t0 = time.perf_counter()
                    ctx.interpolate_labels(fill)
                    ctx.sync()
                    fills.append((time.perf_counter() - t0) * 1e3)
                    ctx.interpolate_labels(back)
                    ctx.sync()
                moved = int(ctx.interpolate_labels(scene.InterpolateEdit(whole, to={0: 7}))["changed"])
                tables = []
                for r in range(2 * (a.edit_reps // 2) + 2):
                    t0 = time.perf_counter()
                    ctx.edit_labels(scene.Relabel(whole, to={7: 8} if r % 2 == 0 else {8: 7}))
                    ctx.sync()
                    tables.append((time.perf_counter() - t0) * 1e3)
                ctx.edit_labels(scene.Relabel(whole, to={7: 0}))
                lines += ["    the edit: the unlabelled texels the interpolated canopy holds join it, %s texels; milliseconds, median (min .. max)" % "{:,}".format(moved),
                          "      volym_interpolate_labels                    %s" % _ms(fills),
                          "      volym_edit_labels, table alone, same texels %s" % _ms(tables[1:])]
                if n <= a.host_up_to:
                    t0 = time.perf_counter()
                    now = ctx.read_labels()
                    t1 = time.perf_counter()
                    snap = scene.interpolate_volume(vol, dims, q, labels=now.ravel())
                    new, result = scene.interpolate_labels_volume(vol, dims, fill, now.ravel(), snap[2], q.box)
                    t2 = time.perf_counter()
                    ctx.set_labels(new.ravel(), dims)
                    ctx.set_segment_importances(table)
                    ctx.sync()
                    t3 = time.perf_counter()
                    assert int(result["changed"]) == moved, "the host route must move the texels the edit moves"
                    lines.append("    the host route, once: volym_read_labels %.1f ms, the NumPy twins %.1f ms, the re-upload %.1f ms: %.1f ms" % (
                        (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        lines.append("")
        print("\n".join(lines[-24:]), flush=True)
        if a.out:                                       # (after every size: a run cut short keeps what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
