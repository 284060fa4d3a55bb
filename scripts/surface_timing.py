"""What the surface passes cost (volym_surface_pass / volym_surface_faces_pass), on seeded synthetic bonsai volumes
with their label maps on the device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.

  the passes   one segment (the canopy, label 2), every label (the isosurface density >= 1 with its faces booked per label), and the
               canopy inside a box of one eighth (the middle half of every axis).  Per case three timings, HIP events around each of
               --reps passes after 5 warm-ups, inputs resident, --blocks blocks per case; minimum over all passes, median of the
               block medians, and their range (spread):
                 count+scan  volym_surface_pass: the zeroing kernel, the count pass and the three scan kernels;
                 rows only   volym_surface_pass over a box one texel wide with the same rows: the same scan, and a count pass that
                             reads one texel per row -- an upper bound of the scan's share;
                 emit        volym_surface_faces_pass into the context's own buffer.
  for scale    in the same session, on the same volume: volym_measure_pass over the same box (it reads the same two bytes per texel
               once), and at 256^3 scene.surface_volume, the NumPy twin, on host copies (the download of the two volumes not counted).

    python scripts/surface_timing.py [--sizes 256,1024] [--reps 30] [--blocks 3] [--out profiles/surface.txt]
"""
import argparse
import os
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
    return "    %-12s min %9.1f   median %9.1f   spread %6.1f" % (name, float(min(b.min() for b in blocks)), float(np.median(med)), max(med) - min(med))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--twin-up-to", type=int, default=256, help="largest size at which the NumPy twin is timed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["surface passes, microseconds, HIP events around each of %d passes per block, %d blocks per case;" % (a.reps, a.blocks),
             "min = minimum over all passes, median = median of the block medians, spread = range of the block medians", ""]
    stream = torch.cuda.Stream()
    for n in (int(v) for v in a.sizes.split(",")):
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
                s = scene.Surface(box, 0, 1, select)
                narrow = scene.Surface(((box[0][0], box[0][1], box[0][2]), (box[0][0] + 1, box[1][1], box[1][2])), 0, 1, select)
                both = [_timed(stream, lambda: ctx.surface_pass(s), a.reps) for _ in range(a.blocks)]
                total = int(ctx.read_surface()["total"])
                rows = [_timed(stream, lambda: ctx.surface_pass(narrow), a.reps) for _ in range(a.blocks)]
                ctx.surface_pass(s)
                emit = [_timed(stream, ctx.surface_faces_pass, a.reps) for _ in range(a.blocks)]
                measure = [_timed(stream, lambda: ctx.measure_pass(scene.Measure(box)), a.reps) for _ in range(a.blocks)]
                lines.append("  %s: %s rows, %s faces" % (case, "{:,}".format((box[1][1] - box[0][1]) * (box[1][2] - box[0][2])), "{:,}".format(total)))
                lines += [_line("count+scan", both), _line("rows only", rows), _line("emit", emit), _line("measure pass", measure)]
                if n <= a.twin_up_to:
                    got = ctx.read_surface(), ctx.read_surface_faces(total)
                    t0 = time.perf_counter()
                    want = scene.surface_volume(vol, dims, s, labels=lab)
                    secs = time.perf_counter() - t0
                    same = got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
                    lines.append("    NumPy twin on host copies: %.1f ms; summary and faces %s the passes'" % (secs * 1e3, "equal" if same else "DIFFER FROM"))
        lines.append("")
        print("\n".join(lines[-20:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
