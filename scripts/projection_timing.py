"""What a projection pass costs (volym_project_pass), on seeded synthetic bonsai volumes with their label maps on the
device: synth_bonsai(256) at 1920x1080 and 3840x2160, synth_bonsai(1024) at 3840x2160, step 0.0025, benchmark pose.

  the pass     (a fourth case: 256^3 at 1920x1080 under a crop box that keeps the middle half of every axis, so that there is
               empty space: the synthetic scene's air is noise.)  Whole frame, records and image (MAX | LABELS), default path and VOLYM_PROJECT_NO_SKIP: HIP events around each of --reps
               (>= 50) passes after 5 warm-ups, inputs resident; minimum and median.  Each path is timed in --blocks (3) blocks, the two
               paths in turn; the spread of a path is the range of its block medians, and a difference between the paths inside
               twice the larger spread is reported as no difference.  The records of the two paths are compared byte for byte.
  step sweep   synth_bonsai(256) at 1920x1080, without and with that crop box, steps 0.01, 0.0025 and 0.000625 (a quarter of the
               samples, and four times as many): both paths, one block of --reps passes each, median and samples per hit ray.  Time
               proportional to the samples of a ray while 4x the rays cost less than 4x says the pass is bound by its longest
               chains of dependent iterations, not by throughput.
  for scale    timed the same way in the same session: the whole-frame pick pass (alpha_min 0.5) and the default frame of the same
               view (after volym_settle).

    python scripts/projection_timing.py [--sizes 256,1024] [--reps 50] [--blocks 3] [--out profiles/projection.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from volym_amd import _lib, demo, scene, synth  # noqa: E402

# (w, h, crop): crop = the fraction of every axis a centred crop box keeps, None: no box (the synthetic scene's air is noise, not zeros:
# without a box it has no empty macro cell, with one everything outside it is empty)
CASES = {256: [(1920, 1080, None), (3840, 2160, None), (1920, 1080, 0.5)], 1024: [(3840, 2160, None)]}
STEP = 0.0025
SWEEP = (0.01, 0.0025, 0.000625)


def _timed(stream, fn, reps, warm=5):
    """microseconds of each of `reps` calls of fn (enqueue only), a HIP event on either side, after `warm` untimed ones"""
    for _ in range(warm):
        fn()
    stream.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record(stream)
    for i in range(reps):
        fn()
        ev[i + 1].record(stream)
    stream.synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["whole-frame projection pass (records and image, MAX | LABELS, step %g), benchmark pose; microseconds, HIP events around each of %d passes"
             % (STEP, a.reps), "per block; %d blocks per path, the paths in turn; min = minimum over all passes, median = median of the block medians," % a.blocks,
             "spread = range of the block medians", ""]
    sweep = ["", "step sweep: one block of %d passes per path, median" % a.reps]
    stream = torch.cuda.Stream()
    for n in (int(v) for v in a.sizes.split(",")):
        dims = (n, n, n)
        raw, labels = synth.synth_bonsai(n, with_labels=True)
        vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
        del raw, labels
        for w, h, crop in CASES[n]:
            with demo.GpuContext(w, h, 0) as ctx:
                ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
                ctx.set_volume(vol, dims, 0)
                ctx.set_transfer_function(scene.default_lut())
                ctx.set_labels(lab, dims)
                ctx.set_segment_importances(scene.segment_table([{"label_value": 2, "importance": 255}]))
                if crop is not None:
                    lo = int(n * (1.0 - crop) / 2.0)
                    ctx.set_crop_box((lo, lo, lo), (n - lo, n - lo, n - lo))
                state = scene.State.with_parameters(w / h, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
                state.update()
                ctx.update(state.camera_uniforms(), state.parameter_uniforms())
                paths = {"default": scene.Projection(STEP, _lib.PROJECT_MAX, _lib.PROJECT_LABELS, palette=np.full((256, 4), 96, np.uint8)),
                         "NO_SKIP": scene.Projection(STEP, _lib.PROJECT_MAX, _lib.PROJECT_LABELS | _lib.PROJECT_NO_SKIP, palette=np.full((256, 4), 96, np.uint8))}
                blocks = {k: [] for k in paths}
                records = {}
                for _ in range(a.blocks):
                    for k, p in paths.items():
                        blocks[k].append(_timed(stream, lambda: ctx.project_pass(p, own_image=True), a.reps))
                        records[k] = ctx.read_projection()
                same = records["default"].tobytes() == records["NO_SKIP"].tobytes()
                r = records["default"]
                hit = r["status"] > 0
                lines.append("%d^3 at %dx%d%s: %d of %d rays hit, %d with max > 0, %.0f samples per hit ray; records of the two paths %s"
                             % (n, w, h, "" if crop is None else ", crop box keeping the middle %g of every axis" % crop, int(hit.sum()), hit.size, int((r["status"] == 2).sum()), float(r["n_samples"][hit].mean()), "equal" if same else "DIFFER"))
                stat = {}
                for k, b in blocks.items():
                    med = [float(np.median(x)) for x in b]
                    stat[k] = (float(min(x.min() for x in b)), float(np.median(med)), max(med) - min(med))
                    lines.append("  projection pass, %-8s min %9.1f   median %9.1f   spread %6.1f" % ((k,) + stat[k]))
                diff = stat["NO_SKIP"][1] - stat["default"][1]
                bar = 2.0 * max(stat["default"][2], stat["NO_SKIP"][2])
                lines.append("  NO_SKIP - default = %.1f us; twice the larger spread = %.1f us: %s" % (
                    diff, bar, "no difference" if abs(diff) <= bar else ("skipping pays" if diff > 0 else "skipping COSTS")))
                if n == 256 and (w, h) == (1920, 1080):
                    sweep.append("256^3 at 1920x1080%s" % ("" if crop is None else ", crop box keeping the middle %g of every axis" % crop))
                    for step in SWEEP:
                        row = []
                        for flags in (_lib.PROJECT_LABELS, _lib.PROJECT_LABELS | _lib.PROJECT_NO_SKIP):
                            q = scene.Projection(step, _lib.PROJECT_MAX, flags, palette=np.full((256, 4), 96, np.uint8))
                            row.append(float(np.median(_timed(stream, lambda: ctx.project_pass(q, own_image=True), a.reps))))
                        rs = ctx.read_projection()
                        sweep.append("  step %-9g %6.0f samples per hit ray   default median %9.1f   NO_SKIP median %9.1f" % (
                            step, float(rs["n_samples"][rs["status"] > 0].mean()), row[0], row[1]))
                us = _timed(stream, lambda: ctx.pick_pass(None, 0.5), a.reps)
                lines.append("  pick pass, alpha_min 0.5    min %9.1f   median %9.1f   (for scale)" % (float(us.min()), float(np.median(us))))
                for _ in range(4):
                    ctx.compute_pass()
                ctx.settle()
                us = _timed(stream, ctx.compute_pass, a.reps)
                lines.append("  frame, default kernel       min %9.1f   median %9.1f   (for scale)" % (float(us.min()), float(np.median(us))))
                ctx.sync()
            print("\n".join(lines[-6:]), flush=True)
    lines += sweep
    print("\n".join(sweep), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
