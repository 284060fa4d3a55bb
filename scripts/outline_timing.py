"""What an outline pass costs (volym_outline_pass), on seeded synthetic bonsai volumes with their label maps on the
device: standing views of synth_bonsai(256) at 1920x1080 and 3840x2160 and of synth_bonsai(1024) at 3840x2160, the canopy selected,
records of a whole-frame pick pass (alpha_min 0.5).

Timed per case, all in one session and on one stream, HIP events around each of --reps (>= 50) calls after 5 warm-ups, minimum and
median in microseconds (copy and passes: two such runs each, alternating, pooled):

  outline pass            radius 1 and radius 8, into the context's own target
  copy                    a device-to-device copy of 12 * W * H bytes: it moves 24 * W * H bytes in all, what the pass moves
                          (16 + 4 read, 4 written per pixel)
  two launches            two near-empty kernel launches back to back: the outline pass of a 64 x 16 frame (one block each), through
                          the same launch path
  pick pass, frame        for scale

So that the events time the device and not the host's enqueue rate, every timed run is enqueued behind a long matrix product on
the same stream: the host has enqueued all of it before the device starts on it.

The bar: the pass's median must not exceed the copy's median + the two launches' median + the copy's own spread (median - minimum).

    python scripts/outline_timing.py [--sizes 256,1024] [--reps 50] [--out profiles/outline_pass.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from volym_amd import _lib, demo, scene, synth  # noqa: E402

CASES = {256: [(1920, 1080), (3840, 2160)], 1024: [(3840, 2160)]}
RING, FILL = (255, 255, 0, 255), (255, 255, 0, 48)


def _timed(stream, fn, reps, plug, warm=5):
    """microseconds of each of `reps` calls of fn (enqueue only), a HIP event on either side, after `warm` untimed ones"""
    for _ in range(warm):
        fn()
    stream.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    plug()
    ev[0].record(stream)
    for i in range(reps):
        fn()
        ev[i + 1].record(stream)
    stream.synchronize()
    return np.array([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps)])


def _mm(us):
    return float(np.min(us)), float(np.median(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    stream = torch.cuda.Stream()
    canopy = scene.selection_mask([2])
    lines = ["outline pass against a device-to-device copy of the bytes it moves; microseconds, minimum / median of %d, HIP events around each" % a.reps,
             "bar: pass median <= copy median + two-launch median + copy spread (median - minimum)", ""]
    ok = True
    with torch.cuda.stream(stream):
        m = torch.ones((8192, 8192), dtype=torch.float32, device="cuda")
        plug = lambda: torch.mm(m, m)
        with demo.GpuContext(64, 16, 0) as tiny:
            tiny.set_stream(stream.cuda_stream)
            dims, raw_lab = (16, 16, 16), synth.synth_bonsai(16, with_labels=True)
            tiny.set_volume(scene.prepare_volume(raw_lab[0], dims, True), dims, 0)
            tiny.set_transfer_function(scene.default_lut())
            tiny.set_labels(scene.prepare_volume(raw_lab[1], dims, True), dims)
            tiny.set_segment_importances(scene.segment_table([{"label_value": 2, "importance": 255}]))
            state = scene.State.with_parameters(4.0, scene.StateParameters.benchmark())
            state.update()
            tiny.update(state.camera_uniforms(), state.parameter_uniforms())
            tiny.compute_pass()
            tiny.pick_pass(None, 0.5)
            launches = _mm(_timed(stream, lambda: tiny.outline_pass(canopy, RING, FILL, 1), a.reps, plug))
            tiny.sync()
        lines += ["two near-empty launches (outline pass of a 64 x 16 frame)   %8.1f / %8.1f" % launches, ""]
        for n in sizes:
            dims = (n, n, n)
            raw, labels = synth.synth_bonsai(n, with_labels=True)
            vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
            del raw, labels
            for w, h in CASES[n]:
                with demo.GpuContext(w, h, 0) as ctx:
                    ctx.set_stream(stream.cuda_stream)
                    ctx.set_volume(vol, dims, 0)
                    ctx.set_transfer_function(scene.default_lut())
                    ctx.set_labels(lab, dims)
                    ctx.set_segment_importances(scene.segment_table([{"label_value": 2, "importance": 255}]))
                    state = scene.State.with_parameters(w / h, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
                    state.update()
                    ctx.update(state.camera_uniforms(), state.parameter_uniforms())
                    for _ in range(4):
                        ctx.compute_pass()
                    ctx.settle()
                    frame = _mm(_timed(stream, ctx.compute_pass, a.reps, plug))
                    pick = _mm(_timed(stream, lambda: ctx.pick_pass(None, 0.5), a.reps, plug))
                    recs = ctx.read_picks()
                    n_sel = int(((recs["status"] == 2) & (recs["label"] == 2)).sum())
                    del recs
                    src = torch.zeros(12 * w * h, dtype=torch.uint8, device="cuda")
                    dst = torch.zeros(12 * w * h, dtype=torch.uint8, device="cuda")
                    rows = {}
                    for k in range(2):                                  # copy, passes, copy again and passes again: alternating, then pooled
                        rows.setdefault("copy", []).append(_timed(stream, lambda: dst.copy_(src), a.reps, plug))
                        for radius in (1, 8):
                            rows.setdefault(radius, []).append(_timed(stream, lambda: ctx.outline_pass(canopy, RING, FILL, radius), a.reps, plug))
                    ctx.sync()
                    del src, dst
                best = {k: _mm(np.concatenate(v)) for k, v in rows.items()}      # both runs of each, pooled
                copy = best["copy"]
                bar = copy[1] + launches[1] + (copy[1] - copy[0])
                lines.append("%d^3 at %dx%d, %d pixels selected" % (n, w, h, n_sel))
                for radius in (1, 8):
                    mn, med = best[radius]
                    verdict = "within" if med <= bar else "ABOVE (by %.1f)" % (med - bar)
                    ok = ok and med <= bar
                    lines.append("  outline pass, radius %d        %9.1f / %9.1f   %s the bar of %.1f" % (radius, mn, med, verdict, bar))
                lines.append("  copy of %d bytes        %9.1f / %9.1f   (%.0f GB/s read + written at the median)" % (12 * w * h, copy[0], copy[1], 24 * w * h / copy[1] / 1e3))
                lines.append("  every run (min / median): copy %s; radius 1 %s; radius 8 %s" % tuple(
                    ", ".join("%.1f / %.1f" % _mm(t) for t in rows[k]) for k in ("copy", 1, 8)))
                lines.append("  whole-frame pick pass         %9.1f / %9.1f   (for scale)" % pick)
                lines.append("  frame, default kernel         %9.1f / %9.1f   (for scale)" % frame)
            del vol, lab
    lines.append("")
    lines.append("every outline pass within its bar" if ok else "an outline pass exceeds its bar: see DESIGN.md 4.7")
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
