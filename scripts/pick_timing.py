"""What a pick pass costs (volym_pick_pass), on seeded synthetic bonsai volumes with their label maps on the device.

  whole-frame pass   alpha_min = 0 and 0.5: synth_bonsai(256) at 1920x1080 and 3840x2160, synth_bonsai(1024) at 3840x2160 (base
                     parameters and straight look-ahead 15).  HIP events around each of --reps (>= 50) passes after 5 warm-ups, inputs
                     resident: minimum and median.  Beside it, timed the same way in the same session: the frame of VOLYM_OPT_KERNEL = 1
                     -- the same launch shape and leaps, a superset of the work per ray -- and the default kernel's frame (after
                     volym_settle) for scale.  With --parent-lib those frames come from a child process that loads that library (the
                     build of the parent commit); the pass's median must not exceed the parent's kernel-1 median by more than that
                     measurement's own spread (median - minimum).
  one pixel          volym_pick: wall clock of the blocking call, median of 200.
  frame loop         a standing view at 1920x1080, volym_throttle(3) pacing: wall clock per frame with and without a whole-frame
                     pick pass enqueued behind every frame.

    python scripts/pick_timing.py [--sizes 256,1024] [--reps 50] [--parent-lib PATH] [--out profiles/pick_pass.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from volym_amd import _lib, demo, scene, synth  # noqa: E402

STRAIGHT = dict(use_importance_rendering=1, importance_check_ahead_steps=15)
CASES = {256: [((1920, 1080), "base", {}), ((3840, 2160), "base", {})],
         1024: [((3840, 2160), "base", {}), ((3840, 2160), "straight 15", STRAIGHT)]}


def _scene(n):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    return dims, vol, lab


def _context(w, h, dims, vol, lab, kernel, stream):
    ctx = demo.GpuContext(w, h, 0)
    ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
    ctx.set_option(_lib.OPT_KERNEL, kernel)
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut())
    ctx.set_labels(lab, dims)
    ctx.set_segment_importances(scene.segment_table([{"label_value": 2, "importance": 255}]))
    return ctx


def _update(ctx, w, h, kw):
    state = scene.State.with_parameters(w / h, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01, **kw))
    state.update()
    ctx.update(state.camera_uniforms(), state.parameter_uniforms())


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


def frames(sizes, reps):
    """{"n w h name": {"kernel 1": (min, median), "default": (min, median)}} of this process's library"""
    out = {}
    stream = torch.cuda.Stream()
    for n in sizes:
        dims, vol, lab = _scene(n)
        for (w, h), name, kw in CASES[n]:
            row = {}
            for label, kernel in (("kernel 1", 1), ("default", 2)):
                with _context(w, h, dims, vol, lab, kernel, stream) as ctx:
                    _update(ctx, w, h, kw)
                    for _ in range(4):
                        ctx.compute_pass()
                    ctx.settle()
                    us = _timed(stream, ctx.compute_pass, reps)
                    row[label] = (float(us.min()), float(np.median(us)))
                    ctx.sync()
            out["%d %d %d %s" % (n, w, h, name)] = row
    return out


def picks(sizes, reps):
    out = {}
    extra = {}
    stream = torch.cuda.Stream()
    for n in sizes:
        dims, vol, lab = _scene(n)
        for (w, h), name, kw in CASES[n]:
            with _context(w, h, dims, vol, lab, 2, stream) as ctx:
                _update(ctx, w, h, kw)
                for _ in range(4):
                    ctx.compute_pass()                       # (the slot's distance field exists from the first frame on)
                ctx.settle()
                row = {}
                for a_min in (0.0, 0.5):
                    us = _timed(stream, lambda: ctx.pick_pass(None, a_min), reps)
                    r = ctx.read_picks()
                    row["alpha_min %.1f" % a_min] = (float(us.min()), float(np.median(us)), int((r["status"] == 2).sum()))
                out["%d %d %d %s" % (n, w, h, name)] = row
                if n == sizes[0] and (w, h) == (1920, 1080):
                    ys, xs = np.nonzero(r["status"] == 2)
                    x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
                    lat = []
                    for _ in range(210):
                        t0 = time.perf_counter()
                        ctx.pick(x, y, 0.5)
                        lat.append((time.perf_counter() - t0) * 1e6)
                    extra["one pixel"] = (float(np.median(lat[10:])), float(np.min(lat[10:])))
                    for with_pick in (False, True):
                        def loop(k):
                            for _ in range(k):
                                ctx.compute_pass()
                                if with_pick:
                                    ctx.pick_pass(None, 0.5)
                                ctx.throttle(3)
                            ctx.sync()
                        loop(50)
                        t0 = time.perf_counter()
                        loop(400)
                        extra["loop with pick" if with_pick else "loop"] = (time.perf_counter() - t0) / 400 * 1e6
    return out, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--parent-lib", default=None, help="libvolym_hip.so built from the parent commit: its frames are timed in a child process")
    ap.add_argument("--frames-only", action="store_true", help="(the child's role) print the frame timings of the loaded library as JSON")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    if a.frames_only:
        for name in ("volym_pick_pass", "volym_read_picks", "volym_pick_device_ptr", "volym_pick"):
            _lib.SIGNATURES.pop(name)             # the parent's library has no pick calls: this process does not bind them
        print("FRAMES " + json.dumps(frames(sizes, a.reps)), flush=True)
        return
    if a.parent_lib:
        env = dict(os.environ, VOLYM_HIP_LIB=os.path.abspath(a.parent_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames-only", "--sizes", a.sizes, "--reps", str(a.reps)], env=env,
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit("the child that times the parent's frames failed:\n" + p.stderr[-2000:])
        ref = json.loads(next(l for l in p.stdout.split("\n") if l.startswith("FRAMES "))[7:])
        whose = "parent commit's library"
    else:
        ref = frames(sizes, a.reps)
        whose = "this library"
    got, extra = picks(sizes, a.reps)
    lines = ["whole-frame pick pass against frames of the same scene and size; microseconds, minimum / median of %d, HIP events around each" % a.reps,
             "frames: %s" % whose, ""]
    ok = True
    for key, row in got.items():
        n, w, h, name = key.split(" ", 3)
        k1, dflt = ref[key]["kernel 1"], ref[key]["default"]
        spread = k1[1] - k1[0]
        lines.append("%s^3 at %sx%s, %s" % (n, w, h, name))
        for label, (mn, med, n_picked) in row.items():
            verdict = "within" if med <= k1[1] + spread else "ABOVE"
            ok = ok and verdict == "within"
            lines.append("  pick pass, %-14s %9.1f / %9.1f   (%d rays picked)   %s the kernel-1 frame's median + spread" % (label, mn, med, n_picked, verdict))
        lines.append("  frame, VOLYM_OPT_KERNEL = 1 %9.1f / %9.1f   (spread: median - minimum = %.1f)" % (k1[0], k1[1], spread))
        lines.append("  frame, default kernel       %9.1f / %9.1f   (for scale)" % (dflt[0], dflt[1]))
    if "one pixel" in extra:
        lines += ["", "volym_pick of one pixel (blocking call, wall clock): median of 200 %.1f us, minimum %.1f us" % extra["one pixel"],
                  "frame loop, standing view at 1920x1080, volym_throttle(3): %.1f us per frame; with a whole-frame pick pass behind every frame: %.1f us" % (
                      extra["loop"], extra["loop with pick"])]
    lines.append("")
    lines.append("every pick pass within its bar" if ok else "a pick pass exceeds its bar: see DESIGN.md 4.6")
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
