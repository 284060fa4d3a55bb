"""What a measure pass costs (volym_measure_pass), on seeded synthetic bonsai volumes with their label maps on the
device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.

  the pass     the whole volume, a box of one eighth (the middle half of every axis) and the whole volume under a crop box that
               keeps that eighth; every label in one histogram group, and the labels spread over eight.  HIP events around each of
               --reps (>= 50) passes (the init kernel and the pass) after 5 warm-ups, inputs resident; --blocks (3) blocks per case;
               minimum over all passes, median of the block medians, and their range (spread).
  for scale    in the same session, on the same volume: volym_set_segment_importances, the segment map that moves the same two bytes
               per texel (host clock around the call, which ends in a stream synchronisation; median of 5, as
               scripts/segment_edit_timing.py takes it), and NumPy on host copies -- np.bincount over label * 256 + density, the path
               a caller without the pass would take (the download of the two volumes not counted).

    python scripts/measure_timing.py [--sizes 256,1024] [--reps 50] [--blocks 3] [--out profiles/measure.txt]
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


def _host_bincount(vol, lab, n):
    """seconds of the host path: counts per (label, byte) over the whole volume, a slab of z at a time (the keys of 1024^3 are 8 GiB)"""
    t0 = time.perf_counter()
    table = np.zeros(65536, np.int64)
    slab = max(1, (1 << 26) // (n * n))
    for z in range(0, n, slab):
        sl = slice(z * n * n, min(n, z + slab) * n * n)
        table += np.bincount(lab[sl].astype(np.int64) * 256 + vol[sl], minlength=65536)
    return time.perf_counter() - t0, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["measure pass (init kernel + pass), microseconds, HIP events around each of %d passes per block, %d blocks per case;" % (a.reps, a.blocks),
             "min = minimum over all passes, median = median of the block medians, spread = range of the block medians", ""]
    stream = torch.cuda.Stream()
    one, eight = np.zeros(256, np.int64), np.arange(256, dtype=np.int64) % 8
    for n in (int(v) for v in a.sizes.split(",")):
        dims = (n, n, n)
        raw, labels = synth.synth_bonsai(n, with_labels=True)
        vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
        del raw, labels
        q = n // 4
        eighth = ((q, q, q), (n - q, n - q, n - q))
        with demo.GpuContext(640, 480, 0) as ctx:
            ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
            ctx.set_volume(vol, dims, 0)
            ctx.set_labels(lab, dims)
            lines.append("%d^3, %s layout, labels 0, 2, 3, 4 (%s texels)" % (n, "bricked" if n ** 3 > (64 << 20) else "linear", "{:,}".format(n ** 3)))
            results = {}
            for case, box, crop in (("whole volume", None, None), ("box of one eighth", eighth, None), ("whole under a crop of one eighth", None, eighth)):
                if crop is not None:
                    ctx.set_crop_box(*crop)
                for gname, group in (("1 group", one), ("8 groups", eight)):
                    m = scene.Measure(box, 0, group, dims=dims)
                    blocks = [_timed(stream, lambda: ctx.measure_pass(m), a.reps) for _ in range(a.blocks)]
                    med = [float(np.median(b)) for b in blocks]
                    lines.append("  %-32s %-8s  min %9.1f   median %9.1f   spread %6.1f" % (case, gname, float(min(b.min() for b in blocks)), float(np.median(med)), max(med) - min(med)))
                    results[(case, gname)] = ctx.read_measure()
                if crop is not None:
                    ctx.set_crop_box((0, 0, 0), dims)
            rec, hist = results[("whole volume", "1 group")]
            tables = [scene.segment_table([{"label_value": 2, "importance": 255}]), scene.segment_table([{"label_value": 3, "importance": 255}])]
            ms = []
            for r in range(6):
                t0 = time.perf_counter()
                ctx.set_segment_importances(tables[r % 2])
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            lines.append("  segment map (volym_set_segment_importances, host clock, median of 5 after the first): %.3f ms" % float(np.median(ms[1:])))
        secs, table = _host_bincount(vol, lab, n)
        table = table.reshape(256, 256)
        same = table.sum(axis=1).tolist() == rec["count"].tolist() and table.sum(axis=0).tolist() == hist[0].tolist()
        lines.append("  NumPy bincount over label * 256 + density on host copies: %.1f ms; counts and histogram %s the pass's" % (secs * 1e3, "equal" if same else "DIFFER FROM"))
        lines.append("")
        print("\n".join(lines[-10:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
