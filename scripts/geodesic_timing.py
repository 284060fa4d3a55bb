"""What the geodesic pass and the flood cost (volym_geodesic_pass, volym_flood_labels), on seeded synthetic bonsai
volumes with their label maps on the device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.

  the pass     from the trunk (label 3) through the unlabelled matter, unlimited and with r = 8; from every label; a wand from one
               texel of the canopy through the canopy's matter within 40 bytes of that texel's.  The pass blocks, so a host clock
               around the call is its cost as a caller sees it; HIP events on the stream on either side give the device's share.
               --reps passes per block after 2 warm-ups, --blocks blocks per case: minimum over all passes, median of the block
               medians, their range (spread).  With the development build (make DEV=1, VOLYM_HIP_LIB) the rounds enqueued and the
               tiles relaxed in all are printed beside them.
  the batch    the first case again with VOLYM_GEODESIC_BATCH = 1, 2, 4, 8, 16 and 32 rounds between two reads of the count.
  the flood    after the unlimited pass from the trunk: a host clock around volym_flood_labels, ending in volym_sync, --edit-reps
               times; between two floods a relabel sends the texels back (not timed).
  for scale    on the same seeds: the nearest pass and the fill (the Euclidean sibling), and the components pass of the medium's
               predicate, HIP events as above.
  the host     once, at sizes up to --host-up-to: volym_read_labels, scipy.ndimage.binary_propagation from the seeds through the
               medium where scipy is installed, else the NumPy twin, np.where, volym_set_labels and the segment table again.
  the kernels  --kernel-stats FILE... appends each kernel's share of the kernel time from kernel-statistics CSVs of profiler runs of
               this script (columns Name, TotalDurationNs): all cases together.

    python scripts/geodesic_timing.py [--sizes 256,1024] [--reps 5] [--blocks 3] [--edit-reps 5] [--out profiles/geodesic.txt] [--kernel-stats FILE...]
"""
import argparse
import csv
import ctypes as C
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

KERNELS = ("zero", "init", "relax", "finish", "pack")


def kernel_shares(path):
    """lines: the share of every geodesic kernel in the summed kernel time of a profiler's kernel-statistics CSV"""
    total = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"volym_geodesic_([a-z_]+?)_kernel", row.get("Name", ""))
            if m:
                total[m.group(1)] = total.get(m.group(1), 0.0) + float(row["TotalDurationNs"])
    whole = sum(total.get(k, 0.0) for k in KERNELS) or 1.0
    return ["each kernel's share of the kernel time of the geodesic passes above (%s):" % os.path.basename(path)] + \
           ["    %-8s %5.1f %%" % (k, 100.0 * total.get(k, 0.0) / whole) for k in KERNELS]


def _ms(values):
    return "%9.3f (%.3f .. %.3f)" % (float(np.median(values)), float(np.min(values)), float(np.max(values)))


def _counts(ctx):
    """(rounds, tiles relaxed) of the latest pass, or None without the development build"""
    call = getattr(_lib.lib(), "volym_dev_geodesic_counts", None)
    if call is None:
        return None
    out = (C.c_ulonglong * 2)()
    call.argtypes, call.restype = [C.c_void_p, C.POINTER(C.c_ulonglong)], C.c_int
    return (int(out[0]), int(out[1])) if call(ctx.handle, out) == 0 else None


def _blocking(ctx, stream, fn, reps, warm=2):
    """(host microseconds, device microseconds) of each of `reps` blocking calls: a host clock round the call, a HIP event either side"""
    for _ in range(warm):
        fn()
    stream.synchronize()
    host, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e6)
        e1.record(stream)
        stream.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3)
    return np.array(host), np.array(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--edit-reps", type=int, default=5)
    ap.add_argument("--host-up-to", type=int, default=256, help="largest size at which the host route is timed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    a = ap.parse_args()
    lines = ["geodesic pass, microseconds, a host clock round each of %d blocking passes per block (host) and HIP events either side of it (device), %d blocks per case;" % (
        a.reps, a.blocks), "min = minimum over all passes, median = median of the block medians, spread = range of the block medians", ""]
    stream = torch.cuda.Stream()
    for n in (int(v) for v in a.sizes.split(",") if v):
        dims = (n, n, n)
        raw, labels = synth.synth_bonsai(n, with_labels=True)
        vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
        del raw, labels
        whole = ((0, 0, 0), dims)
        T = scene.smooth_table
        table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}])
        at = np.flatnonzero(lab == 2)
        at = int(at[at.size // 2])                                  # one texel of the canopy
        click = (at % n, (at // n) % n, at // (n * n))
        byte = int(vol[at])
        with demo.GpuContext(640, 480, 0) as ctx:
            ctx.set_stream(stream.cuda_stream)         # the caller's stream: torch events time what goes on it
            ctx.set_volume(vol, dims, 0)
            ctx.set_transfer_function(scene.default_lut())
            ctx.set_labels(lab, dims)
            ctx.set_segment_importances(table)
            lines.append("%d^3, %s layout, labels 0, 2, 3, 4 (%s texels)" % (n, "bricked" if n ** 3 > (64 << 20) else "linear", "{:,}".format(n ** 3)))
            trunk = scene.Geodesic(whole, 0, (1, 255), T([3]), T([0]))
            cases = (("from the trunk through the unlabelled matter", trunk), ("from the trunk, r = 8", trunk.replace(max_steps=8)),
                     ("from every label through the unlabelled matter", scene.Geodesic(whole, 0, (1, 255), T(range(1, 256)), T([0]))),
                     ("a wand from %r of the canopy, byte %d +- 40" % (click, byte), scene.Geodesic(whole, 0, (max(byte - 40, 0), min(byte + 40, 255)), T([]), T([2]), 0, [click])))
            for case, g in cases:
                host, dev = [], []
                for _ in range(a.blocks):
                    h, d = _blocking(ctx, stream, lambda: ctx.geodesic_pass(g), a.reps)
                    host.append(h)
                    dev.append(d)
                s, counts = ctx.read_geodesic(), _counts(ctx)
                lines.append("  %s: %s seeds, %s medium, %s reached, at most %s steps%s" % (
                    case, "{:,}".format(int(s["n_seed"])), "{:,}".format(int(s["n_medium"])), "{:,}".format(int(s["n_reached"])),
                    "no" if not int(s["n_reached"]) else int(s["max_steps"]), "" if counts is None else "; %d rounds enqueued, %s tiles relaxed in all" % counts))
                lines += [_line("host", host), _line("device", dev)]
            # the batch
            lines.append("  rounds per batch (VOLYM_GEODESIC_BATCH), the first case, host microseconds:")
            for batch in (1, 2, 4, 8, 16, 32):
                os.environ["VOLYM_GEODESIC_BATCH"] = str(batch)
                host = [_blocking(ctx, stream, lambda: ctx.geodesic_pass(trunk), a.reps)[0] for _ in range(a.blocks)]
                counts = _counts(ctx)
                lines.append(_line("batch %d" % batch, host) + ("" if counts is None else "   %d rounds enqueued" % counts[0]))
            del os.environ["VOLYM_GEODESIC_BATCH"]
            # the flood
            ctx.geodesic_pass(trunk)
            flood = scene.Flood(whole, 0, (0, 255), T([0]), T([3]), {3: 7}, (1, 0xFFFFFFFF))
            back = scene.Relabel(whole, to={7: 0})
            changed = int(ctx.flood_labels(flood)["changed"])
            assert int(ctx.edit_labels(back)["changed"]) == changed
            ctx.sync()
            floods = []
            for _ in range(a.edit_reps):
                t0 = time.perf_counter()
                ctx.flood_labels(flood)
                ctx.sync()
                floods.append((time.perf_counter() - t0) * 1e3)
                ctx.edit_labels(back)
                ctx.sync()
            lines += ["  the flood: what the trunk reaches through the unlabelled matter becomes label 7, %s texels; milliseconds, median (min .. max)" % "{:,}".format(changed),
                      "    volym_flood_labels                         %s" % _ms(floods)]
            # for scale
            seeds = scene.Distance(whole, 0, 1, scene.surface_select([3]))
            medium = scene.Components(whole, 0, 1, scene.surface_select([0, 3]))
            ctx.nearest_pass(seeds)
            ctx.components_pass(medium)
            near = [_timed(stream, lambda: ctx.nearest_pass(seeds), a.reps) for _ in range(a.blocks)]
            comp = [_timed(stream, lambda: ctx.components_pass(medium), a.reps) for _ in range(a.blocks)]
            fill = scene.Fill(whole, 0, (1, 255), T([0]), T([3]), (1, 64))
            fills = []
            for _ in range(a.edit_reps):
                t0 = time.perf_counter()
                moved = int(ctx.fill_labels(fill)["changed"])
                ctx.sync()
                fills.append((time.perf_counter() - t0) * 1e3)
                ctx.set_labels(lab, dims)
                ctx.set_segment_importances(table)
                ctx.sync()
            lines += ["  for scale, the same seeds, device microseconds:", _line("nearest pass", near), _line("components pass", comp),
                      "    volym_fill_labels within 8 texels, %s texels, milliseconds %s" % ("{:,}".format(moved), _ms(fills))]
            if n <= a.host_up_to:
                t0 = time.perf_counter()
                now = ctx.read_labels()
                t1 = time.perf_counter()
                v3 = vol.reshape(n, n, n)
                try:
                    from scipy import ndimage
                    how = "scipy.ndimage.binary_propagation"
                    grown = ndimage.binary_propagation((now == 3) & (v3 >= 1), mask=(v3 >= 1) & ((now == 0) | (now == 3)))
                    new = np.where(grown & (now == 0), 7, now).astype(np.uint8)
                except ImportError:
                    how = "the NumPy twin (scipy is not installed)"
                    _, keys = scene.geodesic_volume(vol, dims, trunk, labels=now.ravel())
                    new = np.where((keys != np.uint32(_lib.GEODESIC_NONE)) & (now == 0), 7, now).astype(np.uint8)
                t2 = time.perf_counter()
                ctx.set_labels(new.ravel(), dims)
                ctx.set_segment_importances(table)
                ctx.sync()
                t3 = time.perf_counter()
                assert int((new != now).sum()) == changed, "the host route must move the texels the flood moves"
                lines.append("    the host route, once: volym_read_labels %.1f ms, %s %.1f ms, the re-upload %.1f ms: %.1f ms" % (
                    (t1 - t0) * 1e3, how, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        lines.append("")
        print("\n".join(lines[-40:]), flush=True)
    for path in a.kernel_stats:
        lines += kernel_shares(path) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
