"""Time the smoothing two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3), the pot hidden:
  device -- volym_smooth_labels: the vote kernel over the request's box, the swap of the records it left with the labels, the label
            statistics rescanned, importances rewritten inside the hull of the changed texels, lists reset; beside it the table-only
            volym_edit_labels over the same box, which loads every label chunk and shares everything after the kernel;
  host   -- the path the call replaces: volym_read_labels, the twin (scene.smooth_volume, in slabs of 16 slices with their halo),
            then volym_set_labels, volym_set_segment_importances and volym_set_segment_visibility.
Passes: joint at radius 1 and at radius 3 over the whole volume; the canopy (label 2) against label 0 at radius 1; joint at radius 1
inside a slab of 64 slices about the volume's middle.  A pass is not its own inverse, so every repetition starts from the labels of
the start, handed to the context again outside the clock.  A figure is a host clock around the call, ending in volym_sync; one warm-up,
then --reps repetitions (device), or --host-reps repetitions without one (host, the slab alone: the twin over the whole volume is 16
times that): median, minimum and maximum (--host-reps 0 leaves the host path out, for a run under `rocprofv3 --kernel-trace --stats`,
which gives the vote kernel's own time).

    python scripts/smooth_timing.py [--size 1024] [--reps 9] [--host-reps 1] [--out profiles/smooth.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from volym_amd import _lib, demo, scene, synth  # noqa: E402

W, H = 1920, 1080


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _say(text):
    print(text, flush=True)


def _host_pass(vol, dims, smooth, labels, step=16):
    """the twin over the request's box in slabs of `step` slices, each with the halo its neighbourhoods reach into; labels [z, y, x]"""
    nx, ny, nz = dims
    (x0, y0, z0), (x1, y1, z1) = smooth.box
    rz = smooth.radius[2]
    out = labels.copy()
    v = vol.reshape(nz, ny, nx)
    for a in range(z0, z1, step):
        b = min(a + step, z1)
        lo, hi = max(a - rz, 0), min(b + rz, nz)
        part = smooth.replace(box=((x0, y0, a - lo), (x1, y1, b - lo)))
        new, _ = scene.smooth_volume(v[lo:hi], (nx, ny, hi - lo), part, labels[lo:hi])
        out[a:b] = new[a - lo:b - lo]
    return out


def run(n, reps, host_reps, cache=None):
    dims = (n, n, n)
    path = os.path.join(cache, "bonsai_%d.npz" % n) if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        vol, lab = z["vol"], z["lab"]
    else:
        raw, labels = synth.synth_bonsai(n, with_labels=True)
        vol = scene.prepare_volume(raw, dims, True)
        lab = scene.prepare_volume(labels, dims, True)
        del raw, labels
        if path:
            np.savez(path, vol=vol, lab=lab)
    table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}, {"label_value": 9, "importance": 128}])
    hidden = scene.visibility_mask((4,))
    whole = ((0, 0, 0), dims)
    slab = ((0, 0, n // 2 - min(32, n // 2)), (n, n, n // 2 + min(32, n // 2)))
    pair = scene.smooth_table([0, 2])
    passes = [("joint, radius 1, whole volume", scene.Smooth(1, whole)), ("joint, radius 3, whole volume", scene.Smooth(3, whole)),
              ("label 2 against 0, radius 1, whole volume", scene.Smooth(1, whole, give=pair, take=pair)),
              ("joint, radius 1, slab of %d slices" % (slab[1][2] - slab[0][2]), scene.Smooth(1, slab))]
    rows = []
    with demo.GpuContext(W, H, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())

        def start_over():
            ctx.set_labels(lab, dims)
            ctx.set_segment_importances(table)
            ctx.set_segment_visibility(hidden)
            ctx.sync()

        start_over()
        _say("scene of %d^3 on the device" % n)
        floors = {}
        for name, s in passes:
            if s.box not in floors:
                there, back = scene.Relabel(s.box, to={2: 9}), scene.Relabel(s.box, to={9: 2})
                ctx.edit_labels(there)
                ctx.edit_labels(back)
                ctx.sync()
                ms = []
                for r in range(reps + reps % 2):                        # (an even number: the labels end as they began)
                    t0 = time.perf_counter()
                    ctx.edit_labels(there if r % 2 == 0 else back)
                    ctx.sync()
                    ms.append((time.perf_counter() - t0) * 1e3)
                floors[s.box] = _stats(ms[:reps])
            changed, ms = 0, []
            for r in range(reps + 1):                                   # (the first is the warm-up)
                start_over()
                t0 = time.perf_counter()
                changed = int(ctx.smooth_labels(s)["changed"])
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            texels = int(np.prod([b - a for a, b in zip(*s.box)]))
            rows.append({"name": name, "changed": changed, "off": _stats(ms[1:]), "floor": floors[s.box], "texels": texels, "smooth": s})
            _say("%s: %d texels changed, device %.3f ms, table-only edit %.3f ms" % (name, changed, rows[-1]["off"][0], floors[s.box][0]))
        row = rows[-1]                                                  # the slab: the one the host path is run for
        host = []
        for r in range(max(host_reps, 0)):                              # (no warm-up: NumPy has none to give)
            start_over()
            t0 = time.perf_counter()
            now = ctx.read_labels()
            t1 = time.perf_counter()
            new = _host_pass(vol, dims, row["smooth"], now)
            t2 = time.perf_counter()
            ctx.set_labels(new.ravel(), dims)
            ctx.set_segment_importances(table)
            ctx.set_segment_visibility(hidden)
            ctx.sync()
            t3 = time.perf_counter()
            host.append((t3 - t0) * 1e3)
            row["host_parts"] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)
            assert int((new != now).sum()) == row["changed"], "the host path and the device must change the same texels"
        if host:
            row["host"] = _stats(host)
            _say("%s: host %.1f ms (read %.1f, twin %.1f, re-upload %.1f)" % ((row["name"], row["host"][0]) + row["host_parts"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--cache", default=None, help="a directory to keep the prepared scene in between runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(a.size, a.reps, a.host_reps, a.cache)
    lines = ["%d^3, labels on the device, the pot hidden; milliseconds per call, history off, median (min .. max) of %d" % (a.size, a.reps)]
    for row in rows:
        lines.append("%-44s %10d of %d texels changed" % (row["name"], row["changed"], row["texels"]))
        lines.append("    %-36s %9.3f (%.3f .. %.3f)" % (("the whole call",) + row["off"]))
        lines.append("    %-36s %9.3f (%.3f .. %.3f)   the call is %.1fx" % (("table-only edit, same box",) + row["floor"] + (row["off"][0] / row["floor"][0],)))
        lines.append("    %-36s %9.3f" % ("labels + density once at 8 TB/s", 2.0 * row["texels"] / 8e12 * 1e3))
        if "host" in row:
            lines.append("    %-36s %9.1f (%.1f .. %.1f)   %.0fx   read %.1f, twin %.1f, re-upload %.1f" %
                         (("host: read + twin + re-upload",) + row["host"] + (row["host"][0] / row["off"][0],) + row["host_parts"]))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
