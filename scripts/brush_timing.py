"""Time the brush two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3), the pot hidden:
  device -- volym_brush_labels: the brush kernel over the stroke's hull, the label statistics rescanned, importances rewritten
            inside the hull of the changed texels, lists reset; with the history off, with it on, and the undo of such a step;
  host   -- the path the call replaces: volym_read_labels of the stroke's box, the stroke's mask in NumPy (scene.brush_mask over
            that box), then volym_set_labels, volym_set_segment_importances and volym_set_segment_visibility.
Strokes, all inside the canopy (label 2 <-> 9, so that a stroke and the same stroke with the inverse table leave the labels as
they were): one ball of radius 8; 64 points 3 texels apart along a gently waving line, radius 4; 256 such points, radius 4.  The
points are synthetic -- no pick pass runs here; a pick record gives the same kind of triple.  A figure is a host clock around the
call, ending in volym_sync; one warm-up, then --reps (device) or --host-reps (host) repetitions: median, minimum and maximum
(--host-reps 0 leaves the host path out, for a run under `rocprofv3 --kernel-trace --stats`).

    python scripts/brush_timing.py [--size 1024] [--reps 9] [--host-reps 2] [--out profiles/brush.txt]
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


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _say(text):
    print(text, flush=True)


def _line(centre, n_points, dims, step=3):
    """n_points texels `step` apart along x through `centre`, waving a few texels in y and z, inside the volume"""
    k = np.arange(n_points) - n_points // 2
    x = centre[0] + step * k
    y = centre[1] + np.round(6 * np.sin(k / 5.0)).astype(np.int64)
    z = centre[2] + np.round(6 * np.cos(k / 7.0)).astype(np.int64)
    return [tuple(int(np.clip(v, 0, d - 1)) for v, d in zip(p, dims)) for p in zip(x, y, z)]


def run(n, reps, host_reps):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    del raw, labels
    table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}, {"label_value": 9, "importance": 128}])
    hidden = scene.visibility_mask((4,))
    coarse = np.argwhere(lab.reshape(n, n, n)[::8, ::8, ::8] == 2)                 # the canopy's middle, from every 8th texel
    centre = tuple(int(v) * 8 for v in np.median(coarse, axis=0)[::-1])
    strokes = [("one ball, radius 8", [centre], 64), ("64 points, radius 4", _line(centre, 64, dims), 16), ("256 points, radius 4", _line(centre, 256, dims), 16)]
    rows = []
    with demo.GpuContext(1920, 1080, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.set_segment_visibility(hidden)
        ctx.sync()
        _say("scene of %d^3 on the device, strokes around %r" % (n, centre))
        for name, points, r2 in strokes:
            there, back = scene.Brush(points, r2, to={2: 9}, dims=dims), scene.Brush(points, r2, to={9: 2}, dims=dims)
            box = scene.brush_box(there, dims)
            row = {"name": name, "box": box, "items": [scene.relabel_slab_items(dims, box, b) for b in (False, True)]}
            for history in (0, 256 << 20):
                ctx.label_history(history)
                changed = int(ctx.brush_labels(there)["changed"])
                ctx.brush_labels(back)                   # warm-up, and the state every repetition starts from
                ctx.sync()
                ms = []
                for r in range(reps):
                    t0 = time.perf_counter()
                    ctx.brush_labels(there if r % 2 == 0 else back)
                    ctx.sync()
                    ms.append((time.perf_counter() - t0) * 1e3)
                if reps % 2:
                    ctx.brush_labels(back)
                row["changed"] = changed
                row["on" if history else "off"] = _stats(ms)
            ms = []
            for r in range(reps):                        # (history on) a stroke, then its undo, timed alone
                ctx.brush_labels(there)
                ctx.sync()
                t0 = time.perf_counter()
                ctx.undo_labels()
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            row["undo"] = _stats(ms)
            row["records"] = ctx.label_history_info()["next_redo_records"]
            ctx.label_history(0)
            rows.append(row)
            _say("%s: %d texels, device %.3f ms (history on %.3f, undo %.3f)" % (name, row["changed"], row["off"][0], row["on"][0], row["undo"][0]))
        assert np.array_equal(ctx.read_labels().ravel(), lab), "the strokes and their inverses must leave the labels as they were"
        for row, (name, points, r2) in zip(rows, strokes):
            if host_reps <= 0:
                break
            lo, hi = row["box"]
            sub_dims = tuple(h - l for l, h in zip(lo, hi))
            moved = [tuple(p[a] - lo[a] for a in range(3)) for p in points]
            now = lab.copy()
            full = now.reshape(n, n, n)
            host = []
            for r in range(host_reps + 1):
                a, b = (2, 9) if r % 2 == 0 else (9, 2)
                t0 = time.perf_counter()
                sub = ctx.read_labels((lo, hi))
                mask = scene.brush_mask(scene.Brush(moved, r2, dims=sub_dims), sub_dims)
                full[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = np.where(mask & (sub == a), b, sub)
                ctx.set_labels(now, dims)
                ctx.set_segment_importances(table)
                ctx.set_segment_visibility(hidden)
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
            row["host"] = _stats(host[1:])
            if host_reps % 2 == 0:                       # (an odd number of strokes so far: back to the labels of the start)
                ctx.set_labels(lab, dims)
                ctx.set_segment_importances(table)
                ctx.set_segment_visibility(hidden)
            _say("%s: host %.1f ms" % (name, row["host"][0]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(a.size, a.reps, a.host_reps)
    lines = ["%d^3, labels on the device, the pot hidden; milliseconds per call, median (min .. max) of %d" % (a.size, a.reps)]
    for row in rows:
        lo, hi = row["box"]
        lines.append("%-22s %8d texels, box %s..%s, %d chunks journalled" % (row["name"], row["changed"], lo, hi, row["records"]))
        for key, what in (("off", "volym_brush_labels, history off"), ("on", "volym_brush_labels, history on"), ("undo", "volym_undo_labels of that step")):
            lines.append("    %-36s %9.3f (%.3f .. %.3f)" % ((what,) + row[key]))
        if "host" in row:
            lines.append("    %-36s %9.1f (%.1f .. %.1f)   %.0fx" % (("host: read box + mask + re-upload",) + row["host"] + (row["host"][0] / row["off"][0],)))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
