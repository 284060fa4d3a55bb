"""Time the lasso two ways, on a seeded synthetic bonsai volume with its label map on the device (default 1024^3), the pot hidden,
in the benchmark camera's view of a 1920 x 1080 frame:
  device -- volym_lasso_labels: the raster kernel over the polygon's rect, the edit kernel over the request's box (the whole volume),
            the label statistics rescanned, importances rewritten inside the hull of the changed texels, lists reset; beside it the
            table-only volym_edit_labels over the whole volume, which loads every label chunk and shares that transition;
  host   -- the path the call replaces: volym_read_labels, the twin's projection in NumPy (scene.lasso_texels and scene.lasso_mask,
            in slabs of 32 slices), then volym_set_labels, volym_set_segment_importances and volym_set_segment_visibility.
Lassos, all on the canopy (label 2 <-> 9, so that a lasso and the same lasso with the inverse table leave the labels as they were):
a rectangle over the middle quarter of the frame through the whole depth; a wavy closed curve of 1024 vertices; the same with OUTSIDE;
the same confined to a slab of 16 texels about the volume's middle by `depth`.  A figure is a host clock around the call, ending in
volym_sync; one warm-up, then --reps repetitions (device), or --host-reps repetitions without one (host, the first two lassos): median, minimum and maximum (--host-reps 0 leaves
the host path out, for a run under `rocprofv3 --kernel-trace --stats`, which gives the two kernels' own times).

    python scripts/lasso_timing.py [--size 1024] [--reps 9] [--host-reps 1] [--out profiles/lasso.txt]
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


def _curve(n=1024, r=330.0):
    """a closed wavy curve of n vertices about the middle of the frame"""
    a = 2.0 * np.pi * np.arange(n) / n
    rr = r * (1.0 + 0.15 * np.sin(7 * a) + 0.05 * np.cos(23 * a))
    return [(int(round(W / 2 + 1.3 * q * np.cos(t))), int(round(H / 2 + q * np.sin(t)))) for q, t in zip(rr, a)]


def _host_selected(lasso, dims, z0, z1):
    """the twin's selection of slices [z0, z1): the view moved by z0 slices, which the rule allows (c' = c + 2 z0 m[.][2])"""
    v = lasso.view
    moved = v.replace(c=tuple(v.c[r] + 2 * z0 * v.m[r][2] for r in range(3)))
    lands, px, py = scene.lasso_texels(moved, (dims[0], dims[1], z1 - z0))
    inside = lands & lasso._mask[py, px]
    return inside != bool(lasso.flags & _lib.LASSO_OUTSIDE)


def run(n, reps, host_reps):
    dims = (n, n, n)
    raw, labels = synth.synth_bonsai(n, with_labels=True)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    del raw, labels
    table = scene.segment_table([{"label_value": 2, "importance": 255}, {"label_value": 3, "importance": 0}, {"label_value": 9, "importance": 128}])
    hidden = scene.visibility_mask((4,))
    state = scene.State.with_parameters(W / H, scene.StateParameters.benchmark())
    state.update()
    view = scene.lasso_view(state.camera_uniforms(), W, H, dims)
    mid = (view.m[2][0] + view.m[2][1] + view.m[2][2]) * n + view.c[2]       # D at the volume's middle
    slab = view.replace(depth=(mid - 8 * 2 ** view.scale_log2 // n, mid + 8 * 2 ** view.scale_log2 // n))
    quarter = [(W // 4, H // 4), (3 * W // 4, H // 4), (3 * W // 4, 3 * H // 4), (W // 4, 3 * H // 4)]
    curve = _curve()
    lassos = [("quarter-frame rectangle", quarter, view, 0), ("1024-vertex lasso", curve, view, 0), ("1024-vertex lasso, OUTSIDE", curve, view, _lib.LASSO_OUTSIDE),
              ("1024-vertex lasso, 16-texel slab", curve, slab, 0)]
    rows = []
    with demo.GpuContext(W, H, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(scene.default_lut())
        ctx.set_labels(lab, dims)
        ctx.set_segment_importances(table)
        ctx.set_segment_visibility(hidden)
        ctx.sync()
        _say("scene of %d^3 on the device, view scaled by 2^%d" % (n, view.scale_log2))

        def timed(there, back, call):
            changed = int(call(there)["changed"])
            call(back)                                   # warm-up, and the state every repetition starts from
            ctx.sync()
            ms = []
            for r in range(reps):
                t0 = time.perf_counter()
                call(there if r % 2 == 0 else back)
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            if reps % 2:
                call(back)
            return changed, _stats(ms)

        changed, ms = timed(scene.Relabel(dims=dims, to={2: 9}), scene.Relabel(dims=dims, to={9: 2}), ctx.edit_labels)
        rows.append({"name": "table-only volym_edit_labels, whole volume", "changed": changed, "off": ms})
        _say("table-only edit: %d texels, %.3f ms" % (changed, ms[0]))
        for name, points, v, flags in lassos:
            there, back = (scene.Lasso(points, v, flags=flags, to=t, dims=dims) for t in ({2: 9}, {9: 2}))
            changed, ms = timed(there, back, ctx.lasso_labels)
            rows.append({"name": name, "changed": changed, "off": ms, "rect": scene.lasso_rect(there), "lasso": there})
            _say("%s: %d texels, device %.3f ms" % (name, changed, ms[0]))
        assert np.array_equal(ctx.read_labels().ravel(), lab), "the lassos and their inverses must leave the labels as they were"
        for row in rows[1:3]:                            # (the rectangle and the lasso: the other two cost the host the same)
            if host_reps <= 0:
                break
            l = row["lasso"]
            l._mask = scene.lasso_mask(l.points, W, H)
            host = []
            for r in range(host_reps):                   # (no warm-up: NumPy has none to give, and a repetition takes a minute)
                a, b = (2, 9) if r % 2 == 0 else (9, 2)
                t0 = time.perf_counter()
                now = ctx.read_labels()
                for z0 in range(0, n, 32):
                    z1 = min(z0 + 32, n)
                    part = now[z0:z1]
                    part[_host_selected(l, dims, z0, z1) & (part == a)] = b
                ctx.set_labels(now.ravel(), dims)
                ctx.set_segment_importances(table)
                ctx.set_segment_visibility(hidden)
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
            row["host"] = _stats(host)
            if host_reps % 2 == 1:                       # (an odd number of lassos so far: back to the labels of the start)
                ctx.set_labels(lab, dims)
                ctx.set_segment_importances(table)
                ctx.set_segment_visibility(hidden)
            _say("%s: host %.1f ms" % (row["name"], row["host"][0]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(a.size, a.reps, a.host_reps)
    lines = ["%d^3, labels on the device, the pot hidden, %d x %d; milliseconds per call, history off, median (min .. max) of %d" % (a.size, W, H, a.reps)]
    for row in rows:
        lines.append("%-44s %10d texels%s" % (row["name"], row["changed"], ", mask rect %r" % (row["rect"],) if "rect" in row else ""))
        lines.append("    %-36s %9.3f (%.3f .. %.3f)" % (("the whole call",) + row["off"]))
        if "host" in row:
            lines.append("    %-36s %9.1f (%.1f .. %.1f)   %.0fx" % (("host: read + project + re-upload",) + row["host"] + (row["host"][0] / row["off"][0],)))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
