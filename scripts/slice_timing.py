"""What a slice pass costs (volym_slice_pass), on a seeded synthetic bonsai volume of --size^3 (default 1024) with its
label map on the device, in both device layouts (linear, 4x4x4 bricks): --pixels^2 (default 1024^2) slices normal to x, y and z
through the middle of the volume, one texel per pixel, and one oblique slice (normal (1, 2, 3)), in two dressings:

  DENSITY                 the density bytes alone: one byte gather per pixel
  TF | LABELS | MARK_CUT  transfer-function colours, the segments overlaid, the cut marked, under a crop box, an oblique clip plane
                          and a hidden segment: two byte gathers, two LDS reads and two blends per pixel

Method: after --warm untimed passes, --reps passes are enqueued between two HIP events on one stream, behind a long matrix product
so that the host has enqueued all of them before the device starts; the figure is the events' time / reps, in microseconds; the
best and the median of --runs such runs.  Twice: "standing", every pass the same slice (after the warm-up the lines it touches
are cache resident: a redraw with another palette or mode), and "scrubbing", every pass at another position 68 texels on (no
two consecutive passes share a 64-byte line or brick, and the layout that shares most -- linear, normal to x -- sees a line
again after 15 passes and a gigabyte of other lines: the lines come from HBM).  Beside each figure: the bytes the pass must touch at worst -- 64 per pixel and gather
(every pixel its own 64-byte sector or brick) plus the 4 it stores -- and the HBM rate the figure would imply if it did; a rate
far above the HBM's ~8 TB/s (or far below) says how much of that worst case the orientation really touches.

Against it, the only alternative the parent offers: scene.slice_frame, the NumPy twin, on the host copy of the same prepared arrays
(the arrays a caller may no longer hold), best of 3, in milliseconds.

    python scripts/slice_timing.py [--size 1024] [--pixels 1024] [--reps 200] [--runs 5] [--out profiles/slice.txt] [--host-only]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from volym_amd import _lib, scene, synth  # noqa: E402


def slices(n, px):
    """(name, slice) of the four orientations: one texel per pixel through the middle of an n^3 volume, px x px pixels"""
    dims = (n, n, n)
    out = []
    for axis in "xyz":
        s = scene.slice_axis(axis, n // 2, dims)
        # the same map centred on a px x px output (px > n: background round the volume)
        off = [-((px - n) // 2) * (s.du[a] + s.dv[a]) for a in range(3)]
        out.append(("normal to " + axis, s.replace(origin=tuple(o + d for o, d in zip(s.origin, off)), width=px, height=px)))
    out.append(("oblique (1, 2, 3)", scene.slice_through((n / 2.0,) * 3, (1, 2, 3), (0, 0, 1), (px, px), 1.0)))
    return out


def dressings(palette):
    full = _lib.SLICE_LABELS | _lib.SLICE_MARK_CUT
    return [("DENSITY", dict(mode=_lib.SLICE_DENSITY, flags=0), 1),
            ("TF | LABELS | MARK_CUT", dict(mode=_lib.SLICE_TF, flags=full, palette=palette, cut_rgba=(255, 0, 0, 96)), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-only", action="store_true", help="the NumPy twin's figures alone (no device)")
    a = ap.parse_args()
    if not a.host_only:
        import torch  # noqa: F401  (torch's HIP runtime first, as in bench.py)
    n, px = a.size, a.pixels
    dims = (n, n, n)
    raw, lab_raw = synth.synth_bonsai(n, with_labels=True)
    vol, labels = scene.prepare_volume(raw, dims, True), scene.prepare_volume(lab_raw, dims, True)
    del raw, lab_raw
    lut = scene.default_lut()
    palette = np.zeros((256, 4), np.uint8)
    palette[2], palette[3], palette[4] = (0, 255, 0, 96), (160, 82, 45, 96), (200, 200, 200, 96)
    lo, hi = (n // 8, 0, n // 16), (n - n // 8, n - n // 10, n)
    plane = scene.clip_plane_texels((1.0, 0.5, 1.0), (0.6, 0.6, 0.6), dims)
    cut = {"box": (lo, hi), "plane": plane, "visible": scene.visibility_mask([3])}
    geo = slices(n, px)
    lines = ["slice pass, %d^3 synthetic bonsai + labels, %d x %d pixels; device: microseconds per pass, best / median of %d runs of %d passes between two HIP events"
             % (n, px, px, a.runs, a.reps),
             "worst-case bytes: (64 per gather + 4 stored) per pixel; implied rate = worst-case bytes / best scrubbing time", ""]

    if not a.host_only:
        import torch
        from volym_amd import demo
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            m = torch.ones((8192, 8192), dtype=torch.float32, device="cuda")
            for layout, lname in ((0, "linear"), (1, "bricked")):
                with demo.GpuContext(64, 64, 0) as ctx:
                    ctx.set_stream(stream.cuda_stream)
                    ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
                    ctx.set_volume(vol, dims, 0)
                    ctx.set_transfer_function(lut)
                    ctx.set_labels(labels, dims)
                    for dname, kw, gathers in dressings(palette):
                        if gathers == 2:                        # the cut state of the second dressing
                            ctx.set_crop_box(lo, hi)
                            ctx.set_clip_plane(*plane)
                            ctx.set_segment_visibility(cut["visible"])
                        for gname, s in geo:
                            s = s.replace(**kw)
                            ctx.slice_pass(s)                   # grows the target: the one blocking path
                            us = []
                            for _ in range(a.runs):
                                for _ in range(a.warm):
                                    ctx.slice_pass(s)
                                stream.synchronize()
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                torch.mm(m, m)                  # the plug: the device is busy while the host enqueues
                                e0.record(stream)
                                for _ in range(a.reps):
                                    ctx.slice_pass(s)
                                e1.record(stream)
                                stream.synchronize()
                                us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
                            # the same, every pass at another position 68 texels on (along the normal; the oblique one along z), modulo n
                            cs = []
                            for k in range(a.reps):
                                shift = ((k * 68) % n - n // 2) * 65536
                                org = list(s.origin)
                                if gname.startswith("normal"):
                                    org["xyz".index(gname[-1])] = ((k * 68) % n) * 65536 + 0x8000
                                else:
                                    org[2] += shift
                                cs.append(s.replace(origin=tuple(org)).to_c())
                            cold = []
                            for _ in range(a.runs):
                                for c in cs[:a.warm]:
                                    ctx._ck(_lib.lib().volym_slice_pass(ctx.handle, c, None))
                                stream.synchronize()
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                torch.mm(m, m)
                                e0.record(stream)
                                for c in cs:
                                    ctx._ck(_lib.lib().volym_slice_pass(ctx.handle, c, None))
                                e1.record(stream)
                                stream.synchronize()
                                cold.append(e0.elapsed_time(e1) * 1e3 / a.reps)
                            worst = px * px * (64 * gathers + 4)
                            best, med = float(np.min(us)), float(np.median(us))
                            cbest, cmed = float(np.min(cold)), float(np.median(cold))
                            lines.append("%-8s %-24s %-18s standing %7.2f / %7.2f us   scrubbing %7.2f / %7.2f us   worst case %6.1f MB -> %6.0f GB/s scrubbing" % (
                                lname, dname, gname, best, med, cbest, cmed, worst / 1e6, worst / (cbest * 1e-6) / 1e9))
                            print(lines[-1], flush=True)
        lines.append("")

    # the host twin on the same prepared arrays
    now = scene.cut_volume(vol, dims, cut, labels)
    for dname, kw, gathers in dressings(palette):
        for gname, s in geo:
            s = s.replace(**kw)
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                if gathers == 2:
                    scene.slice_frame(now, dims, s, lut=lut, labels=labels, cut=cut, uncut=vol)
                else:
                    scene.slice_frame(vol, dims, s)
                ms.append((time.perf_counter() - t0) * 1e3)
            lines.append("host twin (NumPy) %-24s %-18s %8.1f ms (best of 3)" % (dname, gname, min(ms)))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
