"""`python -m volym_amd [run simple | benchmark] [-d]` -- the headless counterpart of the reference's CLI
(`cargo run`, `cargo run -- benchmark`; src/cli.rs:4-56, src/main.rs:42-49).

benchmark: the reference's sweep (src/main.rs:178-345) -- 4 step sizes x {Base, Importance x {10,15,20},
ImportanceCone x {10,15,20}} = 28 rows, 3 trials each, 1024x768, benchmark parameters -- written to
benchmark_results.csv with the reference's columns (src/main.rs:71-85) followed by Mrays/s, algorithmic
bytes/GB/s and the roofline fraction.  Unlike the reference (presented frames over 2 s of wall clock, with
blit, GUI and possibly vsync inside), a trial here is `--secs` of back-to-back compute passes timed with
HIP events.  The reference's teapot .raw files are not distributed (.MISSING_LARGE_BLOBS); pass
--volume/--labels/--segments for real data, otherwise the synthetic stand-in of volym_amd.synth is used.

run simple: renders the interactive default view (src/state.rs:41-55) once and writes screenshot_<unix time>.png
like the reference's `P` key (src/state.rs:85-113).  --pick X,Y[,ALPHA] then prints what that pixel shows (segment, texel,
depth) as one JSON line.  --outline NAME[,NAME...] (segment names, ids or label values) and --outline-at X,Y (the segment under that
pixel) write the annotated image instead: a ring round the segments and a tint over them (demo.Simple.highlight).
--slice AXIS,INDEX writes the slice view beside the frame -- the plane normal to x, y or z through texel INDEX, transfer-function
colours, segments overlaid, cut texels tinted (demo.Simple.slice) -- as <screenshot>_slice_<axis>.png; --slice-at X,Y the three
orthogonal slices through the texel pixel (X, Y) shows.  --project MAX|MEAN[,STEP] writes the projection view -- maximum or mean
intensity along the rays of the same view, STEP apart (default: a quarter of the march step) -- as <screenshot>_project_<mode>.png
(demo.Simple.project).  --surface [NAME,...][:MIN_BYTE] prints the surface table of the scene in view -- faces per axis, area, enclosed
texels beside the measured count and sphericity per segment (demo.Simple.surface) -- and --surface-out FILE.stl|.obj writes the mesh of
those segments together (demo.Simple.export_surface).  --components [NAME,...][:MIN_BYTE] prints, per segment in view, its connected
pieces -- how many, the largest, and the ten largest with root and box (demo.Simple.components).  --distance [NAME,...][:MIN_BYTE]
prints the distance map's summary for the union of those segments (default: every label) -- solid texels, the deepest point and, per
segment, its nearest texel and the clearance -- and writes the histogram as <screenshot>_distance.json; --distance-inside measures
inside the set instead: thickness (demo.Simple.distance).  --measure [NAME,...] prints the table of segment statistics of the scene in view -- texels, share in view,
mean, deviation, range, centroid and box per segment (demo.Simple.measure) -- and writes the density histogram of the visible scene
and of each listed segment as <screenshot>_histogram.json (demo.Simple.histogram).
--relabel FROM[,FROM...]:TO, --brush X,Y,Z[/X,Y,Z...]:TO:R2, --brush-at X,Y[/X,Y...]:NAME:R, --lasso X,Y/X,Y/X,Y[/...]:FROM[,FROM...]:TO (--lasso-outside), --smooth [NAME,...][:R[,R,R]] (--smooth-iterations N), --split-at X,Y:TO, --keep-largest NAME, --grow NAME:R, --shrink NAME:R, --fill [NAME,...][:R], --separate NAME:R, --flood [NAME,...][:R], --wand-at X,Y:NAME:TOL[:R], --grow-from-seeds NAME[,NAME...][:CONTRAST[:MAX_COST]] and --smart-wand-at X,Y:NAME:CONTRAST:MAX_COST edit the labels on the device
after the first frame, in that order (demo.Simple.relabel, GpuContext.brush_labels, Simple.stroke, lasso, smooth, split_at, keep_largest, grow, shrink, fill, separate, grow_through, wand_at, grow_from_seeds, smart_wand_at, fill_between); the PNG is the frame after them and
each prints its result as one JSON line.  --labels-out FILE writes the labels as they then stand, raw bytes in the orientation of
--labels (demo.Simple.save_labels).  --undo N keeps a history of those edits on the device (demo.Simple.history) and takes the last N
back before the picture and --labels-out, one JSON line {"undo": ...} each.
"""
import argparse
import csv
import math
import sys
import time

import numpy as np

from . import _lib, demo, image, scene, synth

STEP_SIZES = [0.0030, 0.0050, 0.0100, 0.0200]   # src/main.rs:192
IMPORTANCE_STEPS = [10, 15, 20]                  # src/main.rs:193
NUM_TRIALS = 3                                   # src/main.rs:179
CSV_COLUMNS = ["algorithm", "step_size", "importance_steps", "use_cone", "avg_total_frames", "avg_total_time_ms",
               "avg_frame_time_ms", "avg_fps", "std_dev_total_frames", "std_dev_total_time_ms", "std_dev_frame_time_ms",
               "std_dev_fps"]                    # src/main.rs:71-85
EXTRA_COLUMNS = ["mrays_per_s", "b_alg_bytes_per_frame", "algorithmic_gb_per_s", "hbm_roofline_fraction", "n_gpus"]


def sweep_rows():
    """(algorithm, step_size, importance_steps, use_cone) in the reference's order (src/main.rs:197-335)."""
    rows = [("Base", s, 0, False) for s in STEP_SIZES]
    rows += [("Importance", s, n, False) for s in STEP_SIZES for n in IMPORTANCE_STEPS]
    rows += [("ImportanceCone", s, n, True) for s in STEP_SIZES for n in IMPORTANCE_STEPS]
    return rows


def _load_assets(args):
    if args.volume:
        raw = np.fromfile(args.volume, np.uint8)
        labels = np.fromfile(args.labels, np.uint8) if args.labels else np.zeros(0, np.uint8)
        segments = scene.load_segments(args.segments) if args.segments else []
        return raw, labels, segments, "file:" + args.volume
    raw, labels = synth.synth_teapot()
    return raw, labels, synth.TEAPOT_SEGMENTS, "synthetic teapot 256x256x178 (volym_amd.synth)"


def _stats(values):
    m = float(np.mean(values))
    return m, float(np.sqrt(np.mean((np.asarray(values, np.float64) - m) ** 2)))   # population std, src/main.rs:124-158


def benchmark(args):
    W, H = args.width, args.height
    raw, labels, segments, what = _load_assets(args)
    print("volym benchmark: %s, %dx%d, %d rows x %d trials of %.2f s" % (what, W, H, len(sweep_rows()), NUM_TRIALS, args.secs))
    base = scene.StateParameters.benchmark()                        # src/main.rs:180-190
    out_rows = []
    flight = getattr(args, "frames_in_flight", 1)
    with demo.GpuContext(W, H, args.device) as ctx:
        if flight == 2:                                             # before the scene (include/volym_hip.h VOLYM_OPT_FRAMES_IN_FLIGHT)
            ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 2)
        state = scene.State.with_parameters(W / H, base)
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels, segments=segments, dims=(256, 256, 256))

        def trial(n):
            """total milliseconds of n frames: per-launch HIP events on one stream, or -- two frames in flight -- the wall clock of
            n compute passes enqueued back to back (as the reference counts presented frames over wall time, src/main.rs:113-135)"""
            if flight != 2:
                return float(ctx.time_passes(n).sum())
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                ctx.compute_pass()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3

        for (algo, step, isteps, cone) in sweep_rows():
            p = base.replace(raymarching_step_size=step)
            if algo != "Base":
                p = p.replace(use_importance_rendering=1, importance_check_ahead_steps=isteps, use_cone_importance_check=1 if cone else 0)
            state = scene.State.with_parameters(W / H, p)
            state.update()                                          # src/event_loop.rs:100
            d.update_gpu_state(ctx, state)
            ms = ctx.time_passes(8)                                 # warm-up; also sizes the trial
            ctx.settle()                                            # the work list dealt from the warm-up frames is in place
            per = max(float(np.median(ms)), 1e-3)
            n = int(min(max(args.secs * 1e3 / per, 4), 20000))
            frames, times, ftimes, fps = [], [], [], []
            if flight == 2:
                trial(8)                                            # both frame contexts warm, their lists in place
                ctx.settle()
            for _ in range(NUM_TRIALS):
                total = trial(n)
                frames.append(n); times.append(total); ftimes.append(total / n); fps.append(n / (total * 1e-3))
            st = ctx.stats_pass()
            b_alg = st["n_vol"] + st["n_imp"] + 4 * W * H
            ft = float(np.mean(ftimes))
            row = [algo, step, isteps, str(cone).lower()]
            for v in (frames, times, ftimes, fps):
                row.append(_stats(v)[0])
            for v in (frames, times, ftimes, fps):
                row.append(_stats(v)[1])
            row += [W * H / (ft * 1e-3) / 1e6, b_alg, b_alg / (ft * 1e-3) / 1e9, b_alg / (ft * 1e-3) / 8.0e12, 1]
            out_rows.append(row)
            print("%-14s step %.4f steps %2d: %8.3f ms/frame %9.1f fps %9.0f Mrays/s  B_alg %6.1f MB  %5.1f%% of HBM roofline" % (
                algo, step, isteps, ft, _stats(fps)[0], row[12], b_alg / 1e6, 100 * row[15]), flush=True)
    with open(args.output, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS + EXTRA_COLUMNS)
        w.writerows(out_rows)
    print("wrote", args.output)
    return 0


def _crop_arg(text):
    """--crop x0,y0,z0,x1,y1,z1 (unit-cube coordinates) -> (lo01, hi01)"""
    v = [float(t) for t in text.split(",")]
    if len(v) != 6:
        raise SystemExit("--crop: x0,y0,z0,x1,y1,z1 in [0, 1]")
    return tuple(v[:3]), tuple(v[3:])


def _clip_plane_arg(text):
    """--clip-plane NX,NY,NZ,PX,PY,PZ (normal and a point of the plane, unit-cube coordinates) -> (normal, point)"""
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        v = []
    if len(v) != 6 or not all(math.isfinite(t) for t in v) or not any(v[:3]):
        raise SystemExit("--clip-plane: NX,NY,NZ,PX,PY,PZ -- a normal (not zero) and a point of the plane, unit-cube coordinates")
    return tuple(v[:3]), tuple(v[3:])


def _hide_arg(text):
    """--hide 3,4 (label values) -> [3, 4]"""
    try:
        v = [int(t) for t in text.split(",") if t.strip() != ""]
    except ValueError:
        raise SystemExit("--hide: label values 0..255, comma separated")
    if not v or any(not 0 <= l <= 255 for l in v):
        raise SystemExit("--hide: label values 0..255, comma separated")
    return v


def _pick_arg(text):
    """--pick X,Y[,ALPHA] (pixel of the frame, alpha_min) -> (x, y, alpha_min)"""
    try:
        v = text.split(",")
        x, y = int(v[0]), int(v[1])
        alpha = float(v[2]) if len(v) == 3 else 0.5
    except (ValueError, IndexError):
        raise SystemExit("--pick: X,Y[,ALPHA] -- a pixel of the frame and alpha_min in [0, 0.95] (default 0.5)")
    if len(v) > 3 or x < 0 or y < 0:
        raise SystemExit("--pick: X,Y[,ALPHA] -- a pixel of the frame and alpha_min in [0, 0.95] (default 0.5)")
    return x, y, alpha


def _outline_arg(text):
    """--outline Canopy,3 (names or ids of the segments JSON, or label values) -> ["Canopy", 3]"""
    v = [t.strip() for t in text.split(",") if t.strip() != ""]
    if not v:
        raise SystemExit("--outline: segment names, ids or label values, comma separated")
    return [int(t) if t.isdigit() else t for t in v]


def _outline_at_arg(text, flag="--outline-at"):
    """--outline-at X,Y, --clip-at X,Y (pixel of the frame) -> (x, y)"""
    try:
        x, y = (int(t) for t in text.split(","))
    except ValueError:
        raise SystemExit("%s: X,Y -- a pixel of the frame" % flag)
    if x < 0 or y < 0:
        raise SystemExit("%s: X,Y -- a pixel of the frame" % flag)
    return x, y


def _slice_arg(text):
    """--slice z,128 -> ("z", 128)"""
    v = [t.strip() for t in text.split(",")]
    if len(v) != 2 or v[0] not in ("x", "y", "z") or not v[1].isdigit():
        raise SystemExit("--slice: AXIS,INDEX -- x, y or z and a texel index along it")
    return v[0], int(v[1])


def _project_arg(text):
    """--project MAX,0.002 -> ("MAX", 0.002); --project mean -> ("MEAN", None)"""
    v = [t.strip() for t in text.split(",")]
    try:
        if len(v) not in (1, 2) or v[0].upper() not in ("MAX", "MEAN"):
            raise ValueError
        return v[0].upper(), (float(v[1]) if len(v) == 2 else None)
    except ValueError:
        raise SystemExit("--project: MAX or MEAN, then optionally the distance between samples")


def _slice_path(path, axis):
    stem = path[:-4] if path.lower().endswith(".png") else path
    return "%s_slice_%s.png" % (stem, axis)


def _measure_table(rows):
    """the table --measure prints: one line per segment of demo.Simple.measure's dict"""
    lines = ["%-16s %5s %12s %8s %8s %8s %4s %4s  %-22s %s" % ("segment", "label", "texels", "in view", "mean", "std", "min", "max", "centroid", "box")]
    for name, s in rows.items():
        if s is None:
            lines.append("%-16s %5s %12s" % (name, "", "-"))
            continue
        lines.append("%-16s %5d %12d %7.1f%% %8.2f %8.2f %4d %4d  (%6.1f,%6.1f,%6.1f) [%d,%d,%d]..[%d,%d,%d]" % (
            (name, s["label"], s["count"], 100.0 * s["in_view"], s["mean"], s["std"], s["min"], s["max"]) + s["centroid"] + s["box"][0] + s["box"][1]))
    return "\n".join(lines)


def _surface_arg(text, option="--surface"):
    """NAME[,NAME...][:MIN_BYTE] -> (names or label values, None for every segment in view; min_byte)"""
    names, _, m = text.rpartition(":") if ":" in text else (text, "", "")
    try:
        min_byte = int(m) if m else 1
    except ValueError:
        raise SystemExit("%s: NAME[,NAME...][:MIN_BYTE], MIN_BYTE an integer in 1..255" % option)
    return [int(v) if v.isdigit() else v for v in names.split(",") if v] or None, min_byte


def _surface_table(rows):
    """the table --surface prints: one line per segment of demo.Simple.surface's dict"""
    lines = ["%-16s %5s %10s %10s %10s %12s %12s %12s %10s" % ("segment", "label", "faces x", "faces y", "faces z", "area", "enclosed", "measured", "sphericity")]
    for name, s in rows.items():
        lines.append("%-16s %5d %10d %10d %10d %12.1f %12d %12d %10.3f" % ((name, s["label"]) + tuple(s["pairs"]) + (s["area"], s["enclosed"], s["measured"], s["sphericity"])))
    return "\n".join(lines)


def _components_table(rows):
    """what --components prints: per segment of demo.Simple.components' dict its pieces and largest piece, then its ten largest pieces"""
    lines = []
    for name, s in rows.items():
        big = s["largest"]
        lines.append("%-16s label %3d: %d piece%s in %d solid texels, largest %d texels (%.1f%%), %d smaller than 8 texels" % (
            name, s["label"], s["pieces"], "" if s["pieces"] == 1 else "s", s["solid"], big["count"] if big else 0, 100.0 * (s["share"] or 0.0), s["small"]["pieces"]))
        for p in s["top"]:
            lines.append("  piece %-8d %10d texels  root (%d,%d,%d)  box [%d,%d,%d]..[%d,%d,%d]%s" % (
                (p["number"], p["count"]) + p["root"] + p["box"][0] + p["box"][1] + (" open" if p["open"] else "",)))
    return "\n".join(lines) if lines else "components: no solid texel"


def _distance_table(s, inside):
    """what --distance prints: solid texels and the deepest point of demo.Simple.distance's dict, then the nearest texel of every segment"""
    if s["max_d2"] is None:
        lines = ["distance: %d solid texels%s, deepest (none): no texel at a finite distance" % (s["n_solid"], " (inside)" if inside else "")]
    else:
        lines = ["distance: %d solid texels%s, deepest (%d,%d,%d) d2 %d = %.3f, %d texels at a finite distance" % (
            (s["n_solid"], " (inside)" if inside else "") + s["max_at"] + (s["max_d2"], s["max"], s["n_finite"]))]
    for l, c in s["clearance"].items():
        lines.append("  nearest %-16s label %3d: d2 %10d = %9.3f at (%d,%d,%d)" % ((c["segment"], l, c["d2"], c["distance"]) + c["at"]))
    return "\n".join(lines)


def _segment_arg(text):
    """a segment on the command line: a label value or a name / id of the segments JSON"""
    return int(text) if text.isdigit() else text


def _name_and(text, option, what, number=float):
    """--grow NAME:R, --split-at X,Y:TO -> (left part, right part)"""
    left, sep, right = text.rpartition(":")
    if not sep or not left or not right:
        raise SystemExit("%s: %s" % (option, what))
    try:
        return left, (number(right) if number is not None else right)
    except ValueError:
        raise SystemExit("%s: %s" % (option, what))


def _brush_arg(d, ctx, text):
    """--brush X,Y,Z[/X,Y,Z...]:TO:R2 -> the scene.Brush that paints segment TO over every label along that polyline of texels"""
    usage = "X,Y,Z[/X,Y,Z...]:TO:R2 -- texels of the stroke, a label value or segment name, the squared radius"
    rest, r2 = _name_and(text, "--brush", usage, int)
    at, to = _name_and(rest, "--brush", usage, None)
    try:
        points = [tuple(int(v) for v in p.split(",")) for p in at.split("/")]
    except ValueError:
        raise SystemExit("--brush: %s" % usage)
    if not points or any(len(p) != 3 for p in points):
        raise SystemExit("--brush: %s" % usage)
    d._ready_to_edit(ctx)
    return scene.Brush(points, r2, to=d._brush_table(ctx, _segment_arg(to), None), dims=d.dims)


def _smooth_arg(text):
    """--smooth [NAME,...][:R[,R,R]] -> (names or None for a joint pass, radius)"""
    usage = "[NAME,...][:R[,R,R]] -- the segments to smooth against label 0 (none: every label, jointly) and the radius in texels, one or per axis (default 1)"
    names, sep, r = text.partition(":")
    try:
        radius = [int(v) for v in r.split(",")] if sep else [1]
    except ValueError:
        raise SystemExit("--smooth: %s" % usage)
    if len(radius) not in (1, 3) or (sep and not r):
        raise SystemExit("--smooth: %s" % usage)
    return ([_segment_arg(n) for n in names.split(",") if n] or None), (radius[0] if len(radius) == 1 else tuple(radius))


def _fill_arg(text):
    """--fill [NAME,...][:R] -> (names or None for every segment, r or None for no limit)"""
    usage = "[NAME,...][:R] -- the segments that grow into the unlabelled matter (none: every segment) and how far in texels (default: no limit)"
    names, sep, r = text.partition(":")
    try:
        limit = float(r) if sep else None
    except ValueError:
        raise SystemExit("--fill: %s" % usage)
    return ([_segment_arg(n) for n in names.split(",") if n] or None), limit


def _fill_table(d, result):
    """what --fill prints: how many texels joined the nearest segment, then every segment that took some"""
    took = sorted(result["arrived"].items())
    lines = ["fill: %d texels joined the nearest of %d segments" % (result["changed"], len(took))]
    for l, n in took:
        lines.append("  + %-16s label %3d: %10d" % (d._segment_name(l) or "label %d" % l, l, n))
    return "\n".join(lines)


def _flood_table(d, result):
    """what --flood prints: how many texels joined a segment through the matter, then every segment that took some"""
    took = sorted(result["arrived"].items())
    lines = ["flood: %d texels joined %d segments through the matter" % (result["changed"], len(took))]
    for l, n in took:
        lines.append("  + %-16s label %3d: %10d" % (d._segment_name(l) or "label %d" % l, l, n))
    return "\n".join(lines)


def _wand_arg(text):
    """--wand-at X,Y:NAME:TOL[:R] -> (x, y, name, tolerance, r or None)"""
    usage = "X,Y:NAME:TOL[:R] -- a pixel, the segment that takes what the wand reaches, the tolerance in density bytes and the reach in steps (default: no limit)"
    parts = text.split(":")
    try:
        x, y = (int(v) for v in parts[0].split(","))
        name, tol = parts[1], int(parts[2])
        r = int(parts[3]) if len(parts) > 3 else None
        if len(parts) > 4 or not name:
            raise ValueError
    except (ValueError, IndexError):
        raise SystemExit("--wand-at: %s" % usage)
    return x, y, name, tol, r


def _grow_arg(text):
    """--grow-from-seeds NAME[,NAME...][:CONTRAST[:MAX_COST]] -> (names, contrast, max_cost)"""
    usage = ("NAME[,NAME...][:CONTRAST[:MAX_COST]] -- the segments that grow, what a byte of density change across a step costs beside the step's own 1 "
             "(0..255, default 16) and the most a texel may cost (default: no limit)")
    parts = text.split(":")
    try:
        names = [_segment_arg(n) for n in parts[0].split(",") if n]
        contrast = int(parts[1]) if len(parts) > 1 else 16
        max_cost = int(parts[2]) if len(parts) > 2 else 0
        if len(parts) > 3 or not names or not 0 <= contrast <= 255 or max_cost < 0:
            raise ValueError
    except ValueError:
        raise SystemExit("--grow-from-seeds: %s" % usage)
    return names, contrast, max_cost


def _grow_table(d, result):
    """what --grow-from-seeds prints: how many texels joined the segment that reaches them most cheaply, then every segment that took some"""
    took = sorted(result["arrived"].items())
    lines = ["grow from seeds: %d texels joined the cheapest of %d segments" % (result["changed"], len(took))]
    for l, n in took:
        lines.append("  + %-16s label %3d: %10d" % (d._segment_name(l) or "label %d" % l, l, n))
    return "\n".join(lines)


def _fill_between_arg(text):
    """--fill-between NAME[,NAME...]:AXIS[:MAX_GAP] -> (names, axis, max_gap)"""
    usage = ("NAME[,NAME...]:AXIS[:MAX_GAP] -- the segments to interpolate, the axis their painted slices are perpendicular to (x, y or z) and the most "
             "slices a gap may have (default: no limit)")
    parts = text.split(":")
    try:
        names = [_segment_arg(n) for n in parts[0].split(",") if n]
        axis = parts[1] if len(parts) > 1 else ""
        max_gap = int(parts[2]) if len(parts) > 2 else 0
        if len(parts) > 3 or not names or axis not in ("x", "y", "z") or max_gap < 0:
            raise ValueError
    except ValueError:
        raise SystemExit("--fill-between: %s" % usage)
    return names, axis, max_gap


def _fill_between_keys_arg(text):
    """--fill-between-keys Z,Z,... -> the key slices"""
    try:
        keys = [int(v) for v in text.split(",") if v]
        if not keys or min(keys) < 0:
            raise ValueError
    except ValueError:
        raise SystemExit("--fill-between-keys: Z,Z,... -- the slices (coordinates along the axis of --fill-between) that count as painted")
    return keys


def _fill_between_table(result):
    """what --fill-between prints: per segment the keys, the gaps filled and refused and the texels that joined and left"""
    lines = []
    for r in result:
        s = r["summary"]
        lines.append("fill between: %s label %d, %d key slices, %d gaps of %d slices filled, %d refused: %d texels joined, %d left" % (
            r["name"], r["label"], s["n_keys"], s["n_gaps"], s["n_gap_slices"], s["n_refused"], r["relabel"]["arrived"].get(r["label"], 0),
            r["relabel"]["left"].get(r["label"], 0)))
    return "\n".join(lines)


def _smart_wand_arg(text):
    """--smart-wand-at X,Y:NAME:CONTRAST:MAX_COST -> (x, y, name, contrast, max_cost)"""
    usage = "X,Y:NAME:CONTRAST:MAX_COST -- a pixel, the segment that takes what the wand reaches, the cost of a byte of density change and the most a texel may cost"
    parts = text.split(":")
    try:
        x, y = (int(v) for v in parts[0].split(","))
        name, contrast, max_cost = parts[1], int(parts[2]), int(parts[3])
        if len(parts) != 4 or not name:
            raise ValueError
    except (ValueError, IndexError):
        raise SystemExit("--smart-wand-at: %s" % usage)
    return x, y, name, contrast, max_cost


def _label_edits(ctx, d, args):
    """the label edits of the command line on the scene as it stands (demo.Simple.relabel, the brush, stroke, lasso, split_at, keep_largest, grow, shrink):
    [(option, result)]"""
    out = []
    try:
        if getattr(args, "relabel", None):
            froms, to = _name_and(args.relabel, "--relabel", "FROM[,FROM...]:TO -- label values or segment names", None)
            out.append(("relabel", d.relabel(ctx, {_segment_arg(f): _segment_arg(to) for f in froms.split(",") if f})))
        if getattr(args, "brush", None):
            out.append(("brush", d._brush(ctx, _brush_arg(d, ctx, args.brush))))
        if getattr(args, "brush_at", None):
            usage = "X,Y[/X,Y...]:NAME:R -- pixels of the drag, the segment they paint and the radius in texels"
            rest, r = _name_and(args.brush_at, "--brush-at", usage)
            at, name = _name_and(rest, "--brush-at", usage, None)
            s = d.stroke(ctx, [_outline_at_arg(p, "--brush-at") for p in at.split("/")], _segment_arg(name), r, over=None)
            out.append(("brush_at", None if s["relabel"] is None else dict(s["relabel"], picked=s["picked"], missed=s["missed"], calls=s["calls"])))
        if getattr(args, "lasso", None):
            usage = "X,Y/X,Y/X,Y[/...]:FROM[,FROM...]:TO -- pixels of the polygon, the segments it cuts and the segment they join (label values or names)"
            rest, to = _name_and(args.lasso, "--lasso", usage, None)
            at, froms = _name_and(rest, "--lasso", usage, None)
            try:
                pixels = [tuple(int(v) for v in p.split(",")) for p in at.split("/")]
            except ValueError:
                raise SystemExit("--lasso: %s" % usage)
            if len(pixels) < 3 or any(len(p) != 2 for p in pixels):
                raise SystemExit("--lasso: %s" % usage)
            out.append(("lasso", d.lasso(ctx, pixels, _segment_arg(to), over=[_segment_arg(f) for f in froms.split(",") if f],
                                         outside=bool(getattr(args, "lasso_outside", False)))))
        if getattr(args, "smooth", None) is not None:
            names, radius = _smooth_arg(args.smooth)
            iterations = getattr(args, "smooth_iterations", None) or 1
            if iterations < 1:
                raise SystemExit("--smooth-iterations: N is a number of passes, got %d" % iterations)
            out.append(("smooth", d.smooth(ctx, names, radius, iterations)))
        if getattr(args, "split_at", None):
            at, to = _name_and(args.split_at, "--split-at", "X,Y:TO -- a pixel and the segment its piece becomes", None)
            p = d.split_at(ctx, *_outline_at_arg(at, "--split-at"), _segment_arg(to))
            out.append(("split_at", p["relabel"]))
        if getattr(args, "keep_largest", None):
            out.append(("keep_largest", d.keep_largest(ctx, _segment_arg(args.keep_largest))))
        if getattr(args, "grow", None):
            name, r = _name_and(args.grow, "--grow", "NAME:R -- a segment and a margin in texels")
            out.append(("grow", d.grow(ctx, _segment_arg(name), r)))
        if getattr(args, "shrink", None):
            name, r = _name_and(args.shrink, "--shrink", "NAME:R -- a segment and a margin in texels")
            out.append(("shrink", d.shrink(ctx, _segment_arg(name), r)))
        if getattr(args, "fill", None) is not None:
            names, r = _fill_arg(args.fill)
            out.append(("fill", d.fill(ctx, names, r, window=(1, 255))))
        if getattr(args, "separate", None):
            name, r = _name_and(args.separate, "--separate", "NAME:R -- a segment and the depth of its cores in texels")
            out.append(("separate", d.separate(ctx, _segment_arg(name), r)))
        if getattr(args, "flood", None) is not None:
            names, r = _fill_arg(args.flood)
            out.append(("flood", d.grow_through(ctx, names, None if r is None else int(r), window=(1, 255))))
        if getattr(args, "wand_at", None):
            x, y, name, tol, r = _wand_arg(args.wand_at)
            out.append(("wand", d.wand_at(ctx, x, y, _segment_arg(name), tol, r)))
        if getattr(args, "grow_from_seeds", None):
            names, contrast, max_cost = _grow_arg(args.grow_from_seeds)
            out.append(("grow_from_seeds", d.grow_from_seeds(ctx, names, contrast=contrast, max_cost=max_cost)))
        if getattr(args, "smart_wand_at", None):
            x, y, name, contrast, max_cost = _smart_wand_arg(args.smart_wand_at)
            out.append(("smart_wand", d.smart_wand_at(ctx, x, y, _segment_arg(name), contrast, max_cost)))
        if getattr(args, "fill_between", None):
            names, axis, max_gap = _fill_between_arg(args.fill_between)
            keys = _fill_between_keys_arg(args.fill_between_keys) if getattr(args, "fill_between_keys", None) else None
            out.append(("fill_between", d.fill_between(ctx, names, axis, max_gap, keys, replace=keys is not None)))
    except ValueError as e:
        raise SystemExit("label edit: %s" % e)
    return out


def run_simple(args):
    W, H = args.width, args.height
    raw, labels, segments, what = _load_assets(args)
    state = scene.State.with_parameters(W / H, scene.StateParameters())   # interactive defaults, src/state.rs:41-55
    state.update()
    with demo.GpuContext(W, H, args.device) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels, segments=segments, dims=(256, 256, 256))
        if args.crop:
            d.set_crop(ctx, *_crop_arg(args.crop))
        if args.clip_plane:
            d.set_clip_plane(ctx, *_clip_plane_arg(args.clip_plane))
        if args.hide:
            d.set_hidden(ctx, _hide_arg(args.hide))
        d.update_gpu_state(ctx, state)
        d.compute_pass(ctx)
        ctx.sync()
        clipped = None
        if args.clip_at:
            # click to cut: the plane through what the pixel shows, facing the eye; the PNG is the frame after the cut
            plane = d.clip_at(ctx, *_outline_at_arg(args.clip_at, "--clip-at"))
            clipped = {"clip_plane": None if plane is None else {"n": list(plane[0]), "d": plane[1]}}
            d.compute_pass(ctx)
            ctx.sync()
        # label edits, in the order relabel, brush, brush at pixels, lasso, smooth, split, keep the largest, grow, shrink; the PNG is the frame after them
        undo = getattr(args, "undo", None) or 0
        if undo < 0:
            raise SystemExit("--undo: N is a number of edits to take back, got %d" % undo)
        try:
            if undo:
                d.history(ctx)              # on before the edits: a step is journalled by the edit it takes back
        except ValueError as e:
            raise SystemExit("--undo: %s" % e)
        edits = _label_edits(ctx, d, args)
        for _ in range(undo):               # the last N edits back; None: nothing (left) to take back
            edits.append(("undo", d.undo(ctx)))
        if edits:
            d.compute_pass(ctx)
            ctx.sync()
        frame = ctx.read_rgba8()
        picked = d.pick(ctx, *_pick_arg(args.pick)) if getattr(args, "pick", None) else None
        outlined = None
        try:
            if getattr(args, "outline", None):
                outlined = {"outlined_labels": d.highlight(ctx, _outline_arg(args.outline))}
            if getattr(args, "outline_at", None):
                outlined = d.highlight_at(ctx, *_outline_at_arg(args.outline_at))
        except ValueError as e:
            raise SystemExit("--outline: %s" % e)
        if outlined is not None:
            frame = ctx.read_outline()      # the PNG is the annotated image
        slices, sliced_at = {}, None
        try:
            if getattr(args, "slice", None):
                axis, index = _slice_arg(args.slice)
                d.slice(ctx, axis, index, mode=_lib.SLICE_TF)
                slices[axis] = ctx.read_slice()
            if getattr(args, "slice_at", None):
                sliced_at = d.slices_at(ctx, *_outline_at_arg(args.slice_at, "--slice-at"), mode=_lib.SLICE_TF)
                slices.update(sliced_at.pop("slices") or {})
        except ValueError as e:
            raise SystemExit("--slice: %s" % e)
        projection = None
        if getattr(args, "project", None):
            mode, step = _project_arg(args.project)
            try:
                d.project(ctx, mode, step, tf=True)
            except ValueError as e:
                raise SystemExit("--project: %s" % e)
            projection = (mode.lower(), ctx.read_projection_image())
        measured = None
        if getattr(args, "measure", None) is not None:
            names = [v for v in args.measure.split(",") if v]
            try:
                measured = (d.measure(ctx, [int(v) if v.isdigit() else v for v in names] or None),
                            {"visible": d.histogram(ctx), **{v: d.histogram(ctx, [int(v) if v.isdigit() else v]) for v in names}})
            except ValueError as e:
                raise SystemExit("--measure: %s" % e)
        surfaced = None
        if getattr(args, "surface", None) is not None or getattr(args, "surface_out", None):
            names, min_byte = _surface_arg(args.surface or "")
            try:
                surfaced = d.surface(ctx, names, min_byte)
                if args.surface_out:
                    d.export_surface(ctx, args.surface_out, names, min_byte)
            except ValueError as e:
                raise SystemExit("--surface: %s" % e)
        pieces = None
        if getattr(args, "components", None) is not None:
            names, min_byte = _surface_arg(args.components, "--components")
            try:
                pieces = d.components(ctx, names, min_byte)
            except ValueError as e:
                raise SystemExit("--components: %s" % e)
        distances = None
        if getattr(args, "distance", None) is not None:
            names, min_byte = _surface_arg(args.distance, "--distance")
            inside = bool(getattr(args, "distance_inside", False))
            try:
                distances = d.distance(ctx, names, inside, min_byte)
                distances["hist"] = [int(v) for v in ctx.read_distance()["hist"]]
            except ValueError as e:
                raise SystemExit("--distance: %s" % e)
        labels_out = d.save_labels(ctx, args.labels_out) if getattr(args, "labels_out", None) else None
    path = args.screenshot or ("screenshot_%d.png" % int(time.time()))
    image.write_png(path, frame)
    print("run simple: %s, %dx%d -> %s" % (what, W, H, path))
    for option, result in edits:
        import json
        if option == "fill":
            print(_fill_table(d, result))
        elif option == "flood":
            print(_flood_table(d, result))
        elif option == "wand":
            print("wand: %s" % ("nothing under the pixel" if result["relabel"] is None else "%d texels joined label %d, density %d..%d" % (
                result["relabel"]["changed"], result["relabel"]["label"], result["relabel"]["window"][0], result["relabel"]["window"][1])))
        elif option == "grow_from_seeds":
            print(_grow_table(d, result))
        elif option == "smart_wand":
            print("smart wand: %s" % ("nothing under the pixel" if result["relabel"] is None else "%d texels joined label %d" % (
                result["relabel"]["changed"], result["relabel"]["label"])))
        elif option == "fill_between":
            print(_fill_between_table(result))
        elif option == "separate":
            print("separate: %d pieces%s" % (len(result), "".join(", %s %d texels" % (p["name"], p["texels"]) for p in result)))
        print(json.dumps({option: result}))      # one line per label edit: texels changed, per label left and arrived, the hull
    if labels_out is not None:
        print("labels: %d bytes -> %s" % (labels_out, args.labels_out))
    if distances is not None:
        import json
        print(_distance_table(distances, inside))
        stem = path[:-4] if path.lower().endswith(".png") else path
        with open(stem + "_distance.json", "w") as f:
            json.dump({"inside": inside, "n_solid": distances["n_solid"], "n_finite": distances["n_finite"], "max_d2": distances["max_d2"],
                       "max_at": list(distances["max_at"]), "hist": distances["hist"]}, f)
        print("distance histogram -> %s_distance.json" % stem)
    if pieces is not None:
        print(_components_table(pieces))
    if surfaced is not None:
        print(_surface_table(surfaced))
        if args.surface_out:
            print("surface: %s -> %s" % (", ".join(surfaced) or "no faces", args.surface_out))
    for axis, img in sorted(slices.items()):
        image.write_png(_slice_path(path, axis), img)
        print("slice %s: %dx%d -> %s" % (axis, img.shape[1], img.shape[0], _slice_path(path, axis)))
    if projection is not None:
        stem = path[:-4] if path.lower().endswith(".png") else path
        image.write_png("%s_project_%s.png" % (stem, projection[0]), projection[1])
        print("project %s: %dx%d -> %s_project_%s.png" % (projection[0], W, H, stem, projection[0]))
    if measured is not None:
        import json
        print(_measure_table(measured[0]))
        stem = path[:-4] if path.lower().endswith(".png") else path
        with open(stem + "_histogram.json", "w") as f:
            json.dump({k: [int(c) for c in v] for k, v in measured[1].items()}, f)
        print("histogram: %s -> %s_histogram.json" % (", ".join(measured[1]), stem))
    if sliced_at is not None:
        import json
        print(json.dumps(sliced_at))   # one line: the pick the three slices of --slice-at go through
    if clipped is not None:
        import json
        print(json.dumps(clipped))     # one line: the plane --clip-at set (null: the pixel shows nothing)
    if picked is not None:
        import json
        print(json.dumps(picked))      # one line: what the pixel shows (demo.Simple.pick)
    if outlined is not None:
        import json
        print(json.dumps(outlined))    # one line: the label values outlined, or the pick under --outline-at
    return 0


def flythrough(args):
    """Scripted fly-through (volym_amd/flythrough.py): mouse orbit, scroll zoom and every
    widget of the reference's panel over its range (src/gui.rs:198-277), one event + update + compute pass per frame
    (src/event_loop.rs:100-119).  --out DIR keeps every --keep-every-th frame as PNG and writes frames.json: the uniforms
    each kept frame was rendered with (what a test needs to render the same frames with the oracle) and, as metadata only, the
    crop box in texels it was rendered with (the whole volume unless --crop or --crop-sweep is given; the frames of a run
    without them are what they were before the crop box existed) and, with --hide only, the hidden label values ("hidden_labels")."""
    import json
    import os
    from . import flythrough as ft
    W, H = args.width, args.height
    raw, labels, segments, what = _load_assets(args)
    state = scene.State.with_parameters(W / H, scene.StateParameters())      # the interactive defaults, src/state.rs:41-55
    state.update()
    kept, times = [], []
    with demo.GpuContext(W, H, args.device) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels, segments=segments, dims=(256, 256, 256))
        if args.crop:
            d.set_crop(ctx, *_crop_arg(args.crop))
        plane = d.set_clip_plane(ctx, *_clip_plane_arg(args.clip_plane)) if args.clip_plane else None
        hidden = d.set_hidden(ctx, _hide_arg(args.hide)) if args.hide else None
        sweep = ft.crop_sweep(args.frames) if args.crop_sweep else None    # our widget: a crop face dragged over its range
        for i, ev in enumerate(ft.script(args.frames)):
            ft.apply(state, ev)
            state.update()
            if sweep:
                d.set_crop(ctx, *sweep[i])
            d.update_gpu_state(ctx, state)
            t0 = time.perf_counter()
            d.compute_pass(ctx)
            ctx.throttle(3)
            times.append(time.perf_counter() - t0)
            if args.out and i % max(1, args.keep_every) == 0:
                ctx.sync()
                name = "fly_%04d.png" % i
                image.write_png(os.path.join(args.out, name), ctx.read_rgba8())
                kept.append({"frame": i, "event": list(ev), "png": name, "crop_box": [list(b) for b in ctx.crop_box()],
                             "camera_uniforms": bytes(state.camera_uniforms()).hex(),
                             "parameter_uniforms": bytes(state.parameter_uniforms()).hex()})
                if hidden is not None:       # (a run without --hide writes the keys it always wrote)
                    kept[-1]["hidden_labels"] = hidden
                if plane is not None:        # (likewise --clip-plane)
                    kept[-1]["clip_plane"] = {"n": list(plane[0]), "d": plane[1]}
        ctx.sync()
    if args.out:
        with open(os.path.join(args.out, "frames.json"), "w") as f:
            json.dump({"width": W, "height": H, "frames": kept}, f)
    t = np.array(times)
    print("flythrough: %s, %dx%d, %d frames, %d kept: mean %.3f ms per frame (enqueue + back-pressure, 3 frames in flight)" % (
        what, W, H, args.frames, len(kept), t.mean() * 1e3))
    return 0


def turntable(args):
    """The camera orbits the volume the way a mouse drag does (State.process_mouse -> CameraController -> Camera::orbit,
    src/camera.rs:47-61, :96-117), one update + compute pass per frame, every frame a new view: the moving-camera
    figure (the work lists follow the view through the asynchronous cost feedback)."""
    W, H = args.width, args.height
    raw, labels, segments, what = _load_assets(args)
    p = scene.StateParameters.benchmark().replace(raymarching_step_size=args.step)
    state = scene.State.with_parameters(W / H, p)
    state.update()
    times = []
    with demo.GpuContext(W, H, args.device) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels, segments=segments, dims=(256, 256, 256))
        dx = -360.0 / args.frames / 0.2                     # mouse pixels per frame: sensitivity 0.2 deg/px, sign flipped
        dy = -20.0 / args.frames / 0.2
        for i in range(args.frames):
            state.process_mouse(dx, dy if i < args.frames // 2 else -dy)
            state.update()
            d.update_gpu_state(ctx, state)
            times.append(float(ctx.time_passes(1)[0]))
            if args.out and i % max(1, args.frames // args.keep) == 0:
                image.write_png("%s/turntable_%03d.png" % (args.out, i), ctx.read_rgba8())
    t = np.array(times[1:] if len(times) > 1 else times)
    print("turntable: %s, %dx%d, %d frames (one full turn): mean %.3f ms/frame, median %.3f, max %.3f => %.0f Mrays/s" % (
        what, W, H, args.frames, t.mean(), np.median(t), t.max(), W * H / (t.mean() * 1e-3) / 1e6))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="volym", description="MI355X ray-march path of volym")
    ap.add_argument("-d", "--debug", action="store_true", help="verbose logging (src/cli.rs:9-11)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--volume"); ap.add_argument("--labels"); ap.add_argument("--segments")
    sub = ap.add_subparsers(dest="command")
    run = sub.add_parser("run", help="run the demo (default)")
    run.add_argument("demo", nargs="?", default="simple", choices=["simple"])
    run.add_argument("--width", type=int, default=1280); run.add_argument("--height", type=int, default=720)
    run.add_argument("--screenshot")
    run.add_argument("--crop", help="crop box x0,y0,z0,x1,y1,z1 in unit-cube coordinates")
    run.add_argument("--hide", help="label values of the segments to hide, e.g. 3,4")
    run.add_argument("--clip-plane", help="NX,NY,NZ,PX,PY,PZ: oblique clip plane, normal and point in unit-cube coordinates; the side the normal points to is cut away")
    run.add_argument("--clip-at", help="X,Y: after the frame, cut along the plane through what pixel (X, Y) shows, facing the eye; the PNG is the frame after the cut")
    run.add_argument("--pick", help="X,Y[,ALPHA]: after the frame, print what pixel (X, Y) shows as one JSON line (segment, texel, depth)")
    run.add_argument("--outline", help="NAME[,NAME...]: segment names, ids or label values to outline and tint; the PNG is the annotated image")
    run.add_argument("--outline-at", help="X,Y: outline the segment pixel (X, Y) shows; the PNG is the annotated image")
    run.add_argument("--slice", help="AXIS,INDEX: also write the slice normal to x, y or z through texel INDEX as <screenshot>_slice_<axis>.png")
    run.add_argument("--measure", nargs="?", const="", metavar="NAME,...",
                     help="also print the table of segment statistics of the scene in view (all segments, or the named ones) and write the density "
                          "histograms as <screenshot>_histogram.json")
    run.add_argument("--surface", nargs="?", const="", metavar="NAME,...[:MIN_BYTE]",
                     help="also print the surface table of the scene in view (all segments, or the named ones; texels with a density byte of at "
                          "least MIN_BYTE, default 1, are solid): faces per axis, area, enclosed texels beside the measured count, sphericity")
    run.add_argument("--components", nargs="?", const="", metavar="NAME,...[:MIN_BYTE]",
                     help="also print, per segment (all in view, or the named ones), its connected pieces: how many, the largest, and the ten largest with root and box")
    run.add_argument("--distance", nargs="?", const="", metavar="NAME,...[:MIN_BYTE]",
                     help="also print the distance map's summary for the union of the named segments (default: every label): solid texels, the deepest "
                          "point, the nearest texel of every segment; and write the histogram as <screenshot>_distance.json")
    run.add_argument("--distance-inside", action="store_true", help="with --distance: distances inside the set, to its complement (thickness)")
    run.add_argument("--surface-out", metavar="FILE.stl|.obj", help="also write the surface of those segments together as a binary STL or an OBJ mesh")
    run.add_argument("--project", help="MAX|MEAN[,STEP]: also write the maximum or mean intensity projection of the view as <screenshot>_project_<mode>.png")
    run.add_argument("--relabel", help="FROM[,FROM...]:TO: relabel the segments FROM (label values or names) to TO on the device before the picture")
    run.add_argument("--brush", help="X,Y,Z[/X,Y,Z...]:TO:R2: paint segment TO (a label value or name) over every label within sqrt(R2) texels of that "
                                     "polyline of texels of the prepared volume, on the device, after --relabel; one undo step")
    run.add_argument("--brush-at", help="X,Y[/X,Y...]:NAME:R: drag the brush over those pixels: segment NAME within R texels of the polyline of the picked "
                                        "texels (a pixel without a pick breaks it)")
    run.add_argument("--lasso", help="X,Y/X,Y/X,Y[/...]:FROM[,FROM...]:TO: scissors: the texels of the segments FROM that the first frame's view projects into that "
                                     "polygon of pixels (closed implicitly, even-odd; vertices may lie off screen) join segment TO (0: unlabelled), on the device, "
                                     "after --brush-at; one undo step")
    run.add_argument("--smooth", nargs="?", const="", help="[NAME,...][:R[,R,R]]: smooth the segmentation on the device after the first frame: a majority filter over "
                     "R texels (default 1; R,R,R per axis, 1,1,0 inside slices) for the segments NAME against label 0, or jointly for every label without a "
                     "name (demo.Simple.smooth); prints the passes' results")
    run.add_argument("--smooth-iterations", type=int, help="with --smooth: N passes, each an undo step of its own (default 1)")
    run.add_argument("--lasso-outside", action="store_true", help="with --lasso: the texels that do NOT project into the polygon instead (keep only what is under it)")
    run.add_argument("--split-at", help="X,Y:TO: the piece of the segment pixel (X, Y) shows becomes segment TO (a new name gets an entry)")
    run.add_argument("--keep-largest", help="NAME: keep the largest piece of the segment, its other pieces become unlabelled")
    run.add_argument("--grow", help="NAME:R: grow the segment by R texels into the unlabelled texels")
    run.add_argument("--shrink", help="NAME:R: shrink the segment by R texels")
    run.add_argument("--fill", nargs="?", const="", metavar="NAME,...[:R]",
                     help="grow the named segments (default: every segment) at once into the unlabelled matter on the device, after --shrink: every unlabelled texel "
                          "with a density byte above 0 joins the segment it is nearest to, at most R texels away (default: however far) (demo.Simple.fill); one undo step")
    run.add_argument("--separate", metavar="NAME:R", help="separate touching objects of the segment: its cores at depth R become segments of their own and the rest "
                                                          "goes to the nearest of them (demo.Simple.separate); after --fill")
    run.add_argument("--flood", nargs="?", const="", metavar="NAME,...[:R]",
                     help="grow the named segments (default: every segment) at once THROUGH the unlabelled matter of density above 0 on the device, after --separate: "
                          "a texel joins the segment whose seed is the fewest 6-connected steps away, at most R (default: however far); gaps of air are no "
                          "bridge (demo.Simple.grow_through); one undo step")
    run.add_argument("--wand-at", metavar="X,Y:NAME:TOL[:R]", help="the magic wand: from the texel under pixel (X, Y) through the unlabelled matter whose density is within "
                                                                    "TOL of that texel's, at most R steps, into segment NAME (demo.Simple.wand_at); after --flood")
    run.add_argument("--grow-from-seeds", metavar="NAME[,NAME...][:CONTRAST[:MAX_COST]]",
                     help="grow from seeds on the device, after --wand-at: the named segments grow at once through the unlabelled matter of density above 0, where a "
                          "step costs 1 and CONTRAST (default 16) per byte of density change across it; a texel joins the segment that reaches it most cheaply, for "
                          "at most MAX_COST (default: however much) (demo.Simple.grow_from_seeds); one undo step")
    run.add_argument("--smart-wand-at", metavar="X,Y:NAME:CONTRAST:MAX_COST",
                     help="the wand that stops at edges: from the texel under pixel (X, Y) through the unlabelled matter, a step costing 1 and CONTRAST per byte of "
                          "density change, for at most MAX_COST, into segment NAME (demo.Simple.smart_wand_at); after --grow-from-seeds")
    run.add_argument("--fill-between", metavar="NAME[,NAME...]:AXIS[:MAX_GAP]",
                     help="fill between slices on the device, after --smart-wand-at: each named segment, painted on some slices perpendicular to AXIS (x, y or z), is "
                          "interpolated across the slices between them; gaps of more than MAX_GAP slices are left alone (default: no limit) "
                          "(demo.Simple.fill_between); one undo step per segment")
    run.add_argument("--fill-between-keys", metavar="Z,Z,...", help="with --fill-between: only these slices count as painted, and what the segment holds on the "
                                                                     "slices between them outside the interpolated shape goes back to label 0 -- the way to fill again "
                                                                     "after a key slice was repainted")
    run.add_argument("--undo", type=int, metavar="N", help="keep a history of the label edits above on the device and take the last N back, before the "
                                                           "picture and --labels-out; each prints a JSON line {\"undo\": ...}")
    run.add_argument("--labels-out", help="FILE: write the labels as they stand after the edits, raw bytes in the orientation of --labels")
    run.add_argument("--slice-at", help="X,Y: also write the three orthogonal slices through the texel pixel (X, Y) shows")
    b = sub.add_parser("benchmark", help="run benchmarks on all demos")
    b.add_argument("--width", type=int, default=1024); b.add_argument("--height", type=int, default=768)   # src/main.rs:356-359
    b.add_argument("--secs", type=float, default=0.25, help="GPU seconds per trial (the reference uses 2 s of wall clock)")
    b.add_argument("--output", default="benchmark_results.csv")
    b.add_argument("--frames-in-flight", type=int, choices=[1, 2], default=1,
                   help="2: compute passes alternate between two frame contexts on the device (VOLYM_OPT_FRAMES_IN_FLIGHT), frames per wall clock")
    tt = sub.add_parser("turntable", help="scripted orbit of the camera (moving-view timing)")
    tt.add_argument("--width", type=int, default=1920); tt.add_argument("--height", type=int, default=1080)
    tt.add_argument("--frames", type=int, default=72); tt.add_argument("--step", type=float, default=0.01)
    tt.add_argument("--out"); tt.add_argument("--keep", type=int, default=6)
    fl = sub.add_parser("flythrough", help="scripted fly-through: orbit, zoom and every GUI widget over its range")
    fl.add_argument("--width", type=int, default=1280); fl.add_argument("--height", type=int, default=720)
    fl.add_argument("--frames", type=int, default=120); fl.add_argument("--out"); fl.add_argument("--keep-every", type=int, default=10)
    fl.add_argument("--crop", help="crop box x0,y0,z0,x1,y1,z1 in unit-cube coordinates")
    fl.add_argument("--hide", help="label values of the segments to hide, e.g. 3,4")
    fl.add_argument("--clip-plane", help="NX,NY,NZ,PX,PY,PZ: oblique clip plane, normal and point in unit-cube coordinates")
    fl.add_argument("--crop-sweep", action="store_true", help="drag the far z crop face over its range while flying (not a widget of the reference)")
    dv = sub.add_parser("devtools", help="3D-Slicer .seg.nrrd -> segments.json + label .raw (volym_devtools)")
    dv.add_argument("nrrd"); dv.add_argument("segments_json"); dv.add_argument("binary_data")
    args = ap.parse_args(argv)
    if args.command == "devtools":
        from . import devtools
        segs, n = devtools.convert(args.nrrd, args.segments_json, args.binary_data)
        print("devtools: %d segments -> %s, %d label bytes -> %s" % (len(segs), args.segments_json, n, args.binary_data))
        return 0
    if args.command == "benchmark":
        return benchmark(args)
    if args.command == "flythrough":
        return flythrough(args)
    if args.command == "turntable":
        return turntable(args)
    if args.command is None:
        args.width, args.height, args.screenshot = 1280, 720, None
    return run_simple(args)


if __name__ == "__main__":
    sys.exit(main())
