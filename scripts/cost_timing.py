"""What the cost pass and the spread cost (volym_cost_pass, volym_spread_labels), on seeded synthetic bonsai volumes
with their label maps on the device: synth_bonsai(256) in the linear layout and synth_bonsai(1024) in the bricked one.  The cases are
those of scripts/geodesic_timing.py, and the geodesic pass on the same request, measured in the same run in alternating blocks, is
the yardstick: what the weights cost is the ratio to it.

  the pass     from the trunk (label 3) through the unlabelled matter; from every label; a wand from one texel of the canopy through
               the canopy's matter -- each with contrast_cost 0 and with contrast_cost --contrast (step_cost 1, no limit).  The pass
               blocks, so a host clock around the call is its cost as a caller sees it.  --reps passes per block after 2 warm-ups,
               --blocks blocks per case, cost and geodesic blocks alternating: minimum over all passes, median of the block medians,
               their range (spread), and the ratio of the medians.  With the development build (make DEV=1, VOLYM_HIP_LIB) the rounds
               enqueued and the tiles relaxed in all are printed beside them, for both passes.
  the batch    the first case with the contrast again with VOLYM_COST_BATCH = 1, 2, 4, 8, 16 and 32 rounds between two reads of the
               count (the development build reads the variable; the product build does not).
  the spread   after the pass from the trunk: a host clock around volym_spread_labels, ending in volym_sync, --edit-reps times, and
               volym_flood_labels of the same texels by the geodesic map beside it; between two a relabel sends the texels back.
  the host     once, at sizes up to --host-up-to: volym_read_labels, a heap (scipy.sparse.csgraph.dijkstra from all seeds at once
               over the medium's graph) where scipy is installed, else the NumPy twin, np.where, volym_set_labels and the table again.

    python scripts/cost_timing.py [--sizes 256,1024] [--contrast 16] [--reps 5] [--blocks 3] [--edit-reps 5] [--out profiles/cost.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (torch's HIP runtime first, as in bench.py)

from scripts.distance_timing import _line  # noqa: E402
from scripts.geodesic_timing import _blocking, _ms  # noqa: E402
from scripts.geodesic_timing import _counts as _geodesic_counts  # noqa: E402
from volym_amd import _lib, demo, scene, synth  # noqa: E402


def _counts(ctx):
    """(rounds, tiles relaxed) of the latest cost pass, or None without the development build"""
    call = getattr(_lib.lib(), "volym_dev_cost_counts", None)
    if call is None:
        return None
    out = (C.c_ulonglong * 2)()
    call.argtypes, call.restype = [C.c_void_p, C.POINTER(C.c_ulonglong)], C.c_int
    return (int(out[0]), int(out[1])) if call(ctx.handle, out) == 0 else None


def _said(counts):
    return "" if counts is None else "   %d rounds enqueued, %s tiles relaxed" % (counts[0], "{:,}".format(counts[1]))


def host_costs(vol3, passable, seeds, step, contrast):
    """cost of every texel from the nearest of `seeds` (bool [z, y, x]) through `passable`, by scipy's heap; inf where not reached"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    n = vol3.size
    index = np.arange(n, dtype=np.int32).reshape(vol3.shape)
    b = vol3.astype(np.int32)
    rows, cols, data = [], [], []
    for axis in range(3):
        a, d = [slice(None)] * 3, [slice(None)] * 3
        a[axis], d[axis] = slice(1, None), slice(0, -1)
        a, d = tuple(a), tuple(d)
        ok = passable[a] & passable[d]
        rows.append(index[a][ok]); cols.append(index[d][ok])
        data.append((step + contrast * np.abs(b[a][ok] - b[d][ok])).astype(np.float64))
    graph = coo_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    return dijkstra(graph, directed=False, indices=np.flatnonzero(seeds.ravel()), min_only=True).reshape(vol3.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--contrast", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--edit-reps", type=int, default=5)
    ap.add_argument("--host-up-to", type=int, default=256, help="largest size at which the host route is timed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = getattr(_lib.lib(), "volym_dev_cost_counts", None) is not None
    lines = ["cost pass beside the geodesic pass on the same request, microseconds, a host clock round each of %d blocking passes per block, %d blocks per pass and case, "
             "alternating;" % (a.reps, a.blocks), "min = minimum over all passes, median = median of the block medians, spread = range of the block medians; "
             "ratio = cost median / geodesic median", "%s build" % ("development" if dev else "product"), ""]
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
            cases = (("from the trunk through the unlabelled matter", trunk),
                     ("from every label through the unlabelled matter", scene.Geodesic(whole, 0, (1, 255), T(range(1, 256)), T([0]))),
                     ("a wand from %r of the canopy, byte %d +- 40" % (click, byte), scene.Geodesic(whole, 0, (max(byte - 40, 0), min(byte + 40, 255)), T([]), T([2]), 0, [click])))
            as_cost = lambda g, contrast: scene.Cost(g.box, g.flags, g.window, g.seed, g.through, 1, contrast, 0, g.points, 8)
            for case, g in cases:
                for contrast in (0, a.contrast):
                    q = as_cost(g, contrast)
                    cost, geo = [], []
                    for _ in range(a.blocks):
                        cost.append(_blocking(ctx, stream, lambda: ctx.cost_pass(q), a.reps)[0])
                        geo.append(_blocking(ctx, stream, lambda: ctx.geodesic_pass(g), a.reps)[0])
                    s = ctx.read_cost()
                    lines.append("  %s, contrast_cost %d: %s seeds, %s medium, %s reached, at most a cost of %s" % (
                        case, contrast, "{:,}".format(int(s["n_seed"])), "{:,}".format(int(s["n_medium"])), "{:,}".format(int(s["n_reached"])),
                        "none" if not int(s["n_reached"]) else int(s["max_cost"])))
                    ratio = float(np.median([np.median(b) for b in cost])) / float(np.median([np.median(b) for b in geo]))
                    lines += [_line("cost pass", cost) + _said(_counts(ctx)), _line("geodesic pass", geo) + _said(_geodesic_counts(ctx)), "    ratio %.2f" % ratio]
            # the batch
            weighted = as_cost(trunk, a.contrast)
            lines.append("  rounds per batch (VOLYM_COST_BATCH%s), from the trunk with contrast_cost %d, host microseconds:" % ("" if dev else "; NOT READ by this build", a.contrast))
            for batch in (1, 2, 4, 8, 16, 32):
                os.environ["VOLYM_COST_BATCH"] = str(batch)
                host = [_blocking(ctx, stream, lambda: ctx.cost_pass(weighted), a.reps)[0] for _ in range(a.blocks)]
                lines.append(_line("batch %d" % batch, host) + _said(_counts(ctx)))
            del os.environ["VOLYM_COST_BATCH"]
            # the spread beside the flood of the same texels
            ctx.cost_pass(weighted)
            ctx.geodesic_pass(trunk)
            spread = scene.Spread(whole, 0, (0, 255), T([0]), T([3]), {3: 7}, (1, 0xFFFFFFFF))
            flood = scene.Flood(whole, 0, (0, 255), T([0]), T([3]), {3: 7}, (1, 0xFFFFFFFF))
            back = scene.Relabel(whole, to={7: 0})
            changed = int(ctx.spread_labels(spread)["changed"])
            assert int(ctx.edit_labels(back)["changed"]) == changed
            assert int(ctx.flood_labels(flood)["changed"]) == changed, "one seed label: what it reaches is what it reaches most cheaply"
            ctx.edit_labels(back)
            ctx.sync()
            spreads, floods = [], []
            for _ in range(a.edit_reps):
                for call, request, out in ((ctx.spread_labels, spread, spreads), (ctx.flood_labels, flood, floods)):
                    t0 = time.perf_counter()
                    call(request)
                    ctx.sync()
                    out.append((time.perf_counter() - t0) * 1e3)
                    ctx.edit_labels(back)
                    ctx.sync()
            lines += ["  the spread: what the trunk reaches through the unlabelled matter becomes label 7, %s texels; milliseconds, median (min .. max)" % "{:,}".format(changed),
                      "    volym_spread_labels                        %s" % _ms(spreads), "    volym_flood_labels, the same texels        %s" % _ms(floods)]
            if n <= a.host_up_to:
                t0 = time.perf_counter()
                now = ctx.read_labels()
                t1 = time.perf_counter()
                v3 = vol.reshape(n, n, n)
                try:
                    reach = host_costs(v3, (v3 >= 1) & ((now == 0) | (now == 3)), (now == 3) & (v3 >= 1), 1, a.contrast)
                    how = "scipy.sparse.csgraph.dijkstra"
                    new = np.where(np.isfinite(reach) & (now == 0), 7, now).astype(np.uint8)
                except ImportError:
                    how = "the NumPy twin (scipy is not installed)"
                    _, keys = scene.cost_volume(vol, dims, weighted, labels=now.ravel())
                    new = np.where((keys != np.uint32(_lib.COST_NONE)) & (now == 0), 7, now).astype(np.uint8)
                t2 = time.perf_counter()
                ctx.set_labels(new.ravel(), dims)
                ctx.set_segment_importances(table)
                ctx.sync()
                t3 = time.perf_counter()
                assert int((new != now).sum()) == changed, "the host route must move the texels the spread moves"
                lines.append("    the host route, once: volym_read_labels %.1f ms, %s %.1f ms, the re-upload %.1f ms: %.1f ms" % (
                    (t1 - t0) * 1e3, how, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
        lines.append("")
        print("\n".join(lines[-48:]), flush=True)
        if a.out:                                       # (after every size: a run cut short keeps what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
