"""The scenes and requests of the cost tests, shared by tests/test_cost_host.py (which pins the host twins to a heap-based search per
label, to a restatement of the device's schedule, to closed forms and to per-texel loops) and tests/test_gpu_cost.py (which compares
the device with the twins).  Scenes A and B, their boxes, cut states and request pools are those of tests/geodesic_scenes.py, each
request given a rotating (step_cost, contrast_cost, max_cost); the constructed scenes of that file come back with unit steps and with
steps of 3, where their closed forms still hold; the scenes built about weights -- the ramp, the ridge, the tile that is lowered again
and again, the ties of unequal step counts, the row that passes 2^24 -- are built here.  The tile's extents are read from
volym_amd/csrc/cost_kernels.h, so that the scenes built about tile faces follow them.
"""
import os
import re

import numpy as np

from tests import geodesic_scenes as GS

ROOT = GS.ROOT
DIMS, NX, NY, NZ = GS.DIMS, GS.NX, GS.NY, GS.NZ
BOX, PLANE, HIDDEN = GS.BOX, GS.PLANE, GS.HIDDEN
BOXES, CUTS = GS.BOXES, GS.CUTS
LONG_DIMS, LONG_BOXES = GS.LONG_DIMS, GS.LONG_BOXES
scene_a, scene_b = GS.scene_a, GS.scene_b
table = GS.table
NONE = 0xFFFFFFFF                   # _lib.COST_NONE
COST_MAX = 0xFFFFFD                 # _lib.COST_MAX
UNCUT = 1                           # _lib.COST_UNCUT
SPREAD_UNCUT, SPREAD_DRY_RUN = 1, 2 # _lib.SPREAD_UNCUT, _lib.SPREAD_DRY_RUN


def tile():
    """(TX, TY, TZ) of volym_amd/csrc/cost_kernels.h"""
    text = open(os.path.join(ROOT, "volym_amd", "csrc", "cost_kernels.h")).read()
    m = re.search(r"constexpr uint32_t COST_TX = (\d+)u, COST_TY = (\d+)u, COST_TZ = (\d+)u;", text)
    assert m, "cost_kernels.h names the tile's extents"
    return tuple(int(v) for v in m.groups())


def _flat(a):
    return np.ascontiguousarray(a, np.uint8).ravel()


# ---- requests over scenes A and B ------------------------------------------------------------------------------------------------------
# (step_cost, contrast_cost, max_cost, hist_shift) in rotation
WEIGHTS = [(1, 0, 0, 0), (1, 1, 0, 2), (3, 17, 0, 6), (2, 255, 0, 12), (1, 4, 300, 1), (255, 255, 0, 16), (5, 0, 40, 0), (1, 17, 2000, 4)]


def weighted(g, k):
    """the scene.Cost with the box, flags, window, tables and points of the scene.Geodesic g and the k-th weights of the rotation"""
    from volym_amd import scene
    step, contrast, limit, shift = WEIGHTS[k % len(WEIGHTS)]
    return scene.Cost(g.box, g.flags, g.window, g.seed, g.through, step, contrast, limit, g.points, shift)


def requests(flags=0, turn=0):
    """(name, scene.Cost): the requests of the geodesic scenes, each with the weights its place in the list and the turn give it"""
    return [("%s / weights %d" % (name, (k + 3 * turn) % len(WEIGHTS)), weighted(g, k + 3 * turn)) for k, (name, g) in enumerate(GS.requests(flags, turn))]


def expect(host, c, labels=True):
    """the twin's (summary, keys) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.cost_volume(now, host.dims, c, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


as_bytes = GS.as_bytes              # the 6184 bytes of struct volym_cost_summary, then the key map
predicates = GS.predicates          # (seed, medium) over the request's box: the cost pass's are the geodesic pass's
check_closed = GS.check_closed      # a closed form's "at" reads (cost, label)


# ---- the rule restated ---------------------------------------------------------------------------------------------------------------
def _step(c, a, b):
    return c.step + c.contrast * abs(int(a) - int(b))


def dijkstra(seed, medium, label, density, c):
    """The rule label by label: a search with a heap from the seeds of one label at a time, texel by texel; cost is the smallest of
    the searches' costs and cost_label the smallest label that attains it.  Returns (keys as int64 with -1 for NONE, ties): ties
    counts the texels at which two labels or more attain the cost."""
    import heapq
    depth, h, w = seed.shape
    best = np.full(seed.shape, -1, np.int64)
    winner = np.zeros(seed.shape, np.int64)
    tied = np.zeros(seed.shape, bool)
    for l in sorted(set(label[seed].tolist())):
        dist = np.full(seed.shape, -1, np.int64)
        heap = [(0, tuple(t)) for t in np.argwhere(seed & (label == l)).tolist()]
        for _, t in heap:
            dist[t] = 0
        done = set()
        while heap:
            d, t = heapq.heappop(heap)
            if t in done or d != dist[t]:
                continue
            done.add(t)
            z, y, x = t
            for dz, dy, dx in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
                u = (z + dz, y + dy, x + dx)
                if 0 <= u[0] < depth and 0 <= u[1] < h and 0 <= u[2] < w and medium[u] and not seed[u]:
                    nd = d + _step(c, density[t], density[u])
                    if dist[u] < 0 or nd < dist[u]:
                        dist[u] = nd
                        heapq.heappush(heap, (nd, u))
        reached = dist >= 0
        tied |= reached & (best == dist)
        better = reached & ((best < 0) | (dist < best))           # (labels ascend: an equal cost keeps the smaller label)
        tied &= ~better
        best[better] = dist[better]
        winner[better] = l
    best[best > (c.max_cost or COST_MAX)] = -1
    return np.where(best >= 0, best << 8 | winner, -1), int((tied & (best >= 0)).sum())


def scheduled(seed, medium, label, density, c, tiles, rng, from_seeds=False):
    """The device's schedule restated: the keys start as the label on a seed, OPEN on the medium and NONE elsewhere; tiles of
    `tiles` = (tx, ty, tz) texels are relaxed one at a time, in a random order, each to its own fixed point against a halo read once
    (each halo word as old as the round's beginning or as fresh as the latest store, at random), and a tile that lowered a word marks
    its six neighbours for the next round; until no tile is marked.  Round 0 holds every tile, or with from_seeds those the init
    kernel marks: the tiles that hold a seed and their six neighbours (a superset of the tiles beyond the faces seeds lie on).
    Returns (the keys as int64, -1 for NONE; {tile origin (z, y, x): the rounds in which it lowered a word})."""
    none, open_ = 1 << 40, (1 << 40) - 1
    limit = (c.max_cost or COST_MAX) << 8 | 0xFF
    depth, h, w = seed.shape
    tx, ty, tz = tiles
    key = np.pad(np.where(seed, label.astype(np.int64), np.where(medium, open_, none)), 1, constant_values=none)     # (index + 1)
    b = np.pad(density.astype(np.int64), 1)
    grid = [(k, j, i) for k in range(0, depth, tz) for j in range(0, h, ty) for i in range(0, w, tx)]
    around = ((0, 0, tx), (0, 0, -tx), (0, ty, 0), (0, -ty, 0), (tz, 0, 0), (-tz, 0, 0))
    inside = lambda t: 0 <= t[0] < depth and 0 <= t[1] < h and 0 <= t[2] < w
    if from_seeds:
        marked = set()
        for z, y, x in np.argwhere(seed).tolist():
            t = (z // tz * tz, y // ty * ty, x // tx * tx)
            marked |= {t} | {n for n in ((t[0] + d[0], t[1] + d[1], t[2] + d[2]) for d in around) if inside(n)}
    else:
        marked = set(grid)
    lowered_in, round_ = {}, 0
    shifts = [((slice(1, -1), slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1), slice(2, None))),
              ((slice(1, -1), slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None), slice(1, -1))),
              ((slice(0, -2), slice(1, -1), slice(1, -1)), (slice(2, None), slice(1, -1), slice(1, -1)))]
    core = (slice(1, -1), slice(1, -1), slice(1, -1))
    while marked:
        order = sorted(marked)
        rng.shuffle(order)
        nxt = set()
        stale = key.copy()                                          # a tile's halo is as old as the round's beginning, or fresher
        for k, j, i in order:
            region = (slice(k, min(k + tz, depth) + 2), slice(j, min(j + ty, h) + 2), slice(i, min(i + tx, w) + 2))
            pad, bytes_ = key[region].copy(), b[region]
            halo = np.ones(pad.shape, bool)
            halo[core] = False
            pad = np.where(halo & (rng.random(pad.shape) < 0.5), stale[region], pad)
            own = bytes_[core]
            lowered = False
            while True:
                cur = pad[core]
                m = np.full(cur.shape, none, np.int64)
                for pair in shifts:
                    for s in pair:
                        u = pad[s]
                        m = np.minimum(m, np.where(u < open_, u + ((c.step + c.contrast * np.abs(bytes_[s] - own)) << 8), none))
                take = (cur != none) & (m <= limit) & (m < cur)
                if not take.any():
                    break
                cur[take] = m[take]
                lowered = True
            if lowered:
                key[region][core] = pad[core]
                lowered_in.setdefault((k, j, i), []).append(round_)
                nxt |= {n for n in ((k + d[0], j + d[1], i + d[2]) for d in around) if inside(n)}
        marked = nxt
        round_ += 1
    final = key[core]
    return np.where(final < open_, final, -1), lowered_in


def summary_by_loops(keys, seed, medium, lo, hist_shift):
    """every field of the summary by plain loops over the texels of the box, as a dict"""
    out = {"n_seed": 0, "n_medium": 0, "n_reached": 0, "max_cost": NONE, "max_at": [0, 0, 0], "cell": [0] * 256, "cell_medium": [0] * 256, "hist": [0] * 256}
    most = -1
    for (z, y, x), k in np.ndenumerate(keys):
        out["n_seed"] += bool(seed[z, y, x])
        out["n_medium"] += bool(medium[z, y, x]) and not seed[z, y, x]
        if int(k) == NONE:
            continue
        cost, l = int(k) >> 8, int(k) & 0xFF
        out["n_reached"] += 1
        out["cell"][l] += 1
        out["cell_medium"][l] += not seed[z, y, x]
        out["hist"][min(cost >> hist_shift, 255)] += 1
        if cost > most:                                            # (ndenumerate ascends in (z, y, x): the first of the largest stays)
            most, out["max_cost"], out["max_at"] = cost, cost, [lo[0] + x, lo[1] + y, lo[2] + z]
    return out


# ---- the constructed scenes: name -> (dims, vol, labels, request keywords, closed form) ------------------------------------------------
# closed form: as in tests/geodesic_scenes.py -- "keys", "at" ({texel (x, y, z): (cost, label) or None}), "max_at", "n_reached"
_manhattan = GS._manhattan


def unit_cases():
    """(name, dims, vol, labels, scene.Geodesic, closed form): every constructed scene of the geodesic tests.  With step_cost 1 and
    contrast_cost 0 the cost map is the geodesic map, byte for byte; with step_cost c it is that map with the steps multiplied by c."""
    return [(name, dims, vol, lab, g, closed) for name, (dims, vol, lab, g, closed) in GS.constructed().items()]


def times(keys, c):
    """a geodesic key map (uint32, NONE kept) with its steps multiplied by c"""
    k = keys.astype(np.int64)
    return np.where(keys == np.uint32(NONE), np.int64(NONE), ((k >> 8) * c) << 8 | (k & 0xFF)).astype(np.uint32)


def unit_request(g, c=1):
    """the cost request that restates the geodesic request g with steps that cost c each"""
    from volym_amd import scene
    return scene.Cost(g.box, g.flags, g.window, g.seed, g.through, c, 0, g.max_steps * c, g.points, 0)


def ramp():
    """an open box larger than a tile on every axis with b = min(x + y + z, 255), seeded at the origin: every monotone chain is
    cheapest, so cost = step * (x + y + z) + contrast * (b(t) - b(0)), and the far corner is the dearest"""
    tx, ty, tz = tile()
    dims = (tx + 5, ty + 3, tz + 2)
    zz, yy, xx = np.indices(dims[::-1])
    b = np.minimum(xx + yy + zz, 255)
    step, contrast = 3, 7
    n = dims[0] * dims[1] * dims[2]
    return dims, _flat(b), np.zeros(n, np.uint8), {"window": (0, 255), "seed": table(), "points": [(0, 0, 0)], "step": step, "contrast": contrast}, \
        {"keys": (step * (xx + yy + zz) + contrast * (b - b[0, 0, 0])) << 8, "max_at": tuple(v - 1 for v in dims), "n_reached": n}


RIDGE_STEP, RIDGE_CONTRAST = 1, 1


def ridge(two_labels):
    """A flat plateau of byte 50 cut by a one-texel ridge of byte 250 at x = TX, from y = 0 to the last row but one: the only flat way
    round it is through the last row.  One seed (a point) two texels before the ridge in row 0 and the target T two texels behind it:
    four steps over the ridge, or the flat detour through the last row.  Or two seeds of labels 1 and 2, ten texels before and two
    behind: in steps they meet four texels before the ridge, in cost at the ridge."""
    tx, ty, tz = tile()
    dims = (tx + 6, 4 * ty + 3, 3)
    rx, last = tx, 4 * ty + 2
    vol = np.full(dims[::-1], 50, np.uint8)
    vol[:, :last, rx] = 250
    lab = np.zeros(dims[::-1], np.uint8)
    kw = {"window": (1, 255), "through": table(0), "step": RIDGE_STEP, "contrast": RIDGE_CONTRAST}
    if two_labels:
        lab[1, 0, rx - 10], lab[1, 0, rx + 2] = 1, 2
        kw["seed"] = table(1, 2)
        at = {(x, 0, 1): (RIDGE_STEP * (x - (rx - 10)), 1) for x in range(rx - 9, rx)}
        at[(rx, 0, 1)] = (2 * RIDGE_STEP + 200 * RIDGE_CONTRAST, 2)
        at[(rx + 1, 0, 1)] = (RIDGE_STEP, 2)
        return dims, _flat(vol), _flat(lab), kw, {"at": at, "n_reached": dims[0] * dims[1] * dims[2]}
    s, t = (rx - 2, 0, 1), (rx + 2, 0, 1)
    detour = [(x, 0, 1) for x in range(rx - 2, rx)] + [(rx - 1, y, 1) for y in range(1, last + 1)] + [(x, last, 1) for x in range(rx, rx + 2)] + \
             [(rx + 1, y, 1) for y in range(last - 1, -1, -1)] + [t]
    kw.update(seed=table(), points=[s])
    return dims, _flat(vol), _flat(lab), kw, {"at": {t: (RIDGE_STEP * (len(detour) - 1), 0)}, "detour": detour, "over": 4 * RIDGE_STEP + 400 * RIDGE_CONTRAST,
                                               "n_reached": dims[0] * dims[1] * dims[2]}


def relowered():
    """Three corridors of matter, one texel wide, to one target T, each from a seed of its own label, in air.  The first is short and
    steep (2 tile faces, bumps of two bytes), the second longer and less steep (5 faces, bumps of one byte), the third the longest and
    flat (9 faces): T's tile converges by the first, is lowered by the second when it arrives rounds later, and again by the third.
    The closed form names T, the three seeds and the corridors' costs."""
    tx, ty, tz = tile()
    step, contrast = 1, 10
    zt = 2 * tz + 3
    t = (4, 4, zt)
    l1, l2, l3 = 2 * tz, 5 * tz, 9 * ty
    dims = (8, 4 + l3 + 4, zt + l2 + 5)
    vol = np.zeros(dims[::-1], np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    vol[zt - l1:zt + l2 + 1, 4, 4] = 150
    vol[zt, 4:4 + l3 + 1, 4] = 150
    for k in range(5):
        vol[zt - l1 + 2 + 2 * k, 4, 4] = 152                      # five bumps of two bytes, up and down: 40 each
    for k in range(3):
        vol[zt + 10 + 4 * k, 4, 4] = 151                          # three bumps of one byte: 20 each
    seeds = {7: (4, 4, zt - l1), 8: (4, 4, zt + l2), 9: (4, 4 + l3, zt)}
    for l, (x, y, z) in seeds.items():
        lab[z, y, x] = l
    costs = {7: step * l1 + 5 * 4 * contrast, 8: step * l2 + 3 * 2 * contrast, 9: step * l3}
    return dims, _flat(vol), _flat(lab), {"window": (1, 255), "seed": table(7, 8, 9), "through": table(0), "step": step, "contrast": contrast}, \
        {"at": {t: (costs[9], 9)}, "seeds": seeds, "costs": costs, "faces": {7: l1 // tz, 8: l2 // tz, 9: l3 // ty}}


def tied(axis, on_face):
    """Matter of byte 90 everywhere but for the two seeds: label 5, of byte 90, six texels before T along `axis`, and label 3, of byte
    94, two texels behind it.  With step 1 and contrast 1 the flat route costs 6 steps, the short one 2 steps and the 4 bytes out of
    its seed: equal cost from unequal step counts, and 3 wins T.  T lies on a tile face (the first texel of the second tile) or in
    the second tile's interior."""
    ext = tile()
    dims = (2 * ext[0] + 9, 2 * ext[1] + 11, 2 * ext[2] + 10)
    t = [ext[0] // 2 - 1, ext[1] // 2, ext[2] // 2]
    t[axis] = ext[axis] if on_face else ext[axis] + ext[axis] // 2
    flat_n, steep_n, rise = 6, 2, 4
    lo, hi = list(t), list(t)
    lo[axis] -= flat_n
    hi[axis] += steep_n
    vol = np.full(dims[::-1], 90, np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    lab[lo[2], lo[1], lo[0]], lab[hi[2], hi[1], hi[0]] = 5, 3
    vol[hi[2], hi[1], hi[0]] = 90 + rise
    # (no chain passes through a seed; the texels straight behind either seed, which the other's flat chains reach two steps later than
    # their distance says, are the nearer seed's by more than that)
    keys = np.minimum(_manhattan(dims, lo) << 8 | 5, (_manhattan(dims, hi) + rise) << 8 | 3)
    keys[lo[2], lo[1], lo[0]], keys[hi[2], hi[1], hi[0]] = 5, 3
    return dims, _flat(vol), _flat(lab), {"window": (1, 255), "seed": table(3, 5), "through": table(0), "step": 1, "contrast": 1}, \
        {"keys": keys, "at": {tuple(t): (flat_n, 3)}}


OVERFLOW_ROW = 330


def overflow():
    """Two rows of 330 texels alternating bytes 0 and 255 along x, step_cost = contrast_cost = 255, no limit, seeded at one end: a step
    along x costs 65 280.  257 of them cost 16 776 960 <= 2^24 - 3, 258 would pass it -- and key(257) + (65 280 << 8) passes 2^32, where
    a wrapped sum would read as a cost of 16 711 168, below the limit.  The texels up to there hold exact costs, those beyond NONE."""
    dims = (OVERFLOW_ROW, 2, 1)
    zz, yy, xx = np.indices(dims[::-1])
    vol = np.where(xx % 2 == 0, 0, 255)
    cost = 65280 * xx + 255 * yy
    keys = np.where(cost <= COST_MAX, cost << 8, -1)
    return dims, _flat(vol), np.zeros(vol.size, np.uint8), {"window": (0, 255), "seed": table(), "points": [(0, 0, 0)], "step": 255, "contrast": 255, "hist_shift": 16}, \
        {"keys": keys, "n_reached": int((keys >= 0).sum()), "max_at": (257, 0, 0), "at": {(257, 0, 0): (257 * 65280, 0), (258, 0, 0): None, (257, 1, 0): None, (256, 1, 0): (256 * 65280 + 255, 0)}}


def noise(dims, box=None, seed=7, share=0.7, weights=(2, 9, 0)):
    """random matter (`share` of the texels, bytes 1..255) with labels 0..3, seeds 1 and 2 through 0 and 3"""
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    kw = {"seed": table(1, 2), "through": table(0, 3), "step": weights[0], "contrast": weights[1], "max_cost": weights[2], "hist_shift": 3}
    if box is not None:
        kw["box"] = box
    return dims, np.where(rng.random(n) < share, rng.integers(1, 256, n), 0).astype(np.uint8), rng.choice([0, 0, 0, 0, 0, 3, 3, 1, 2], n).astype(np.uint8), kw, {}


def flat(axis):
    """an extent of 1 along `axis`, more than a tile along the others"""
    ext = tile()
    dims = [ext[0] + 5, ext[1] + 6, ext[2] + 3]
    dims[axis] = 1
    return noise(tuple(dims), seed=50 + axis, share=0.8)


def holed_wall():
    """the geodesic scenes' wall of a label with a one-texel hole, the matter before it of byte 100 and behind it of byte 104: beyond
    the wall every chain goes through the hole, and pays the four bytes once, in the step out of it"""
    dims, vol, lab, kw, closed = GS.wall(False)
    tx = tile()[0]
    wx = tx // 2 + 4
    vol3 = vol.reshape(dims[::-1]).copy()
    vol3[:, :, wx + 1:] = 104
    step, contrast = 2, 5
    steps = closed["keys"] >> 8
    xx = np.indices(dims[::-1])[2]
    keys = np.where(closed["keys"] < 0, -1, (step * steps + np.where(xx > wx, 4 * contrast, 0)) << 8)
    return dims, _flat(vol3), lab, dict(kw, step=step, contrast=contrast), {"keys": keys, "n_reached": closed["n_reached"]}


def constructed():
    """name -> (dims, vol, labels, scene.Cost, closed form): the scenes built about weights, and the edges"""
    from volym_amd import scene
    tx, ty, tz = tile()
    off = ((3, 2, 1), (2 * tx + 4, 2 * ty + 3, 2 * tz + 2))
    made = {"monotone ramp": ramp(), "ridge and detour": ridge(False), "ridge between two labels": ridge(True), "a tile lowered again and again": relowered(),
            "the overflow trap": overflow(), "wall of a label with a hole": holed_wall(),
            "one texel along x": flat(0), "one texel along y": flat(1), "one texel along z": flat(2),
            "a box off the tiles": noise((2 * tx + 7, 2 * ty + 5, 2 * tz + 3), off, share=0.62),
            "a box off the tiles, cost 60": noise((2 * tx + 7, 2 * ty + 5, 2 * tz + 3), off, share=0.62, weights=(2, 9, 60))}
    for axis in range(3):
        for on_face in (True, False):
            made["tied along %s, %s" % ("xyz"[axis], "on a tile face" if on_face else "inside a tile")] = tied(axis, on_face)
    out = {name: (dims, vol, lab, scene.Cost(dims=dims, **kw), closed) for name, (dims, vol, lab, kw, closed) in made.items()}
    # the edges of the geodesic scenes under weights: no seed, seeds without medium, the empty box, the points
    theirs = GS.constructed()
    for k, name in enumerate(("no seed", "no medium", "empty box", "points", "checkerboard")):
        dims, vol, lab, g, closed = theirs[name]
        out[name] = (dims, vol, lab, weighted(g, k + 1), {} if name == "points" else {"n_reached": closed["n_reached"]})     # (no weight changes what these reach)
    return out


def faces_crossed(route):
    """how many steps of a route (a list of texels) go from one tile into another"""
    ext = tile()
    return sum(1 for a, b in zip(route, route[1:]) if tuple(a[i] // ext[i] for i in range(3)) != tuple(b[i] // ext[i] for i in range(3)))


def limit_cases(host=None):
    """(name, unlimited scene.Cost over scene A, [limits]): for each request a limit that is an attained cost and one that falls
    strictly between two attained costs, read off the twin's unlimited map"""
    from volym_amd import scene
    host = host or scene_a()
    out = []
    for name, c in requests()[:6]:
        c = c.replace(max_cost=0)
        _, full = scene.cost_volume(host.vol, host.dims, c, labels=host.labels)
        costs = np.unique(full[full != np.uint32(NONE)] >> 8).astype(np.int64)
        costs = costs[costs > 0]
        if costs.size < 4:
            continue
        gaps = np.flatnonzero(np.diff(costs) > 1)
        limits = [int(costs[costs.size // 2]), int(costs[1])]
        if gaps.size:
            limits.append(int(costs[gaps[gaps.size // 2]]) + 1)
        out.append((name, c, limits))
    return out


def cut_off(full, limit):
    """an unlimited key map cut off at `limit`"""
    return np.where((full != np.uint32(NONE)) & ((full >> 8) > limit), np.uint32(NONE), full)


# ---- the spread's requests over scene A ------------------------------------------------------------------------------------------------
class SpreadCase:
    def __init__(self, name, cost, spread, trivial=False):
        self.name, self.cost, self.spread, self.trivial = name, cost, spread, trivial


def spread_cases():
    """(scene A) a cost request and a spread by it, in the pattern of the geodesic scenes' flood_cases: the unlabelled matter among
    three segments, a band of cost, windows of the cut and the uncut bytes, a box inside the pass's box, a take table that excludes a
    label, a `to` table that renames, a wand from a point, a dry run, a band that excludes everything, a pass without seeds"""
    from volym_amd import scene
    Q, S = scene.Cost, scene.Spread
    whole, part = BOXES["whole"], BOXES["x 5..30"]
    seeds = Q(whole, 0, (1, 255), table(1, 2, 3), table(0, 4), 1, 3)
    bright = Q(whole, 0, (90, 255), table(1, 3, 4), table(0, 2), 2, 17)
    inner = Q(part, 0, (40, 255), table(2, 4), table(0, 1, 3), 1, 5, 400)
    wand = Q(whole, 0, (70, 255), table(), table(0, 1, 2, 3, 4), 1, 2, 600, [(17, 9, 11)])
    return [
        SpreadCase("0 and 4 to the seeds 1, 2, 3", seeds, S(whole, give=table(0, 4), take=table(1, 2, 3))),
        SpreadCase("0 within a cost of 60", seeds, S(whole, give=table(0), take=table(1, 2, 3), cost=(1, 60))),
        SpreadCase("bright medium, window 60..200, rows", bright, S(BOXES["rows"], window=(60, 200), give=table(0, 2), take=table(1, 3, 4))),
        SpreadCase("the uncut bytes, x 3..8", bright, S(BOXES["x 3..8"], SPREAD_UNCUT, (1, 220), table(0, 1, 2), table(3, 4))),
        SpreadCase("a box inside the pass's box", inner, S(((6, 4, 2), (29, 18, 17)), give=table(0, 1, 3), take=table(2, 4), cost=(0, 250))),
        SpreadCase("take excludes the cheapest: the texel stays", seeds, S(whole, give=table(0, 4), take=table(2))),
        SpreadCase("to renames: 1 -> 9, 2 -> 3", seeds, S(whole, give=table(0, 1, 2, 4), take=table(1, 2, 3), to={1: 9, 2: 3}, cost=(0, 90))),
        SpreadCase("a wand from an unlabelled click", wand, S(whole, give=1 - table(), take=table(*range(5)), to={l: 6 for l in range(5)})),
        SpreadCase("dry run", seeds, S(whole, SPREAD_DRY_RUN, give=table(0, 4), take=table(1, 2, 3))),
        SpreadCase("a band that excludes everything", seeds, S(whole, give=table(0, 4), take=table(1, 2, 3), cost=(0, 0)), trivial=True),
        SpreadCase("no label gives", seeds, S(whole, give=table(), take=table(1, 2, 3)), trivial=True),
        SpreadCase("no seed", Q(whole, 0, (1, 255), table(9), table(0, 4), 1, 3), S(whole, give=table(0, 4), take=table(9)), trivial=True),
        SpreadCase("empty box", seeds, S(BOXES["empty"], give=table(0, 4), take=table(1, 2, 3)), trivial=True),
        SpreadCase("single texel", seeds, S(BOXES["texel"], give=table(0, 1, 2, 3, 4), take=table(1, 2, 3), to={1: 2, 2: 3, 3: 1})),
    ]


def spread_expect(host, case, snap=None):
    """the twin's (new_labels [flat], result) of `case` in the state `host` is in; snap: the pass's (summary, keys) where it was taken
    in an earlier state"""
    from volym_amd import scene
    snap = snap or expect(host, case.cost)
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, result = scene.spread_volume(now, host.dims, case.spread, host.labels, snap[1], case.cost.box, uncut=host.vol)
    return new.ravel(), result
