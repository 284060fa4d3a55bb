"""The scenes and requests of the geodesic tests, shared by tests/test_geodesic_host.py (which pins the host twins to a per-label
breadth-first search, to a restatement of the device's schedule, to closed forms and to per-texel loops) and
tests/test_gpu_geodesic.py (which compares the device with the twins).  Scenes A and B, their boxes and cut states are those of
tests/measure_scenes.py, the long rows those of tests/surface_scenes.py, the serpentine that of tests/components_scenes.py; the
scenes built for walls, ties, tiles and points and the flood's requests are built here.  The tile's extents are read from
volym_amd/csrc/geodesic_kernels.h, so that the scenes built about tile faces follow them.
"""
import os
import re

import numpy as np

from tests import components_scenes as CS
from tests import measure_scenes as M
from tests import surface_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, NX, NY, NZ = M.DIMS, M.NX, M.NY, M.NZ
BOX, PLANE, HIDDEN = M.BOX, M.PLANE, M.HIDDEN
BOXES, CUTS = M.BOXES, M.CUTS
LONG_DIMS, LONG_BOXES = S.LONG_DIMS, S.LONG_BOXES
scene_a, scene_b = M.scene_a, M.scene_b
NONE = 0xFFFFFFFF                   # _lib.GEODESIC_NONE
UNCUT = 1                           # _lib.GEODESIC_UNCUT
FLOOD_UNCUT, FLOOD_DRY_RUN = 1, 2   # _lib.FLOOD_UNCUT, _lib.FLOOD_DRY_RUN


def tile():
    """(TX, TY, TZ) of volym_amd/csrc/geodesic_kernels.h"""
    text = open(os.path.join(ROOT, "volym_amd", "csrc", "geodesic_kernels.h")).read()
    m = re.search(r"constexpr uint32_t GEO_TX = (\d+)u, GEO_TY = (\d+)u, GEO_TZ = (\d+)u;", text)
    assert m, "geodesic_kernels.h names the tile's extents"
    return tuple(int(v) for v in m.groups())


def table(*labels):
    t = np.zeros(256, np.int64)
    t[list(labels)] = 1
    return t


def _flat(a):
    return np.ascontiguousarray(a, np.uint8).ravel()


# ---- requests over scenes A and B ------------------------------------------------------------------------------------------------------
TABLES = [(table(1, 2, 3), table(0, 4)), (table(2), table(0, 1, 3, 4)), (1 - table(0), table(0)), (table(0), table(1, 2, 3, 4)),
          (table(*range(0, 256, 5)), table(*range(1, 256, 2)))]
WINDOWS = [(1, 255), (60, 255), (0, 140), (100, 200)]
LIMITS = [0, 0, 3, 1, 12]


def requests(flags=0, turn=0):
    """(name, scene.Geodesic): every box with a rotating pair of tables, window and step limit, and the whole volume with every pair"""
    from volym_amd import scene
    out = []
    for k, (b, box) in enumerate(BOXES.items()):
        seed, through = TABLES[(k + turn) % len(TABLES)]
        out.append(("%s / tables %d" % (b, (k + turn) % len(TABLES)),
                    scene.Geodesic(box, flags, WINDOWS[(k + turn) % len(WINDOWS)], seed, through, LIMITS[(k + 2 * turn) % len(LIMITS)])))
    for k, (seed, through) in enumerate(TABLES):
        out.append(("whole / tables %d" % k, scene.Geodesic(BOXES["whole"], flags, WINDOWS[(k + turn + 1) % len(WINDOWS)], seed, through, LIMITS[(k + turn) % len(LIMITS)])))
    return out


def expect(host, g, labels=True):
    """the twin's (summary, keys) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.geodesic_volume(now, host.dims, g, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 6184 bytes of struct volym_geodesic_summary, then the key map"""
    summary, keys = result
    return summary.tobytes() + np.ascontiguousarray(keys, np.uint32).tobytes()


# ---- the rule restated ---------------------------------------------------------------------------------------------------------------
def predicates(density, label, g):
    """(seed, medium, label) over the request's box: bool arrays [z, y, x] from the density and label bytes of that box"""
    lo = g.box[0]
    window = (density >= g.window[0]) & (density <= g.window[1])
    seed = window & (np.asarray(g.seed)[label] != 0)
    for p in g.points:
        seed[p[2] - lo[2], p[1] - lo[1], p[0] - lo[0]] = True
    return seed, window & (np.asarray(g.through)[label] != 0)


def brute_force(seed, medium, label, max_steps=0):
    """The rule label by label: a breadth-first search with a queue from the seeds of one label at a time, texel by texel; steps is
    the smallest of the searches' distances and geo_label the smallest label that attains it.  Returns (keys as int64 with -1 for
    NONE, ties): ties counts the texels at which two labels or more attain the distance."""
    depth, h, w = seed.shape
    best = np.full(seed.shape, -1, np.int64)
    winner = np.zeros(seed.shape, np.int64)
    tied = np.zeros(seed.shape, bool)
    for l in sorted(set(label[seed].tolist())):
        dist = np.full(seed.shape, -1, np.int64)
        queue = [tuple(t) for t in np.argwhere(seed & (label == l)).tolist()]
        for t in queue:
            dist[t] = 0
        head = 0
        while head < len(queue):
            z, y, x = queue[head]
            head += 1
            for dz, dy, dx in ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
                u = (z + dz, y + dy, x + dx)
                if 0 <= u[0] < depth and 0 <= u[1] < h and 0 <= u[2] < w and dist[u] < 0 and medium[u] and not seed[u]:
                    dist[u] = dist[z, y, x] + 1
                    queue.append(u)
        reached = dist >= 0
        tied |= reached & (best == dist)
        better = reached & ((best < 0) | (dist < best))           # (labels ascend: an equal distance keeps the smaller label)
        tied &= ~better
        best[better] = dist[better]
        winner[better] = l
    if max_steps:
        best[best > max_steps] = -1
    return np.where(best >= 0, best << 8 | winner, -1), int((tied & (best >= 0)).sum())


def scheduled(seed, medium, label, max_steps, tiles, rng):
    """The device's schedule restated: the keys start as the label on a seed, OPEN on the medium and NONE elsewhere; tiles of
    `tiles` = (tx, ty, tz) texels are relaxed one at a time, in a random order, each to its own fixed point against a halo read once,
    and a tile that lowered a word marks its six neighbours; until no tile is marked.  Returns the keys as int64, -1 for NONE."""
    none, open_ = 1 << 40, (1 << 40) - 1
    limit = (max_steps or 0xFFFFFD) << 8 | 0xFF
    depth, h, w = seed.shape
    key = np.where(seed, label.astype(np.int64), np.where(medium, open_, none))
    tx, ty, tz = tiles
    grid = [(k, j, i) for k in range(0, depth, tz) for j in range(0, h, ty) for i in range(0, w, tx)]
    marked = set(grid)
    while marked:
        order = sorted(marked)
        rng.shuffle(order)
        nxt = set()
        stale = key.copy()                                          # a tile's halo is as old as the round's beginning, or fresher
        for k, j, i in order:
            pad = np.full((tz + 2, ty + 2, tx + 2), none, np.int64)
            for dz in range(-1, tz + 1):
                for dy in range(-1, ty + 1):
                    for dx in range(-1, tx + 1):
                        z, y, x = k + dz, j + dy, i + dx
                        if 0 <= z < depth and 0 <= y < h and 0 <= x < w:
                            inside = 0 <= dz < tz and 0 <= dy < ty and 0 <= dx < tx
                            pad[dz + 1, dy + 1, dx + 1] = key[z, y, x] if inside or rng.random() < 0.5 else stale[z, y, x]
            lowered = False
            while True:
                c = pad[1:-1, 1:-1, 1:-1]
                m = np.minimum.reduce([pad[1:-1, 1:-1, :-2], pad[1:-1, 1:-1, 2:], pad[1:-1, :-2, 1:-1], pad[1:-1, 2:, 1:-1], pad[:-2, 1:-1, 1:-1], pad[2:, 1:-1, 1:-1]])
                cand = m + 256
                take = (c != none) & (m < open_) & (cand <= limit) & (cand < c)
                if not take.any():
                    break
                c[take] = cand[take]
                lowered = True
            if lowered:
                zs, ys, xs = slice(k, min(k + tz, depth)), slice(j, min(j + ty, h)), slice(i, min(i + tx, w))
                key[zs, ys, xs] = pad[1:-1, 1:-1, 1:-1][:zs.stop - k, :ys.stop - j, :xs.stop - i]
                for dz, dy, dx in ((0, 0, tx), (0, 0, -tx), (0, ty, 0), (0, -ty, 0), (tz, 0, 0), (-tz, 0, 0)):
                    t = (k + dz, j + dy, i + dx)
                    if 0 <= t[0] < depth and 0 <= t[1] < h and 0 <= t[2] < w:
                        nxt.add(t)
        marked = nxt
    return np.where(key < open_, key, -1)


def summary_by_loops(keys, seed, medium, lo):
    """every field of the summary by plain loops over the texels of the box, as a dict"""
    out = {"n_seed": 0, "n_medium": 0, "n_reached": 0, "max_steps": NONE, "max_at": [0, 0, 0], "cell": [0] * 256, "cell_medium": [0] * 256, "hist": [0] * 256}
    most = -1
    for (z, y, x), k in np.ndenumerate(keys):
        out["n_seed"] += bool(seed[z, y, x])
        out["n_medium"] += bool(medium[z, y, x]) and not seed[z, y, x]
        if int(k) == NONE:
            continue
        steps, l = int(k) >> 8, int(k) & 0xFF
        out["n_reached"] += 1
        out["cell"][l] += 1
        out["cell_medium"][l] += not seed[z, y, x]
        out["hist"][min(steps, 255)] += 1
        if steps > most:                                           # (ndenumerate ascends in (z, y, x): the first of the largest stays)
            most, out["max_steps"], out["max_at"] = steps, steps, [lo[0] + x, lo[1] + y, lo[2] + z]
    return out


# ---- the constructed scenes: name -> (dims, vol, labels, request keywords, closed form) ------------------------------------------------
# closed form: any of "keys" (the whole map as int64 [z, y, x], -1 for NONE), "at" ({texel (x, y, z): (steps, label) or None}),
# "max_at", "n_reached"
def _manhattan(dims, t):
    zz, yy, xx = np.indices(dims[::-1])
    return np.abs(xx - t[0]) + np.abs(yy - t[1]) + np.abs(zz - t[2])


def open_box(last):
    """a box of matter larger than a tile on every axis, one seed point in the first or the last corner: steps = |dx| + |dy| + |dz|"""
    tx, ty, tz = tile()
    dims = (tx + 5, ty + 3, tz + 2)
    c = tuple(v - 1 for v in dims) if last else (0, 0, 0)
    far = (0, 0, 0) if last else tuple(v - 1 for v in dims)
    n = dims[0] * dims[1] * dims[2]
    return dims, np.full(n, 100, np.uint8), np.zeros(n, np.uint8), {"seed": table(), "points": [c]}, \
        {"keys": _manhattan(dims, c) << 8, "max_at": far, "n_reached": n}


def serpentine_path():
    """the texels (x, y, z) of components_scenes.serpentine() in the order of the path, from (0, 0, 0)"""
    (w, h, d), vol, _, _, _ = CS.serpentine()
    solid = vol.reshape(d, h, w) != 0
    path, seen = [(0, 0, 0)], {(0, 0, 0)}
    while True:
        x, y, z = path[-1]
        nxt = [t for t in ((x + 1, y, z), (x - 1, y, z), (x, y + 1, z), (x, y - 1, z), (x, y, z + 1), (x, y, z - 1))
               if 0 <= t[0] < w and 0 <= t[1] < h and 0 <= t[2] < d and solid[t[2], t[1], t[0]] and t not in seen]
        if not nxt:
            return path
        assert len(nxt) == 1, "the serpentine is one path"
        path.append(nxt[0])
        seen.add(nxt[0])


def serpentine(max_steps=0):
    """one path of 1339 texels through 66 x 9 x 7, seeded at (0, 0, 0): steps = the position along the path, cut at max_steps"""
    dims, vol, lab, _, _ = CS.serpentine()
    path = serpentine_path()
    keys = np.full(dims[::-1], -1, np.int64)
    for k, (x, y, z) in enumerate(path):
        if not max_steps or k <= max_steps:
            keys[z, y, x] = k << 8
    last = min(max_steps or len(path) - 1, len(path) - 1)
    return dims, vol, lab, {"seed": table(), "points": [(0, 0, 0)], "max_steps": max_steps}, {"keys": keys, "max_at": path[last], "n_reached": last + 1}


def checkerboard():
    """13 x 10 x 9 of matter on (x + y + z) % 2 == 0 alone, three of those texels seeds of label 3: diagonal contact does not connect"""
    dims = (13, 10, 9)
    zz, yy, xx = np.indices(dims[::-1])
    vol = np.where((xx + yy + zz) % 2 == 0, 200, 0)
    lab = np.zeros(dims[::-1], np.uint8)
    keys = np.full(dims[::-1], -1, np.int64)
    for x, y, z in ((0, 0, 0), (5, 4, 3), (12, 9, 7)):
        lab[z, y, x] = 3
        keys[z, y, x] = 3
    return dims, _flat(vol), _flat(lab), {"seed": table(3)}, {"keys": keys, "n_reached": 3}


def wall(by_density):
    """a wall across x with a one-texel hole, made of a label that is not `through` or of a density outside the window: beyond it
    every chain goes through the hole"""
    tx, ty, tz = tile()
    dims = (tx + 8, ty + 4, tz + 4)
    wx, hole, s = tx // 2 + 4, (tx // 2 + 4, 5, 6), (2, 3, 4)
    vol = np.full(dims[::-1], 100, np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    if by_density:
        vol[:, :, wx] = 10
        vol[hole[2], hole[1], hole[0]] = 100
    else:
        lab[:, :, wx] = 7
        lab[hole[2], hole[1], hole[0]] = 0
    zz, yy, xx = np.indices(dims[::-1])
    direct, through = _manhattan(dims, s), sum(abs(a - b) for a, b in zip(s, hole)) + _manhattan(dims, hole)
    keys = np.where(xx < wx, direct, through) << 8
    keys[:, :, wx] = -1
    keys[hole[2], hole[1], hole[0]] = through[hole[2], hole[1], hole[0]] << 8
    return dims, _flat(vol), _flat(lab), {"seed": table(), "through": table(0), "window": (50, 255), "points": [s]}, \
        {"keys": keys, "n_reached": int((keys >= 0).sum())}


def mirrored(axis, on_face):
    """matter everywhere, two seeds of labels 5 (the lower) and 3 mirrored about texel t along `axis`: the plane of t is tied, and 3
    wins it.  t lies on a tile face (the first texel of the second tile) or in a tile's interior"""
    ext = tile()
    dims = (ext[0] + 9, ext[1] + 11, ext[2] + 10)
    t = [ext[0] // 2 - 1, ext[1] // 2, ext[2] // 2]
    t[axis] = ext[axis] if on_face else ext[axis] // 2
    k = 3
    lo, hi = list(t), list(t)
    lo[axis] -= k
    hi[axis] += k
    vol = np.full(dims[::-1], 90, np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    lab[lo[2], lo[1], lo[0]], lab[hi[2], hi[1], hi[0]] = 5, 3
    along = np.indices(dims[::-1])[2 - axis]
    steps = np.minimum(_manhattan(dims, lo), _manhattan(dims, hi))
    keys = steps << 8 | np.where(along < t[axis], 5, 3)
    return dims, _flat(vol), _flat(lab), {"seed": table(3, 5)}, {"keys": keys, "at": {tuple(t): (k, 3)}}


def late_route():
    """A long winding route inside few tiles and a shorter straight one across many, to one target T.  The winding route: the plane
    z = zt, x-lines on y = 0, 2, 4, 6 joined at alternating ends, from the seed of label 2 at (0, 0, zt) to T = (0, 6, zt).  The
    straight one: the column (0, 6, 0 .. zt) from the seed of label 9 at (0, 6, 0).  T's tile converges by the winding route rounds
    before the straight one arrives, and is then lowered and re-propagated.  Returns the scene and, in its closed form, the two routes
    as texel lists."""
    tx, ty, tz = tile()
    w, h = tx + 8, 8
    zt = 17 * tz + 4
    dims = (w, h, zt + 4)
    vol = np.zeros(dims[::-1], np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    winding, x = [], 0
    for yi, y in enumerate((0, 2, 4, 6)):
        xs = list(range(w)) if x == 0 else list(range(w - 1, -1, -1))
        winding += [(v, y, zt) for v in xs]
        x = xs[-1]
        if y < 6:
            winding.append((x, y + 1, zt))
    straight = [(0, 6, z) for z in range(zt + 1)]
    assert winding[-1] == straight[-1] == (0, 6, zt)
    for x, y, z in winding + straight:
        vol[z, y, x] = 150
    lab[zt, 0, 0], lab[0, 6, 0] = 2, 9
    return dims, _flat(vol), _flat(lab), {"seed": table(2, 9)}, {"at": {(0, 6, zt): (zt, 9)}, "winding": winding, "straight": straight}


def faces_crossed(route):
    """how many steps of a route (a list of texels) go from one tile into another"""
    ext = tile()
    return sum(1 for a, b in zip(route, route[1:]) if tuple(a[i] // ext[i] for i in range(3)) != tuple(b[i] // ext[i] for i in range(3)))


def no_seed():
    dims = (9, 6, 5)
    return dims, np.full(270, 80, np.uint8), np.zeros(270, np.uint8), {}, {"keys": np.full(dims[::-1], -1, np.int64), "n_reached": 0, "max_at": (0, 0, 0)}


def no_medium():
    """seeds of label 4 in every third texel, no medium: only the seeds are reached"""
    dims = (10, 7, 4)
    lab = np.where(np.arange(280) % 3 == 0, 4, 1).astype(np.uint8)
    return dims, np.full(280, 80, np.uint8), lab, {"seed": table(4), "through": table(0)}, \
        {"keys": np.where(lab.reshape(dims[::-1]) == 4, 4, -1).astype(np.int64), "n_reached": int((lab == 4).sum())}


def empty_box():
    dims = (9, 6, 5)
    return dims, np.full(270, 80, np.uint8), np.zeros(270, np.uint8), {"box": ((3, 2, 1), (3, 5, 4))}, {"n_reached": 0}


def noise(dims, box=None, seed=7, share=0.7, max_steps=0):
    """random matter (`share` of the texels) with labels 0..3, seeds 1 and 2 through 0 and 3"""
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    kw = {"seed": table(1, 2), "through": table(0, 3), "max_steps": max_steps}
    if box is not None:
        kw["box"] = box
    return dims, np.where(rng.random(n) < share, 200, 0).astype(np.uint8), rng.choice([0, 0, 0, 0, 0, 3, 3, 1, 2], n).astype(np.uint8), kw, {}


def flat(axis):
    """an extent of 1 along `axis`, more than a tile along the others"""
    ext = tile()
    dims = [ext[0] + 5, ext[1] + 6, ext[2] + 3]
    dims[axis] = 1
    return noise(tuple(dims), seed=50 + axis, share=0.8)


def points():
    """Points: a duplicate, one on a wall (neither medium nor of a seed label: a seed all the same, with the wall's label), one
    beside labelled seeds"""
    tx, ty, tz = tile()
    dims = (tx + 6, ty + 2, tz + 1)
    vol = np.full(dims[::-1], 120, np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    lab[:, :, 20] = 7                                              # the wall, closed
    lab[2, 3, 4] = 1                                               # a labelled seed
    kw = {"seed": table(1), "through": table(0), "points": [(30, 5, 5), (30, 5, 5), (20, 4, 4), (5, 3, 2)]}
    zz, yy, xx = np.indices(dims[::-1])
    left = np.minimum(_manhattan(dims, (4, 3, 2)) << 8 | 1, np.minimum(_manhattan(dims, (5, 3, 2)) << 8, (_manhattan(dims, (20, 4, 4)) << 8) | 7))
    right = np.minimum(_manhattan(dims, (30, 5, 5)) << 8, (_manhattan(dims, (20, 4, 4)) << 8) | 7)
    keys = np.where(xx < 20, left, right)
    keys[:, :, 20] = -1
    keys[4, 4, 20] = 7
    return dims, _flat(vol), _flat(lab), kw, {"keys": keys, "at": {(20, 4, 4): (0, 7), (30, 5, 5): (0, 0), (21, 4, 4): (1, 7), (19, 4, 4): (1, 7)}}


def constructed():
    """name -> (dims, vol, labels, scene.Geodesic, closed form)"""
    from volym_amd import scene
    tx, ty, tz = tile()
    made = {"open box from the first corner": open_box(False), "open box from the last corner": open_box(True),
            "serpentine": serpentine(), "serpentine cut in the middle": serpentine(669), "serpentine, one step": serpentine(1),
            "checkerboard": checkerboard(), "wall of a label with a hole": wall(False), "wall of the window with a hole": wall(True),
            "late shorter route": late_route(), "no seed": no_seed(), "no medium": no_medium(), "empty box": empty_box(), "points": points(),
            "one texel along x": flat(0), "one texel along y": flat(1), "one texel along z": flat(2),
            "a box off the tiles": noise((2 * tx + 7, 2 * ty + 5, 2 * tz + 3), ((3, 2, 1), (2 * tx + 4, 2 * ty + 3, 2 * tz + 2)), share=0.62),
            "a box off the tiles, 5 steps": noise((2 * tx + 7, 2 * ty + 5, 2 * tz + 3), ((3, 2, 1), (2 * tx + 4, 2 * ty + 3, 2 * tz + 2)), share=0.62, max_steps=5)}
    for axis in range(3):
        for on_face in (True, False):
            made["mirrored along %s, %s" % ("xyz"[axis], "on a tile face" if on_face else "inside a tile")] = mirrored(axis, on_face)
    return {name: (dims, vol, lab, scene.Geodesic(dims=dims, **kw), closed) for name, (dims, vol, lab, kw, closed) in made.items()}


def check_closed(name, result, closed):
    """a (summary, keys) against the closed form of a constructed scene"""
    summary, keys = result
    signed = np.where(keys == np.uint32(NONE), -1, keys.astype(np.int64))
    if "keys" in closed:
        bad = np.argwhere(signed != closed["keys"])
        assert bad.size == 0, (name, len(bad), bad[:4].tolist(), signed[signed != closed["keys"]][:4].tolist(), closed["keys"][signed != closed["keys"]][:4].tolist())
    for (x, y, z), want in closed.get("at", {}).items():
        k = int(signed[z, y, x])
        assert (None if k < 0 else (k >> 8, k & 0xFF)) == want, (name, (x, y, z), k, want)
    if "n_reached" in closed:
        assert int(summary["n_reached"]) == closed["n_reached"], (name, int(summary["n_reached"]))
    if "max_at" in closed:
        assert tuple(int(v) for v in summary["max_at"]) == tuple(closed["max_at"]), (name, summary["max_at"])
    assert int(summary["cell"].sum()) == int(summary["hist"].sum()) == int(summary["n_reached"]) == int((signed >= 0).sum()), name


# ---- the flood's requests over scene A -------------------------------------------------------------------------------------------------
class FloodCase:
    def __init__(self, name, geodesic, flood, trivial=False):
        self.name, self.geodesic, self.flood, self.trivial = name, geodesic, flood, trivial


def flood_cases():
    """(scene A) a geodesic request and a flood by it: the unlabelled matter among three segments, a band, windows of the cut and the
    uncut bytes, a box inside the pass's box, a take table that excludes a label, a `to` table that renames, a wand from a point, a
    dry run, a band that excludes everything, a pass without seeds"""
    from volym_amd import scene
    G, F = scene.Geodesic, scene.Flood
    whole, part = BOXES["whole"], BOXES["x 5..30"]
    seeds = G(whole, 0, (1, 255), table(1, 2, 3), table(0, 4))
    bright = G(whole, 0, (90, 255), table(1, 3, 4), table(0, 2))
    inner = G(part, 0, (40, 255), table(2, 4), table(0, 1, 3), 6)
    wand = G(whole, 0, (70, 255), table(), table(0, 1, 2, 3, 4), 0, [(17, 9, 11)])
    return [
        FloodCase("0 and 4 to the seeds 1, 2, 3", seeds, F(whole, give=table(0, 4), take=table(1, 2, 3))),
        FloodCase("0 within 2 steps of a seed", seeds, F(whole, give=table(0), take=table(1, 2, 3), steps=(1, 2))),
        FloodCase("bright medium, window 60..200, rows", bright, F(BOXES["rows"], window=(60, 200), give=table(0, 2), take=table(1, 3, 4))),
        FloodCase("the uncut bytes, x 3..8", bright, F(BOXES["x 3..8"], FLOOD_UNCUT, (1, 220), table(0, 1, 2), table(3, 4))),
        FloodCase("a box inside the pass's box", inner, F(((6, 4, 2), (29, 18, 17)), give=table(0, 1, 3), take=table(2, 4), steps=(0, 4))),
        FloodCase("take excludes the nearest: the texel stays", seeds, F(whole, give=table(0, 4), take=table(2))),
        FloodCase("to renames: 1 -> 9, 2 -> 3", seeds, F(whole, give=table(0, 1, 2, 4), take=table(1, 2, 3), to={1: 9, 2: 3}, steps=(0, 3))),
        FloodCase("a wand from an unlabelled click", wand, F(whole, give=1 - table(), take=table(*range(5)), to={l: 6 for l in range(5)})),
        FloodCase("dry run", seeds, F(whole, FLOOD_DRY_RUN, give=table(0, 4), take=table(1, 2, 3))),
        FloodCase("a band that excludes everything", seeds, F(whole, give=table(0, 4), take=table(1, 2, 3), steps=(0, 0)), trivial=True),
        FloodCase("no label gives", seeds, F(whole, give=table(), take=table(1, 2, 3)), trivial=True),
        FloodCase("no seed", G(whole, 0, (1, 255), table(9), table(0, 4)), F(whole, give=table(0, 4), take=table(9)), trivial=True),
        FloodCase("empty box", seeds, F(BOXES["empty"], give=table(0, 4), take=table(1, 2, 3)), trivial=True),
        FloodCase("single texel", seeds, F(BOXES["texel"], give=table(0, 1, 2, 3, 4), take=table(1, 2, 3), to={1: 2, 2: 3, 3: 1})),
    ]


def flood_expect(host, case, snap=None):
    """the twin's (new_labels [flat], result) of `case` in the state `host` is in; snap: the pass's (summary, keys) where it was taken
    in an earlier state"""
    from volym_amd import scene
    snap = snap or expect(host, case.geodesic)
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, result = scene.flood_volume(now, host.dims, case.flood, host.labels, snap[1], case.geodesic.box, uncut=host.vol)
    return new.ravel(), result
