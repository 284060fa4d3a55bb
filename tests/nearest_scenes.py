"""The scenes and requests of the nearest tests, shared by tests/test_nearest_host.py (which pins the host twins to an all-pairs
minimum with lexicographic ties, to the distance twin, to closed forms and to per-texel loops) and tests/test_gpu_nearest.py (which
compares the device with the twins).  Scenes A and B, their boxes and cut states are those of tests/measure_scenes.py, the select
tables, thresholds and long rows those of tests/surface_scenes.py, the weights, the requests and the constructed scenes those of
tests/distance_scenes.py; the scenes built for ties and the fill's requests are built here.
"""
import numpy as np

from tests import distance_scenes as DS
from tests import measure_scenes as M
from tests import surface_scenes as S

DIMS, NX, NY, NZ = M.DIMS, M.NX, M.NY, M.NZ
BOX, PLANE, HIDDEN = M.BOX, M.PLANE, M.HIDDEN
BOXES, CUTS, MIN_BYTES, WEIGHTS = M.BOXES, M.CUTS, S.MIN_BYTES, DS.WEIGHTS
LONG_DIMS, LONG_BOXES = S.LONG_DIMS, S.LONG_BOXES
scene_a, scene_b, selects = M.scene_a, M.scene_b, S.selects
UNCUT, INSIDE = DS.UNCUT, DS.INSIDE
NONE = 0xFFFFFFFF                   # _lib.NEAREST_NONE
FILL_UNCUT, FILL_DRY_RUN = 1, 2     # _lib.FILL_UNCUT, _lib.FILL_DRY_RUN


def requests(flags=0, turn=0):
    """(name, scene.Distance): the distance tests' requests -- every box with a rotating select table, min_byte and the four weights,
    and the whole volume with every select table -- without INSIDE"""
    assert not flags & INSIDE
    return DS.requests(flags, turn)


def expect(host, d, labels=True):
    """the twin's (summary, sites, near_labels) for the state `host` is in; labels False: the context holds no labels of the volume's
    dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.nearest_volume(now, host.dims, d, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 4120 bytes of struct volym_nearest_summary, then the site map, then the label map"""
    summary, sites, near = result
    return summary.tobytes() + np.ascontiguousarray(sites, np.uint32).tobytes() + np.ascontiguousarray(near, np.uint8).tobytes()


def brute_force(solid, label, weight):
    """The rule as an all-pairs minimum: `solid` a bool array and `label` the label bytes, [z, y, x] over the request's box.  Every
    solid texel in turn, in ascending (z, y, x), and only a strictly smaller d2 replaces the best so far: the first of equals stays.
    Returns (sites uint32, near_labels uint8)."""
    depth, h, w = solid.shape
    zz, yy, xx = np.indices(solid.shape)
    best = np.full(solid.shape, np.iinfo(np.int64).max, np.int64)
    sites = np.full(solid.shape, NONE, np.uint32)
    near = np.zeros(solid.shape, np.uint8)
    for z, y, x in np.argwhere(solid).tolist():                      # (argwhere is in ascending (z, y, x))
        d2 = weight[0] * (xx - x) ** 2 + weight[1] * (yy - y) ** 2 + weight[2] * (zz - z) ** 2
        better = d2 < best
        best[better] = d2[better]
        sites[better] = x + w * (y + h * z)
        near[better] = label[z, y, x]
    return sites, near


def summary_by_loops(sites, near, density, label, d):
    """every field of the summary by plain loops over the texels of the box, as a dict"""
    out = {"n_solid": 0, "n_present": 0, "n_finite": 0, "cell": [0] * 256, "cell_present": [0] * 256}
    select = np.asarray(d.select)
    for (z, y, x), s in np.ndenumerate(sites):
        present = int(density[z, y, x]) >= d.min_byte
        solid = present and select[int(label[z, y, x])] != 0
        out["n_present"] += present
        out["n_solid"] += solid
        if int(s) != NONE:
            out["n_finite"] += 1
            out["cell"][int(near[z, y, x])] += 1
            out["cell_present"][int(near[z, y, x])] += present and not solid
    return out


# ---- the scenes built for ties: name -> (dims, vol, labels, request keywords, closed form) -----------------------------------------
# closed form: any of "sites" (the whole site map as int64 [z, y, x]), "near" (the whole label map), "at" ({texel (x, y, z): (site
# texel (x, y, z), label)})
def _flat(a):
    return np.ascontiguousarray(a, np.uint8).ravel()


def _index(dims, x, y, z):
    return x + dims[0] * (y + dims[1] * z)


def mirrored(axis):
    """9 x 7 x 5 with two seeds mirrored about texel (4, 3, 2) along `axis`, labels 1 (the lower) and 2: every texel below the centre's
    plane and ON it goes to the lower seed, the first in (z, y, x)"""
    dims = (9, 7, 5)
    t, k = (4, 3, 2), (3, 2, 2)[axis]
    lo, hi = list(t), list(t)
    lo[axis] -= k
    hi[axis] += k
    vol = np.zeros(dims[::-1], np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    vol[lo[2], lo[1], lo[0]], lab[lo[2], lo[1], lo[0]] = 50, 1
    vol[hi[2], hi[1], hi[0]], lab[hi[2], hi[1], hi[0]] = 50, 2
    along = np.indices(dims[::-1])[2 - axis]
    lower = along <= t[axis]
    return dims, _flat(vol), _flat(lab), {"weight": (9, 4, 25)}, \
        {"sites": np.where(lower, _index(dims, *lo), _index(dims, *hi)), "near": np.where(lower, 1, 2), "at": {t: (tuple(lo), 1)}}


def axis_against_diagonal(which):
    """11 x 9 x 7: two seeds at the same d2 = 4 from texel t = (5, 4, 3), one step along the axis of weight 4 and two steps along an axis
    of weight 1.  The first in (z, y, x) wins t: with weights (4, 1, 1) and offsets (1, 0, 0) against (0, 2, 0) the former, whose y is
    smaller; with (1, 4, 1) and (0, 1, 0) against (2, 0, 0) the latter; with (1, 1, 4) and (0, 0, 1) against (2, 0, 0) the latter"""
    dims, t = (11, 9, 7), (5, 4, 3)
    weight, a, b, first = (((4, 1, 1), (1, 0, 0), (0, 2, 0), 0), ((1, 4, 1), (0, 1, 0), (2, 0, 0), 1), ((1, 1, 4), (0, 0, 1), (2, 0, 0), 1))[which]
    vol = np.zeros(dims[::-1], np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    seeds = [tuple(t[i] + o[i] for i in range(3)) for o in (a, b)]
    for l, (x, y, z) in enumerate(seeds, 1):
        vol[z, y, x], lab[z, y, x] = 9, l
    assert sum(weight[i] * a[i] ** 2 for i in range(3)) == sum(weight[i] * b[i] ** 2 for i in range(3)) == 4
    return dims, _flat(vol), _flat(lab), {"weight": weight}, {"at": {t: (seeds[first], first + 1)}}


def checkerboard(only_one):
    """8 x 6 x 5, labels 1 and 2 on (x + y + z) % 2, every texel present.  Both selected: every site is the texel itself.  Label 1 alone,
    unit weights: a texel of label 2 has up to six neighbours at d2 = 1, and the first in (z, y, x) is the one below (z - 1) where
    there is one"""
    dims = (8, 6, 5)
    zz, yy, xx = np.indices(dims[::-1])
    lab = (1 + (xx + yy + zz) % 2).astype(np.uint8)
    own = _index(dims, xx, yy, zz)
    if not only_one:
        return dims, np.full(lab.size, 77, np.uint8), _flat(lab), {"weight": (1, 4, 9)}, {"sites": own, "near": lab.astype(np.int64)}
    select = np.zeros(256, np.int64)
    select[1] = 1
    at = {(x, y, z): ((x, y, z - 1), 1) for x, y, z in ((3, 2, 2), (4, 4, 1), (1, 0, 4)) if (x + y + z) % 2 == 1}
    at[(1, 0, 0)] = ((0, 0, 0), 1)                     # no z - 1, no y - 1: x - 1
    at[(0, 1, 0)] = ((0, 0, 0), 1)                     # no z - 1: y - 1
    return dims, np.full(lab.size, 77, np.uint8), _flat(lab), {"select": select}, {"near": np.ones(dims[::-1], np.int64), "at": at}


def full_box():
    """9 x 6 x 4, every texel solid with a label of its own kind: every site is the texel itself"""
    dims = (9, 6, 4)
    zz, yy, xx = np.indices(dims[::-1])
    lab = ((xx + 2 * yy + 3 * zz) % 7).astype(np.uint8)
    return dims, np.full(lab.size, 255, np.uint8), _flat(lab), {"weight": (1, 4, 9)}, {"sites": _index(dims, xx, yy, zz), "near": lab.astype(np.int64)}


def empty_set():
    """8 x 5 x 4 with no solid texel: every site is NONE and every label 0"""
    dims = (8, 5, 4)
    return dims, np.zeros(160, np.uint8), np.full(160, 3, np.uint8), {"weight": (1, 4, 9)}, \
        {"sites": np.full(dims[::-1], NONE, np.int64), "near": np.zeros(dims[::-1], np.int64)}


def corner(last):
    """7 x 5 x 6 with one seed, label 9, in the first or the last corner"""
    dims = (7, 5, 6)
    vol = np.zeros(dims[::-1], np.uint8)
    lab = np.zeros(dims[::-1], np.uint8)
    c = (6, 4, 5) if last else (0, 0, 0)
    vol[c[2], c[1], c[0]], lab[c[2], c[1], c[0]] = 1, 9
    return dims, _flat(vol), _flat(lab), {"weight": (25, 1, 4)}, {"sites": np.full(dims[::-1], _index(dims, *c), np.int64), "near": np.full(dims[::-1], 9, np.int64)}


def row_ends(last):
    """distance_scenes.row_ends: seeds only in the last (x = 90) or only in the first (x = 5) chunk of every 97-texel row, each the site
    of its whole row; the label is the row's parity"""
    dims, vol, _, kw, _ = DS.row_ends(last)
    at = 90 if last else 5
    zz, yy, xx = np.indices(dims[::-1])
    lab = (1 + (yy + zz) % 2).astype(np.uint8)
    return dims, vol, _flat(lab), kw, {"sites": _index(dims, at, yy, zz), "near": lab.astype(np.int64)}


def column_end():
    """distance_scenes.column_end: 3 x 70 x 2 whose only seeds are the last entries of the y columns"""
    dims, vol, _, kw, _ = DS.column_end()
    zz, yy, xx = np.indices(dims[::-1])
    lab = (1 + xx).astype(np.uint8)
    return dims, vol, _flat(lab), kw, {"sites": _index(dims, xx, dims[1] - 1, zz), "near": lab.astype(np.int64)}


def flat(axis):
    """an extent of 1 along `axis`, 13 and 11 along the others: random seeds of four labels, weights (4, 9, 1)"""
    dims = [13, 11, 9]
    dims[axis] = 1
    rng = np.random.default_rng(40 + axis)
    n = dims[0] * dims[1] * dims[2]
    return tuple(dims), np.where(rng.random(n) < 0.1, 200, 0).astype(np.uint8), rng.integers(0, 4, n).astype(np.uint8), {"weight": (4, 9, 1)}, {}


def ties():
    """name -> (dims, vol, labels, scene.Distance, closed form): the scenes built for ties"""
    from volym_amd import scene
    made = {"mirrored along x": mirrored(0), "mirrored along y": mirrored(1), "mirrored along z": mirrored(2),
            "axis x against a diagonal": axis_against_diagonal(0), "axis y against a diagonal": axis_against_diagonal(1),
            "axis z against a diagonal": axis_against_diagonal(2), "checkerboard": checkerboard(False), "checkerboard, one label": checkerboard(True),
            "full box": full_box(), "empty set": empty_set(), "first corner": corner(False), "last corner": corner(True),
            "seeds in the last chunk": row_ends(True), "seeds in the first chunk": row_ends(False), "column end": column_end(),
            "one texel along x": flat(0), "one texel along y": flat(1), "one texel along z": flat(2)}
    return {name: (dims, vol, lab, scene.Distance(dims=dims, **kw), closed) for name, (dims, vol, lab, kw, closed) in made.items()}


def constructed():
    """the tie scenes, and the distance tests' constructed scenes that have no INSIDE (closed form: d2 to the site is their map)"""
    out = dict(ties())
    for name, (dims, vol, lab, d, closed) in DS.constructed().items():
        if not d.flags & INSIDE and name not in out:
            out["distance: " + name] = (dims, vol, lab, d, {"d2": closed["map"]} if "map" in closed else {})
    return out


def check_closed(name, result, closed, d):
    """a (summary, sites, near_labels) against the closed form of a constructed scene"""
    from volym_amd import scene
    summary, sites, near = result
    dims = tuple(b - a for a, b in zip(*d.box))
    if "sites" in closed:
        assert np.array_equal(sites.astype(np.int64), closed["sites"]), name
    if "near" in closed:
        assert np.array_equal(near.astype(np.int64), closed["near"]), name
    if "d2" in closed:
        assert np.array_equal(scene.nearest_d2(sites, d.box, d.weight), closed["d2"]), name
    for (x, y, z), (s, l) in closed.get("at", {}).items():
        assert int(sites[z, y, x]) == _index(dims, *s) and int(near[z, y, x]) == l, (name, (x, y, z), int(sites[z, y, x]), int(near[z, y, x]))
    assert int(summary["cell"].sum()) == int(summary["n_finite"]) == (sites.size if int(summary["n_solid"]) else 0), name


# ---- the fill's requests over scene A -------------------------------------------------------------------------------------------------
def table(*labels):
    t = np.zeros(256, np.int64)
    t[list(labels)] = 1
    return t


class FillCase:
    def __init__(self, name, distance, fill, trivial=False):
        self.name, self.distance, self.fill, self.trivial = name, distance, fill, trivial


def fill_cases():
    """(scene A) a nearest request and a fill by it: the unlabelled matter split among three segments, a band, a window of the cut and
    of the uncut bytes, a box inside the pass's box, a take table that excludes a seed, a dry run, a band that excludes everything, a
    pass without solid texels"""
    from volym_amd import scene
    D, F = scene.Distance, scene.Fill
    whole, part = BOXES["whole"], BOXES["x 5..30"]
    seeds = D(whole, 0, 1, table(1, 2, 3), (1, 1, 1))
    bright = D(whole, 0, 140, table(1, 3, 4), (1, 4, 9))
    inner = D(part, 0, 60, table(2, 4), (4, 1, 1))
    return [
        FillCase("0 and 4 to the nearest of 1, 2, 3", seeds, F(whole, give=table(0, 4), take=table(1, 2, 3))),
        FillCase("0 within 2 of a seed", seeds, F(whole, give=table(0), take=table(1, 2, 3), d2=(1, 4))),
        FillCase("bright seeds, window 60..200, rows", bright, F(BOXES["rows"], window=(60, 200), give=table(0, 2), take=table(1, 3, 4))),
        FillCase("the uncut bytes, x 3..8", bright, F(BOXES["x 3..8"], FILL_UNCUT, (1, 120), table(0, 1, 2), table(3, 4))),
        FillCase("a box inside the pass's box", inner, F(((6, 4, 2), (29, 18, 17)), give=table(0, 1, 3), take=table(2, 4), d2=(0, 36))),
        FillCase("take excludes the nearest: the texel stays", seeds, F(whole, give=table(0, 4), take=table(2))),
        FillCase("seeds give too", seeds, F(whole, give=table(0, 1, 2, 3, 4), take=table(1, 2, 3), d2=(0, 9))),
        FillCase("dry run", seeds, F(whole, FILL_DRY_RUN, give=table(0, 4), take=table(1, 2, 3))),
        FillCase("a band that excludes everything", seeds, F(whole, give=table(0, 4), take=table(1, 2, 3), d2=(0, 0)), trivial=True),
        FillCase("no label gives", seeds, F(whole, give=table(), take=table(1, 2, 3)), trivial=True),
        FillCase("no solid texel", D(whole, 0, 1, table(9)), F(whole, give=table(0, 4), take=table(9)), trivial=True),
        FillCase("empty box", seeds, F(BOXES["empty"], give=table(0, 4), take=table(1, 2, 3)), trivial=True),
        FillCase("single texel", seeds, F(BOXES["texel"], give=table(0, 1, 2, 3, 4), take=table(1, 2, 3))),
    ]


def fill_expect(host, case, snap=None):
    """the twin's (new_labels [flat], result) of `case` in the state `host` is in; snap: the pass's (summary, sites, near_labels) where
    it was taken in an earlier state"""
    from volym_amd import scene
    snap = snap or expect(host, case.distance)
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, result = scene.fill_volume(now, host.dims, case.fill, host.labels, snap[1], snap[2], case.distance.box, case.distance.weight, uncut=host.vol)
    return new.ravel(), result


# ---- two touching balls ---------------------------------------------------------------------------------------------------------------
def two_balls(apart=9):
    """30 x 16 x 16: two balls of radius 6 round (10, 8, 8) and (10 + apart, 8, 8), one segment (label 1) of density 200 in air:
    (dims, vol, labels).  9 apart the mid-plane x = 14.5 holds no texel; 10 apart it is x = 15"""
    dims = (30, 16, 16)
    zz, yy, xx = np.indices(dims[::-1])
    solid = np.zeros(dims[::-1], bool)
    for cx in (10, 10 + apart):
        solid |= (xx - cx) ** 2 + (yy - 8) ** 2 + (zz - 8) ** 2 <= 36
    return dims, _flat(np.where(solid, 200, 0)), _flat(solid)
