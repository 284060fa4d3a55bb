"""The scenes and requests of the distance tests, shared by tests/test_distance_host.py (which pins the host twin to a brute-force
all-pairs minimum, to scipy and to the closed forms below) and tests/test_gpu_distance.py (which compares the device with the twin).
Scenes A and B, their boxes and cut states are those of tests/measure_scenes.py, the select tables, thresholds and long rows those of
tests/surface_scenes.py; the constructed scenes are built here.
"""
import numpy as np

from tests import measure_scenes as M
from tests import surface_scenes as S

DIMS, NX, NY, NZ = M.DIMS, M.NX, M.NY, M.NZ
BOX, PLANE, HIDDEN = M.BOX, M.PLANE, M.HIDDEN
BOXES, CUTS, MIN_BYTES = M.BOXES, M.CUTS, S.MIN_BYTES
LONG_DIMS, LONG_BOXES = S.LONG_DIMS, S.LONG_BOXES
scene_a, scene_b, selects = M.scene_a, M.scene_b, S.selects
UNCUT, INSIDE = 1, 2                # _lib.DISTANCE_UNCUT, _lib.DISTANCE_INSIDE
NONE = 0xFFFFFFFF                   # _lib.DISTANCE_NONE
WEIGHTS = ((1, 1, 1), (1, 4, 25), (64, 1, 9), (25, 64, 4))


def requests(flags=0, turn=0):
    """(name, scene.Distance): every box with a rotating select table, min_byte and weights (`turn` shifts the rotation), and the
    whole volume with every select table"""
    from volym_amd import scene
    sel = selects()
    names = ("mix", "all", "one")
    out = []
    for k, (b, box) in enumerate(BOXES.items()):
        k += turn
        n, m, w = names[k % 3], MIN_BYTES[(k // 2) % 3], WEIGHTS[k % 4]
        out.append(("%s / %s / %d / %r" % (b, n, m, w), scene.Distance(box, flags, m, sel[n], w)))
    out += [("whole / %s / 128" % n, scene.Distance(BOXES["whole"], flags, 128, sel[n], WEIGHTS[(k + turn) % 4])) for k, n in enumerate(sel)]
    return out


def expect(host, d, labels=True):
    """the twin's (summary, map) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.distance_volume(now, host.dims, d, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 6184 bytes of struct volym_distance_summary, then the map"""
    summary, dmap = result
    return summary.tobytes() + np.ascontiguousarray(dmap, np.uint32).tobytes()


def brute_force(solid, weight, inside):
    """The rule as an all-pairs minimum: `solid` a bool array [z, y, x] over the request's box.  Every seed in turn; with INSIDE the
    seeds are the texels that are not solid, those of a shell of one texel round the box included (the nearest texel outside the
    box is the axis-aligned one, which lies in that shell).  Returns D as uint32 [z, y, x]."""
    seeds = np.pad(~solid, 1, constant_values=True) if inside else np.pad(solid, 1)
    zz, yy, xx = np.indices(solid.shape)
    best = np.full(solid.shape, NONE, np.int64)
    for z, y, x in (np.argwhere(seeds) - 1).tolist():
        np.minimum(best, weight[0] * (xx - x) ** 2 + weight[1] * (yy - y) ** 2 + weight[2] * (zz - z) ** 2, out=best)
    return best.astype(np.uint32)


# ---- the constructed scenes: name -> (dims, vol, labels, request keywords, closed form) ---------------------------------------------
# closed form: any of "map" (the whole of D as int64 [z, y, x]), "max_d2", "max_at", "near" ({label: d2}), "n_finite", "bins"
# ({bin: count} of the histogram, the bins named only)
def _flat(a):
    return np.ascontiguousarray(a, np.uint8).ravel()


def single_texel():
    """11 x 9 x 7 with one solid texel at (7, 2, 5), weights (4, 1, 25): D is the weighted d2 to it"""
    w, h, d = 11, 9, 7
    vol = np.zeros((d, h, w), np.uint8)
    vol[5, 2, 7] = 200
    zz, yy, xx = np.indices((d, h, w))
    dmap = 4 * (xx - 7) ** 2 + (yy - 2) ** 2 + 25 * (zz - 5) ** 2
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {"weight": (4, 1, 25)}, \
        {"map": dmap, "max_d2": 4 * 49 + 36 + 625, "max_at": (0, 8, 0), "n_finite": w * h * d, "near": {0: 0}}


def ball():
    """19^3 with a solid ball of radius 6 round (9, 9, 9), INSIDE: the deepest point is the centre, and the nearest texels that are not
    solid are (15, 10, 9) and its like at 36 + 1 = 37, the smallest sum of three squares above 36"""
    n, c = 19, 9
    zz, yy, xx = np.indices((n, n, n))
    vol = np.where((xx - c) ** 2 + (yy - c) ** 2 + (zz - c) ** 2 <= 36, 90, 0)
    return (n, n, n), _flat(vol), np.zeros(n ** 3, np.uint8), {"flags": INSIDE}, {"max_d2": 37, "max_at": (c, c, c), "n_finite": n ** 3, "near": {0: 1}}


def slabs(weight):
    """14 x 6 x 5: slab A (label 1) on x < 3, slab B (label 2) on x >= 9, A selected: the clearance of B is gap^2 * weight, the gap
    being 9 - 2 = 7, at the first texel of B's face"""
    w, h, d = 14, 6, 5
    vol = np.zeros((d, h, w), np.uint8)
    lab = np.zeros((d, h, w), np.uint8)
    vol[:, :, :3], lab[:, :, :3] = 60, 1
    vol[:, :, 9:], lab[:, :, 9:] = 60, 2
    select = np.zeros(256, np.int64)
    select[1] = 1
    return (w, h, d), _flat(vol), _flat(lab), {"select": select, "weight": (weight, 1, 1)}, \
        {"near": {1: 0, 2: 49 * weight}, "near_at": {2: (9, 0, 0)}, "max_d2": 121 * weight, "max_at": (13, 0, 0), "n_finite": w * h * d}


def empty_set():
    """8 x 5 x 4 with no solid texel: everything is NONE"""
    w, h, d = 8, 5, 4
    return (w, h, d), np.zeros(w * h * d, np.uint8), np.zeros(w * h * d, np.uint8), {"weight": (1, 4, 9)}, \
        {"map": np.full((d, h, w), NONE, np.int64), "max_d2": NONE, "max_at": (0, 0, 0), "n_finite": 0, "near": {}}


def full_box(inside):
    """9 x 6 x 4, every texel solid, weights (1, 4, 9): all 0, or with INSIDE the border rule alone"""
    w, h, d = 9, 6, 4
    zz, yy, xx = np.indices((d, h, w))
    border = np.minimum(np.minimum(np.minimum(xx + 1, w - xx) ** 2, 4 * np.minimum(yy + 1, h - yy) ** 2), 9 * np.minimum(zz + 1, d - zz) ** 2)
    dmap = border if inside else np.zeros((d, h, w), np.int64)
    return (w, h, d), np.full(w * h * d, 255, np.uint8), np.zeros(w * h * d, np.uint8), {"flags": INSIDE if inside else 0, "weight": (1, 4, 9)}, \
        {"map": dmap, "n_finite": w * h * d, "max_d2": int(dmap.max()), "near": {0: int(dmap.min())}}


def row_ends(last):
    """97 x 3 x 2: seeds only in the last chunk of every 97-texel row (x = 90), or only in the first (x = 5): the carries of the row
    sweep, from the right and from the left"""
    w, h, d = 97, 3, 2
    at = 90 if last else 5
    vol = np.zeros((d, h, w), np.uint8)
    vol[:, :, at] = 17
    dmap = np.broadcast_to(9 * (np.arange(w) - at) ** 2, (d, h, w)).astype(np.int64)
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {"weight": (9, 1, 1)}, {"map": dmap, "max_d2": 9 * max(at, w - 1 - at) ** 2, "n_finite": w * h * d}


def column_end():
    """3 x 70 x 2 whose only seeds are the last entries of the y columns"""
    w, h, d = 3, 70, 2
    vol = np.zeros((d, h, w), np.uint8)
    vol[:, h - 1, :] = 5
    dmap = np.broadcast_to((4 * (np.arange(h) - (h - 1)) ** 2)[None, :, None], (d, h, w)).astype(np.int64)
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {"weight": (1, 4, 1)}, {"map": dmap, "max_d2": 4 * 69 ** 2, "max_at": (0, 0, 0), "n_finite": w * h * d}


def squares():
    """300 x 4 x 4, long and thin, one seed at (0, 0, 0): D = x^2 + y^2 + z^2 takes every perfect square up to 299^2 (y = z = 0),
    every square + 1, the squares - 1 3, 8, 24, 35 and 99, and values from 255^2 on.  Bin k of the histogram holds the texels with
    (k - 1)^2 < D <= k^2, bin 255 everything above 254^2: counted here with math.isqrt"""
    import math
    w, h, d = 300, 4, 4
    vol = np.zeros((d, h, w), np.uint8)
    vol[0, 0, 0] = 1
    zz, yy, xx = np.indices((d, h, w))
    dmap = xx ** 2 + yy ** 2 + zz ** 2
    values = set(dmap.ravel().tolist())
    assert {3, 8, 24, 35, 99, 100, 101, 255 ** 2, 255 ** 2 + 1, 299 ** 2} <= values
    bins = {}
    for v in dmap.ravel().tolist():
        k = min(math.isqrt(v - 1) + 1 if v else 0, 255)
        bins[k] = bins.get(k, 0) + 1
    bins.update({k: 0 for k in range(256) if k not in bins})
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {}, \
        {"map": dmap, "max_d2": 299 ** 2 + 9 + 9, "max_at": (299, 3, 3), "n_finite": w * h * d, "bins": bins}


def constructed():
    """name -> (dims, vol, labels, scene.Distance, closed form)"""
    from volym_amd import scene
    made = {"single texel": single_texel(), "ball": ball(), "slabs": slabs(1), "slabs weighted": slabs(25), "empty set": empty_set(),
            "full box": full_box(False), "full box inside": full_box(True), "seeds in the last chunk": row_ends(True),
            "seeds in the first chunk": row_ends(False), "column end": column_end(), "squares": squares()}
    return {name: (dims, vol, lab, scene.Distance(dims=dims, **kw), closed) for name, (dims, vol, lab, kw, closed) in made.items()}


def check_closed(name, result, closed):
    """a (summary, map) against the closed form of a constructed scene"""
    summary, dmap = result
    if "map" in closed:
        assert np.array_equal(dmap.astype(np.int64), closed["map"]), name
    for k in ("max_d2", "n_finite"):
        if k in closed:
            assert int(summary[k]) == closed[k], (name, k, int(summary[k]), closed[k])
    if "max_at" in closed:
        assert tuple(int(v) for v in summary["max_at"]) == closed["max_at"], (name, summary["max_at"])
    if "near" in closed:
        got = {l: int(summary["near_d2"][l]) for l in np.flatnonzero(summary["near_d2"] != NONE).tolist()}
        assert got == closed["near"], (name, got)
    for l, at in closed.get("near_at", {}).items():
        assert tuple(int(v) for v in summary["near_at"][l]) == at, (name, l)
    for k, v in closed.get("bins", {}).items():
        assert int(summary["hist"][k]) == v, (name, "bin", k)
