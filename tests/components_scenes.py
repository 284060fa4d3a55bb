"""The scenes and requests of the components tests, shared by tests/test_components_host.py (which pins the host twin to a plain flood
fill and to the closed forms below) and tests/test_gpu_components.py (which compares the device with the twin).  Scenes A and B, their
boxes, cut states, select tables and thresholds are those of tests/measure_scenes.py and tests/surface_scenes.py; the constructed
scenes are built here.
"""
import functools

import numpy as np

from tests import measure_scenes as M
from tests import surface_scenes as S

DIMS, NX, NY, NZ = M.DIMS, M.NX, M.NY, M.NZ
BOX, PLANE, HIDDEN = M.BOX, M.PLANE, M.HIDDEN
BOXES, CUTS, MIN_BYTES = S.BOXES, S.CUTS, S.MIN_BYTES
LONG_DIMS, LONG_BOXES = S.LONG_DIMS, S.LONG_BOXES
scene_a, scene_b, selects = M.scene_a, M.scene_b, S.selects
UNCUT, SPLIT = 1, 2                 # _lib.COMPONENTS_UNCUT, _lib.COMPONENTS_SPLIT_LABELS


def every_request(flags=0):
    """(name, scene.Components): every box with every select table at every min_byte"""
    from volym_amd import scene
    return [("%s / %s / %d" % (b, n, m), scene.Components(box, flags, m, sel)) for b, box in BOXES.items() for n, sel in selects().items() for m in MIN_BYTES]


def requests(flags=0):
    """(name, scene.Components): the short list for every cut state -- every box with a rotating select table and min_byte, and the
    whole volume with every select table and every min_byte"""
    from volym_amd import scene
    sel = selects()
    turn = ("mix", "all", "one")
    out = [("%s / %s / %d" % (b, turn[k % 3], MIN_BYTES[(k // 2) % 3]), scene.Components(box, flags, MIN_BYTES[(k // 2) % 3], sel[turn[k % 3]]))
           for k, (b, box) in enumerate(BOXES.items())]
    out += [("whole / %s / 128" % n, scene.Components(BOXES["whole"], flags, 128, sel[n])) for n in sel]
    out += [("whole / all / %d" % m, scene.Components(BOXES["whole"], flags, m, sel["all"])) for m in MIN_BYTES if m != 128]
    return out


@functools.lru_cache(None)
def scan_components(split):
    """(scene.Components over S.SCAN_BOX, the twin's (summary, table, ids) of S.scan_scene): the surface test's request with
    SPLIT_LABELS, or no flags and every label selected; computed once, left unchanged"""
    from volym_amd import scene
    dims, vol, labels = S.scan_scene()
    c = scene.Components(S.SCAN_BOX, SPLIT, S.SCAN_MIN_BYTE, scene.surface_select(S.SCAN_LABELS)) if split else scene.Components(S.SCAN_BOX, 0, S.SCAN_MIN_BYTE)
    return c, scene.components_volume(vol, dims, c, labels=labels)


def expect(host, c, labels=True):
    """the twin's (summary, table, ids) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.components_volume(now, host.dims, c, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 2072 bytes of struct volym_components_summary, then the records, then the id volume"""
    summary, table, ids = result
    return summary.tobytes() + np.ascontiguousarray(table).tobytes() + np.ascontiguousarray(ids, np.uint32).tobytes()


def flood_fill(solid, lab=None):
    """The rule as a plain breadth-first flood fill: `solid` a bool array [z, y, x] over the request's box, `lab` the labels over it
    when links need equal labels.  Returns (ids [z, y, x] with -1 for not solid, the root (x, y, z) of every component in box
    coordinates, its count): the scan meets roots in ascending (z, y, x), so the numbers are canonical."""
    d, h, w = solid.shape
    ids = np.full((d, h, w), -1, np.int64)
    roots, counts = [], []
    sol = solid.tolist()
    la = lab.tolist() if lab is not None else None
    out = ids.tolist()
    for z in range(d):
        for y in range(h):
            for x in range(w):
                if not sol[z][y][x] or out[z][y][x] >= 0:
                    continue
                k = len(roots)
                roots.append((x, y, z))
                out[z][y][x] = k
                queue, n = [(x, y, z)], 0
                while queue:
                    cx, cy, cz = queue.pop()
                    n += 1
                    for ax, ay, az in ((cx - 1, cy, cz), (cx + 1, cy, cz), (cx, cy - 1, cz), (cx, cy + 1, cz), (cx, cy, cz - 1), (cx, cy, cz + 1)):
                        if 0 <= ax < w and 0 <= ay < h and 0 <= az < d and sol[az][ay][ax] and out[az][ay][ax] < 0 and \
                                (la is None or la[az][ay][ax] == la[cz][cy][cx]):
                            out[az][ay][ax] = k
                            queue.append((ax, ay, az))
                counts.append(n)
    return np.array(out, np.int64).reshape(d, h, w), roots, counts


# ---- the constructed scenes: name -> (dims, vol, labels, request keywords, closed form) ---------------------------------------------
# closed form: n_components, n_solid, and optionally "counts" (of every component in canonical order) and "open" (its border flags)
def _flat(a):
    return np.ascontiguousarray(a, np.uint8).ravel()


def serpentine():
    """One path, one texel thick, through a 66 x 9 x 7 box: full x-lines on the even y of the even z, run back and forth, joined at
    alternating ends by single texels on the odd y and, from plane to plane, on the odd z.  Its last texel is thousands of links
    from its root (0, 0, 0), and its unions arrive in every order."""
    w, h, d = 66, 9, 7
    vol = np.zeros((d, h, w), np.uint8)
    x, n = 0, 0
    planes = list(range(0, d, 2))
    for zi, z in enumerate(planes):
        ys = list(range(0, h, 2))
        if zi % 2:
            ys.reverse()
        for yi, y in enumerate(ys):
            vol[z, y, :] = 200
            n += w
            x = w - 1 - x                                        # the line ends at the other side
            if yi + 1 < len(ys):
                vol[z, (y + ys[yi + 1]) // 2, x] = 200
                n += 1
        if zi + 1 < len(planes):
            vol[z + 1, ys[-1], x] = 200
            n += 1
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {}, {"n_components": 1, "n_solid": n, "counts": [n], "open": [1]}


def combs():
    """Two interleaved combs that never touch, 70 x 19 x 3: spines at x = 0 and x = 69, teeth on y = 0, 4, 8, ... from the left and
    on y = 2, 6, 10, ... from the right, one empty texel between tooth and tooth and between tooth and the other spine."""
    w, h, d = 70, 19, 3
    vol = np.zeros((d, h, w), np.uint8)
    vol[:, :, 0] = 9
    vol[:, :, w - 1] = 9
    vol[:, 0::4, 0:w - 2] = 9
    vol[:, 2::4, 2:w] = 9
    left = d * (h + len(range(0, h, 4)) * (w - 3))
    right = d * (h + len(range(2, h, 4)) * (w - 3))
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {}, {"n_components": 2, "n_solid": left + right, "counts": [left, right], "open": [1, 1]}


def checkerboard():
    """13 x 7 x 5, solid where x + y + z is even: every solid texel is its own piece"""
    w, h, d = 13, 7, 5
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    vol = np.where((xx + yy + zz) % 2 == 0, 77, 0)
    n = int((vol > 0).sum())
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {}, {"n_components": n, "n_solid": n, "counts": [1] * n}


def slabs(joined):
    """9 x 6 x 5: two slabs of two z planes, and between them one texel (4, 3, 2), or none"""
    w, h, d = 9, 6, 5
    vol = np.zeros((d, h, w), np.uint8)
    vol[0:2] = 50
    vol[3:5] = 50
    if joined:
        vol[2, 3, 4] = 50
        closed = {"n_components": 1, "n_solid": 4 * w * h + 1, "counts": [4 * w * h + 1], "open": [1]}
    else:
        closed = {"n_components": 2, "n_solid": 4 * w * h, "counts": [2 * w * h, 2 * w * h], "open": [1, 1]}
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {}, closed


def label_blocks(split):
    """10 x 4 x 3, all solid, label 1 for x < 5 and 2 from there: one piece, or with SPLIT_LABELS two"""
    w, h, d = 10, 4, 3
    lab = np.zeros((d, h, w), np.uint8)
    lab[:, :, :5], lab[:, :, 5:] = 1, 2
    closed = {"n_components": 2, "n_solid": w * h * d, "counts": [w * h * d // 2] * 2, "open": [1, 1]} if split else \
             {"n_components": 1, "n_solid": w * h * d, "counts": [w * h * d], "open": [1]}
    return (w, h, d), np.full(w * h * d, 99, np.uint8), _flat(lab), {"flags": SPLIT if split else 0}, closed


def cut_by_the_box():
    """12 x 12 x 3: a U in the plane z = 1 (prongs at x = 2 and x = 8 from y = 1, joined along y = 9); the request's box ends at
    y = 8 and leaves two prongs, each on the box's y face"""
    w, h, d = 12, 12, 3
    vol = np.zeros((d, h, w), np.uint8)
    vol[1, 1:10, 2] = 30
    vol[1, 1:10, 8] = 30
    vol[1, 9, 2:9] = 30
    return (w, h, d), _flat(vol), np.zeros(w * h * d, np.uint8), {"box": ((1, 0, 0), (11, 8, 3))}, \
        {"n_components": 2, "n_solid": 14, "counts": [7, 7], "open": [1, 1]}


def constructed():
    """name -> (dims, vol, labels, scene.Components, closed form)"""
    from volym_amd import scene
    made = {"serpentine": serpentine(), "combs": combs(), "checkerboard": checkerboard(), "slabs joined": slabs(True), "slabs apart": slabs(False),
            "label blocks": label_blocks(False), "label blocks split": label_blocks(True), "cut by the box": cut_by_the_box()}
    return {name: (dims, vol, lab, scene.Components(dims=dims, **kw), closed) for name, (dims, vol, lab, kw, closed) in made.items()}
