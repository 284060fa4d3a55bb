"""The scenes and requests of the interpolate tests (fill between slices), shared by tests/test_interpolate_host.py (which pins the
host twins to a per-texel restatement in Python integers, to scipy's transform, to closed forms and to a case built about the 64-bit
comparison) and tests/test_gpu_interpolate.py (which compares the device with the twins).  Scenes A and B, their boxes and cut states
are those of tests/geodesic_scenes.py, the long rows those of tests/surface_scenes.py; the painted, strip, disc and wide scenes are
built here, in slices-first order [k, u, v] and turned to the axis asked for.
"""
import numpy as np

from tests import geodesic_scenes as GS

DIMS, NX, NY, NZ = GS.DIMS, GS.NX, GS.NY, GS.NZ
BOX, PLANE, HIDDEN = GS.BOX, GS.PLANE, GS.HIDDEN
BOXES, CUTS = GS.BOXES, GS.CUTS
LONG_DIMS, LONG_BOXES = GS.LONG_DIMS, GS.LONG_BOXES
scene_a, scene_b, table = GS.scene_a, GS.scene_b, GS.table
NONE = 0xFFFFFFFF                               # _lib.INTERPOLATE_NONE
UNCUT, KEYS = 1, 2                              # _lib.INTERPOLATE_UNCUT, _lib.INTERPOLATE_KEYS
SHAPE, INSIDE, GAP = 1, 2, 4                    # the bits of a state byte
EDIT_UNCUT, EDIT_DRY_RUN = 1, 2
OUTSIDE_SLICE, KEY_SLICE, GAP_SLICE, REFUSED_SLICE = 0, 1, 2, 3


# ---- requests over scenes A and B ------------------------------------------------------------------------------------------------------
SELECTS = [table(1, 2, 3), table(2), 1 - table(0), table(0, 4), table(*range(0, 256, 5))]
WEIGHTS = [(1, 1, 1), (64, 1, 4), (1, 64, 64), (4, 9, 25)]
MIN_BYTES = [0, 128, 1, 200]
MAX_GAPS = [0, 3, 0, 2]
KEY_SETS = [None, (0, 4, 5, 11, 18, 30), (2, 9, 12, 13, 36), None, (1, 3, 16, 17, 21)]


def requests(flags=0, turn=0):
    """(name, scene.Interpolate): every box of the scenes on every axis in turn, with a rotating selection, min_byte, weights, max_gap
    and KEYS set (None: the slices that hold the shape)"""
    from volym_amd import scene
    out = []
    for k, (b, box) in enumerate(BOXES.items()):
        for axis in range(3):
            j = k + turn + axis
            keys = KEY_SETS[j % len(KEY_SETS)]
            out.append(("%s / axis %d / turn %d" % (b, axis, j),
                        scene.Interpolate(box, flags | (KEYS if keys is not None else 0), MIN_BYTES[j % 4], SELECTS[j % len(SELECTS)], WEIGHTS[(j + axis) % 4], axis,
                                          MAX_GAPS[(j + k) % 4], keys or ())))
    return out


def expect(host, q, labels=True):
    """the twin's (summary, map, state) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.interpolate_volume(now, host.dims, q, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 65592 bytes of struct volym_interpolate_summary, then the signed map, then the state map"""
    summary, words, state = result
    return summary.tobytes() + np.ascontiguousarray(words, np.uint32).tobytes() + np.ascontiguousarray(state, np.uint8).tobytes()


# ---- the rule restated -------------------------------------------------------------------------------------------------------------------
def turned(a, axis):
    """[k, u, v] (slices first) -> [z, y, x] with the slices perpendicular to `axis`"""
    return np.ascontiguousarray(np.moveaxis(a, 0, 2 - axis))


def slices_first(a, axis):
    """[z, y, x] -> [k, u, v]"""
    return np.moveaxis(a, 2 - axis, 0)


def plane_weights(weight, axis):
    """the weights of u and v"""
    return [weight[a] for a in (2, 1, 0) if a != axis]


def inside_by_words(m0, m1, a, b, wrap=None):
    """the decision of the rule from the two words, Python integers; wrap: the products are taken modulo it (what arithmetic of that
    width would give)"""
    def shape(m):
        return m != NONE and (m & 1) == 1

    def outside(m):
        return m != NONE and (m & 1) == 0

    left, right = a * a * (m0 >> 1), b * b * (m1 >> 1)
    if wrap:
        left, right = left % wrap, right % wrap
    return (shape(m0) and shape(m1)) or (shape(m0) and outside(m1) and left > right) or (shape(m1) and outside(m0) and right > left)


def brute_force(shape, weights, keys=None, max_gap=0):
    """The rule texel by texel over Python integers.  shape: bool [k, u, v]; keys: the slice indices (None: the slices with a SHAPE
    texel).  Returns (words, state, kinds): Python ints [k][u][v] as nested lists in NumPy arrays (int64, uint8) and the kind per slice."""
    n, nu, nv = shape.shape
    wu, wv = int(weights[0]), int(weights[1])
    is_key = [bool(shape[k].any()) if keys is None else k in keys for k in range(n)]
    words = np.full(shape.shape, NONE, np.int64)
    state = np.where(shape, SHAPE, 0).astype(np.uint8)
    for k in range(n):
        if not is_key[k]:
            continue
        on = [(u, v) for u in range(nu) for v in range(nv) if shape[k, u, v]]
        off = [(u, v) for u in range(nu) for v in range(nv) if not shape[k, u, v]]
        for u in range(nu):
            for v in range(nv):
                if shape[k, u, v]:
                    best = min(wu * min(u + 1, nu - u) ** 2, wv * min(v + 1, nv - v) ** 2)
                    for s, t in off:
                        best = min(best, wu * (u - s) ** 2 + wv * (v - t) ** 2)
                    words[k, u, v] = best << 1 | 1
                    state[k, u, v] |= INSIDE
                elif on:
                    words[k, u, v] = min(wu * (u - s) ** 2 + wv * (v - t) ** 2 for s, t in on) << 1
    kinds = [KEY_SLICE if is_key[k] else OUTSIDE_SLICE for k in range(n)]
    at = [k for k in range(n) if is_key[k]]
    for z0, z1 in zip(at, at[1:]):
        if z1 - z0 < 2:
            continue
        if max_gap and z1 - z0 - 1 > max_gap:
            for z in range(z0 + 1, z1):
                kinds[z] = REFUSED_SLICE
            continue
        for z in range(z0 + 1, z1):
            kinds[z] = GAP_SLICE
            for u in range(nu):
                for v in range(nv):
                    state[z, u, v] |= GAP
                    if inside_by_words(int(words[z0, u, v]), int(words[z1, u, v]), z1 - z, z - z0):
                        state[z, u, v] |= INSIDE
    return words, state, kinds


def state_from_words(words, summary, axis, lo, wrap=None):
    """the state bytes of the gap slices again, from a signed map [z, y, x] and its summary, by inside_by_words: GAP | INSIDE bits only,
    [k, u, v]"""
    w = slices_first(np.asarray(words, np.int64), axis)
    out = np.zeros(w.shape, np.uint8)
    for k in range(int(summary["n_slices"])):
        rec = summary["slice"][k]
        if int(rec["kind"]) != GAP_SLICE:
            continue
        z0, z1 = int(rec["key_lo"]) - lo, int(rec["key_hi"]) - lo
        for (u, v), m0 in np.ndenumerate(w[z0]):
            out[k, u, v] = GAP | (INSIDE if inside_by_words(int(m0), int(w[z1, u, v]), z1 - k, k - z0, wrap) else 0)
    return out


# ---- the constructed scenes ----------------------------------------------------------------------------------------------------------------
def _blob(nu, nv, cu, cv, r2):
    u, v = np.indices((nu, nv))
    return (u - cu) ** 2 + (v - cv) ** 2 <= r2


def scene_of(shape, axis, label=5, noise=None):
    """(dims, vol, labels) of a bool [k, u, v]: the shape carries `label`, everything else 0 (or `noise`, an array of other labels);
    the density is 200 on the shape and 90 elsewhere"""
    s = turned(shape, axis)
    lab = np.where(s, label, 0 if noise is None else turned(noise, axis)).astype(np.uint8)
    vol = np.where(s, 200, 90).astype(np.uint8)
    return s.shape[::-1], vol.ravel(), lab.ravel()


def painted(n=17, nu=14, nv=19):
    """blobs painted on slices 2, 7, 8 and 15: a gap of 4, two adjacent keys, a gap of 6, and slices outside on both ends"""
    shape = np.zeros((n, nu, nv), bool)
    shape[2] = _blob(nu, nv, 6, 8, 30)
    shape[7] = _blob(nu, nv, 8, 11, 12) | _blob(nu, nv, 3, 3, 2)
    shape[8] = _blob(nu, nv, 7, 10, 20)
    shape[15] = _blob(nu, nv, 5, 9, 45)
    return shape


STRIP = dict(n=9, nu=41, nv=30, p0=21, p1=12, row=20)      # {v < p0} on slice 0, {v < p1} on slice 8; the closed form holds on the middle row


def strips():
    """Half-plane strips on two keys.  On row `row` the border is further than the strip's edge for every v >= p1 (v + 1 >= p0 - v and
    21^2 >= (p0 - v)^2), so Din = (p0 - v)^2 there and a texel of slice z is INSIDE iff a (p0 - v) > b (v - p1 + 1); the two factors
    add up to 10 and a + b to 8, so a = b = 4 meets equality at v = 16."""
    c = STRIP
    shape = np.zeros((c["n"], c["nu"], c["nv"]), bool)
    shape[0, :, :c["p0"]] = True
    shape[c["n"] - 1, :, :c["p1"]] = True
    return shape


def discs(r0=15, r1=5, n=11, size=41):
    """concentric discs of radius r0 and r1 on slices 0 and n - 1"""
    shape = np.zeros((n, size, size), bool)
    shape[0] = _blob(size, size, size // 2, size // 2, r0 * r0)
    shape[n - 1] = _blob(size, size, size // 2, size // 2, r1 * r1)
    return shape


def disjoint(thin=False):
    """two keys whose shapes do not overlap in projection.  The rule lets each shape shrink towards the other key -- a texel of one
    shape stays INSIDE while a^2 Din > b^2 Dout -- so nothing joins them, and nothing at all is INSIDE once every Din is small against
    the Dout across: `thin`, lines one texel wide (Din = 1) ten texels apart (Dout >= 100 > 4^2)."""
    shape = np.zeros((6, 12, 20), bool)
    if thin:
        shape[0, 2:6, 3] = True
        shape[5, 7:11, 13] = True
    else:
        shape[0, 2:6, 1:7] = True
        shape[5, 7:11, 12:19] = True
    return shape


def wide():
    """The case about the 64-bit comparison: a plane 200 wide, weight 64 along it, a gap of 150 slices; strips {v < 190} and {v < 10}.
    a^2 D reaches 150^2 * 64 * 180^2 > 2^45."""
    shape = np.zeros((152, 3, 200), bool)
    shape[0, :, :190] = True
    shape[151, :, :10] = True
    return shape


def wide_weight(axis):
    """weight 64 on the axis v runs along"""
    v_axis = [a for a in (2, 1, 0) if a != axis][1]
    w = [1, 1, 1]
    w[v_axis] = 64
    return tuple(w)


def constructed():
    """name -> (dims, vol, labels, scene.Interpolate): the twin decides; the host tests pin the twin on the same scenes"""
    from volym_amd import scene
    out = {}
    sel = table(5)

    def add(name, shape, axis, box=None, **kw):
        dims, vol, lab = scene_of(shape, axis)
        out["%s / axis %d" % (name, axis)] = (dims, vol, lab, scene.Interpolate(box, kw.pop("flags", 0), kw.pop("min_byte", 0), sel, kw.pop("weight", (1, 1, 1)), axis,
                                                                              dims=dims, **kw))

    for axis in range(3):
        p = painted()
        add("painted", p, axis, weight=(1, 4, 9))
        add("painted, max_gap 4: one gap at it, one wider", p, axis, max_gap=4)
        add("painted, max_gap 6", p, axis, max_gap=6)
        add("painted, KEYS with a slice without SHAPE", p, axis, flags=KEYS, keys=(2, 5, 7, 15, 16))
        add("painted, min_byte above the rest", p, axis, min_byte=150)
        add("a single key", p[6:8] & np.array([False, True])[:, None, None], axis)
        add("no key", np.zeros((5, 4, 6), bool), axis)
        add("extent 1 along the axis", p[2:3], axis)
        add("extent 2 along the axis", p[7:9], axis)
        add("extent 3 along the axis", p[[2, 3, 15]], axis)
        add("in-plane extents of 1", np.array([1, 0, 0, 0, 1, 1, 0, 1], bool).reshape(8, 1, 1), axis)
        add("one in-plane extent of 1", painted()[:, 5:6, :], axis)
        full = np.zeros((5, 6, 9), bool)
        full[0] = True
        full[4, 2:4, 3:6] = True
        add("a key that is all SHAPE", full, axis, weight=(4, 1, 25))
        add("strips with ties", strips(), axis)
        add("discs", discs(), axis)
        add("disjoint", disjoint(), axis)
        add("disjoint and thin", disjoint(True), axis)
        add("wide", wide(), axis, weight=wide_weight(axis))
        big = np.zeros((23, 29, 37), bool)
        big[4, 6:20, 5:30] = _blob(14, 25, 7, 12, 40)
        big[12, 6:20, 5:30] = _blob(14, 25, 5, 15, 14)
        big[13, 2:9, 2:9] = True                                 # outside the box below: no key for it
        lo = [0, 0, 0]
        hi = list(turned(big, axis).shape[::-1])
        for a, (l, h) in zip([a for a in (2, 1, 0) if a != axis], ((5, 21), (3, 33))):
            lo[a], hi[a] = l, h
        lo[axis], hi[axis] = 1, 21
        add("a box off the origin and off the brick grid", big, axis, box=(tuple(lo), tuple(hi)), weight=(9, 1, 4))
    return out


# ---- the edit's requests over a snapshot ---------------------------------------------------------------------------------------------------
class EditCase:
    def __init__(self, name, interpolate, edit):
        self.name, self.interpolate, self.edit = name, interpolate, edit


def edit_scene():
    """(dims, vol, labels): the painted scene along z, its blobs label 5, with a stale earlier fill (label 5 on slices 4 and 11, partly
    outside the interpolated shape) and other labels about; random density"""
    rng = np.random.default_rng(11)
    p = painted()
    lab = np.where(p, 5, 0).astype(np.uint8)
    lab[4, 1:9, 2:12] = 5
    lab[11, 3:12, 6:18] = 5
    lab[5, :, :4] = 7
    lab[12, 10:, :] = 9
    dims = lab.shape[::-1]
    vol = rng.integers(1, 256, lab.size).astype(np.uint8)
    return dims, vol, lab.ravel()


def edit_cases(dims):
    from volym_amd import scene
    q = scene.Interpolate(None, KEYS, 0, table(5), (1, 1, 1), 2, 0, (2, 7, 8, 15), dims=dims)
    sub = ((2, 1, 3), (15, 12, 14))
    E = scene.InterpolateEdit
    return [EditCase("to alone", q, E(dims=dims, to={0: 5})),
            EditCase("out alone", q, E(dims=dims, out={5: 0})),
            EditCase("both", q, E(dims=dims, to={0: 5, 7: 5}, out={5: 0, 9: 1})),
            EditCase("a density window", q, E(dims=dims, window=(60, 180), to={0: 5}, out={5: 0})),
            EditCase("a sub-box", q, E(sub, to={0: 5, 9: 5}, out={5: 0})),
            EditCase("a dry run", q, E(dims=dims, flags=EDIT_DRY_RUN, to={0: 5}, out={5: 0})),
            EditCase("identity tables", q, E(dims=dims)),
            EditCase("a pass without KEYS: the stale fill makes keys", q.replace(flags=0, keys=()), E(dims=dims, to={0: 5}, out={5: 0})),
            EditCase("along x", q.replace(axis=0, keys=(1, 6, 13, 18)), E(dims=dims, to={0: 5, 7: 5}, out={5: 0}))]
