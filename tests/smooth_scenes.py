"""The scenes and requests of the smoothing tests, shared by tests/test_smooth_host.py (which pins the twin to a plain triple loop and
asserts on it the conditions the device tests rely on) and tests/test_gpu_smooth.py (which compares the device with the twin).

The scenes are those of tests/relabel_scenes.py: A (37 x 22 x 19, five labels in blocks), B (random labels over all 256 values) and
the ragged scene (97 x 80 x 71, a shell (1), a core (2) and a blob (5) in air (0)).  No axis is a multiple of 4 and a row is no
multiple of 16, so linear chunks wrap rows and slices.  Every request is laid out in scene A's dimensions, which fit inside the ragged
scene's; "whole" follows the scene.

A Case is a request and the scenes in which it may change fewer than 20 texels (`few`): scene A's blocks are aligned to the slices,
so smoothing inside slices changes nothing there, and the ragged scene's labels are smooth already.
"""
import numpy as np

from tests import measure_scenes as MS
from tests import relabel_scenes as RS

DIMS = MS.DIMS
RAGGED_DIMS = RS.RAGGED_DIMS
SCENES = {"a": RS.scene_a, "b": RS.scene_b, "ragged": RS.scene_ragged}
SMALL_DIMS = ((7, 5, 3), (5, 3, 9))
EVERYWHERE = ("a", "b", "ragged")

# what the rule changes, checked on the CPU with a prototype of it before the device existed: (scene, radius) -> texels; and the
# linear chunks that hold them
TEXELS = {("a", (1, 1, 1)): 154, ("a", (1, 1, 0)): 0, ("b", (1, 1, 1)): 9218, ("ragged", (1, 1, 1)): 262, ("ragged", (1, 1, 0)): 21}
LINEAR_CHUNKS = {("a", (1, 1, 1)): (51, 967), ("b", (1, 1, 1)): (964, 967)}


class Case:
    def __init__(self, name, smooth, few=()):
        self.name, self.smooth, self.few = name, smooth, tuple(few)


def table(*labels):
    t = np.zeros(256, np.int64)
    t[list(labels)] = 1
    return t


def but(*labels):
    t = np.ones(256, np.int64)
    t[list(labels)] = 0
    return t


def cases(dims=DIMS):
    """the requests of the issue, for a scene of `dims` (at least scene A's)"""
    from volym_amd import _lib, scene
    B = dict(MS.BOXES, whole=((0, 0, 0), tuple(dims)))

    def S(radius, box="whole", **kw):
        return scene.Smooth(radius, B[box], dims=dims, **kw)

    pair = table(0, 2)
    return [
        Case("joint, radius 1", S((1, 1, 1))),
        Case("joint, radius 2", S((2, 2, 2))),
        Case("joint, radius 3", S((3, 3, 3))),
        Case("joint, inside slices", S((1, 1, 0)), few=("a",)),
        Case("joint, along x by 3", S((3, 0, 0))),
        Case("joint, radius 0, 2, 1", S((0, 2, 1)), few=("a",)),
        Case("joint, radius 2, rows", S((2, 2, 2), "rows"), few=("ragged",)),
        Case("joint, radius 2, 1, 2, x 3..8", S((2, 1, 2), "x 3..8"), few=("ragged",)),
        Case("joint, radius 2, x 5..30", S((2, 2, 2), "x 5..30"), few=("ragged",)),
        Case("joint, radius 3, x 5..30", S((3, 3, 3), "x 5..30"), few=("ragged",)),
        Case("joint, inside slices, rows", S((1, 1, 0), "rows"), few=("a", "ragged")),
        Case("2 against 0, radius 1", S((1, 1, 1), give=pair, take=pair), few=("a", "b")),
        Case("2 against 0, radius 2, 2, 1", S((2, 2, 1), give=pair, take=pair), few=("b",)),
        Case("take leaves out 0 and 2", S((1, 1, 1), take=but(0, 2))),
        Case("only 1 gives, radius 2", S((2, 2, 2), give=table(1))),
        Case("window 100..180", S((1, 1, 1), window=(100, 180))),
        Case("uncut bytes, window 1..120, radius 2", S((2, 2, 2), flags=_lib.SMOOTH_UNCUT, window=(1, 120))),
        Case("dry run", S((1, 1, 1), flags=_lib.SMOOTH_DRY_RUN)),
        Case("single texel", S((1, 1, 1), "texel"), few=EVERYWHERE),
        Case("empty box", S((1, 1, 1), "empty"), few=EVERYWHERE),
    ]


def scene_small(dims, seed=3):
    """a small volume of four labels in random order: a slice may be smaller than a chunk"""
    host = RS.Host(dims)
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    host.vol = rng.integers(1, 256, nx * ny * nz).astype(np.uint8)
    host.labels = rng.integers(0, 4, nx * ny * nz).astype(np.uint8)
    return host


def scene_overflow():
    """the ragged scene's volume with random labels over 16 values: a pass at radius 1 changes most of its 34 435 linear chunks, more
    than the first launch's staging area holds"""
    host = RS.scene_ragged()
    host.labels = np.random.default_rng(29).integers(0, 16, host.labels.size).astype(np.uint8)
    return host


def first_capacity(items):
    """the records the staging area of the vote's first launch holds for a slab of `items` items"""
    return min(items, max(4096, items // 16))


def small_requests(dims):
    """every flag and radius combination on a small volume: (name, request)"""
    from volym_amd import _lib, scene
    out = []
    for flags in (0, _lib.SMOOTH_UNCUT, _lib.SMOOTH_DRY_RUN, _lib.SMOOTH_UNCUT | _lib.SMOOTH_DRY_RUN):
        for radius in ((1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 1, 0), (3, 0, 0), (0, 2, 1), (0, 0, 1), (2, 1, 3)):
            out.append(("flags %d, radius %r" % (flags, radius), scene.Smooth(radius, None, flags, (40, 255) if flags & _lib.SMOOTH_UNCUT else (0, 255),
                                                                               take=but(3) if radius[0] == 2 else None, dims=dims)))
    return out


def expect(host, case, smooth=None):
    """the twin's (new_labels [flat], result) of `case` in the state `host` is in"""
    from volym_amd import scene
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, result = scene.smooth_volume(now, host.dims, smooth or case.smooth, host.labels, uncut=host.vol)
    return new.ravel(), result


def plain_smooth(vol, dims, r, labels):
    """The rule as a plain triple loop over Python integers and a collections.Counter: (new labels [flat], changed, left, arrived,
    box or None).  `vol` is the density the window reads."""
    from collections import Counter
    nx, ny, nz = dims
    lab = [int(v) for v in np.asarray(labels).ravel()]
    den = [int(v) for v in np.asarray(vol).ravel()]
    new = list(lab)
    (x0, y0, z0), (x1, y1, z1) = r.box
    rx, ry, rz = r.radius
    takes = [m for m in range(256) if r.take[m]]
    left, arrived, hull, changed = Counter(), Counter(), None, 0
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                at = x + nx * (y + ny * z)
                l = lab[at]
                if not r.give[l] or not r.window[0] <= den[at] <= r.window[1]:
                    continue
                count = Counter()
                for w in range(max(z - rz, 0), min(z + rz, nz - 1) + 1):
                    for v in range(max(y - ry, 0), min(y + ry, ny - 1) + 1):
                        for u in range(max(x - rx, 0), min(x + rx, nx - 1) + 1):
                            count[lab[u + nx * (v + ny * w)]] += 1
                top = max(count[m] for m in set(takes) | {l})
                if count[l] == top:
                    continue
                winner = min(m for m in takes if count[m] == top)
                changed += 1
                left[l] += 1
                arrived[winner] += 1
                hull = (x, y, z, x + 1, y + 1, z + 1) if hull is None else tuple(min(a, b) for a, b in zip(hull[:3], (x, y, z))) + \
                    tuple(max(a, b) for a, b in zip(hull[3:], (x + 1, y + 1, z + 1)))
                if not r.flags & 16:
                    new[at] = winner
    return np.array(new, np.uint8), changed, left, arrived, hull
