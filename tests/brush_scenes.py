"""The scenes and strokes of the brush tests, shared by tests/test_brush_host.py (which pins the twin to the exact rule and asserts
on it the conditions the device tests rely on) and tests/test_gpu_brush.py (which compares the device with the twin).

Scenes A and B are those of tests/measure_scenes.py: 37 x 22 x 19, random density bytes 1..255, five labels in blocks (A) or random
labels over all 256 values (B).  No axis is a multiple of 4 and a row is no multiple of 16, so linear chunks wrap rows and slices.
The ragged scene is that of tests/relabel_scenes.py: 97 x 80 x 71, a shell (1), a core (2) and a blob (5) in air (0).  Every stroke
is laid out in scene A's dimensions, which fit inside the ragged scene's; the corner ball, the capsule along x and the two whole rows
follow the scene's own width and far corner.

A Case is a stroke and what the host test asserts about it: `trivial` (it may change fewer than 50 texels), `ragged` (in the ragged
scene its changed texels share linear chunks across rows), `count` (the texels within the stroke, in scene A's dimensions -- what the
stroke changes there when its table moves every label).

The small scene is 5 x 3 x 9 with three labels in blocks of three slices: a slice has 15 texels, fewer than a chunk, so every linear
chunk spans up to four rows and two slices, and the last chunk is partial.  Its strokes (small_cases) are run by the device tests
with the history off and on; rows_shared says what the host test asserts of them.
"""
import numpy as np

from tests import measure_scenes as MS
from tests import relabel_scenes as RS

DIMS = MS.DIMS
RAGGED_DIMS = RS.RAGGED_DIMS
SCENES = {"a": RS.scene_a, "b": RS.scene_b, "ragged": RS.scene_ragged}
SMALL_DIMS = (5, 3, 9)


class Case:
    def __init__(self, name, brush, trivial=False, ragged=False, count=None):
        self.name, self.brush, self.trivial, self.ragged, self.count = name, brush, trivial, ragged, count


def every(value):
    """the table that sends every label to `value`"""
    return np.full(256, value, np.int64)


def swap_1_2():
    to = np.arange(256, dtype=np.int64)
    to[1], to[2] = 2, 1
    return to


def walk(dims, n=256, seed=5):
    """a random walk of n points inside the volume with steps of at most 3 texels per axis"""
    rng = np.random.default_rng(seed)
    p = np.array([d // 2 for d in dims], np.int64)
    out = []
    for _ in range(n):
        out.append(tuple(int(v) for v in p))
        p = np.clip(p + rng.integers(-3, 4, 3), 0, np.array(dims) - 1)
    return out


def cases(dims=DIMS):
    """the strokes of the issue, for a scene of `dims` (at least scene A's)"""
    from volym_amd import _lib, scene
    nx, ny, nz = dims
    far = (nx - 1, ny - 1, nz - 1)

    def B(points, r2, **kw):
        kw.setdefault("to", every(7))
        return scene.Brush(points, r2, dims=dims, **kw)

    lift = _lib.BRUSH_LIFT
    return [
        Case("single texel", B([(17, 9, 11)], 0), trivial=True, count=1),
        Case("ball of r2 25 at the origin", B([(0, 0, 0)], 25)),
        Case("ball of r2 25 at the far corner", B([far], 25)),
        Case("capsule along x, r2 4", B([(2, 10, 9), (nx - 3, 10, 9)], 4), ragged=True, count=449 if dims == DIMS else None),
        Case("the long diagonal, r2 6", B([(1, 1, 1), (35, 20, 17)], 6), count=826),
        Case("weights 1, 1, 25, r2 25", B([(18, 10, 9)], 25, weight=(1, 1, 25)), count=83),
        Case("weights 64, 1, 3, r2 64, oblique", B([(5, 3, 4), (20, 15, 12)], 64, weight=(64, 1, 3))),
        Case("four points, a lift at the third", B([(3, 3, 3), (14, 5, 4), (20, 16, 12, lift), (33, 18, 15)], 5)),
        Case("two crossing capsules, 1 <-> 2", B([(4, 4, 8), (32, 18, 10), (32, 4, 9, lift), (4, 18, 9)], 9, to=swap_1_2())),
        Case("repeated points", B([(9, 9, 9), (9, 9, 9), (15, 12, 9), (15, 12, 9), (15, 12, 9), (9, 9, 9)], 3)),
        Case("256 points of a random walk", B(walk(DIMS), 2)),
        Case("two whole rows, r2 0", B([(0, 4, 5), (nx - 1, 4, 5), (0, 5, 5, lift), (nx - 1, 5, 5)], 0), ragged=True, count=2 * nx),
        Case("a window 100..180", B([(6, 6, 6), (30, 15, 13)], 16, window=(100, 180))),
        Case("a box that cuts the stroke", B([(2, 10, 9), (34, 10, 9)], 9, box=((10, 9, 2), (25, 22, 12)))),
        Case("uncut bytes, window 1..120", B([(6, 15, 6), (30, 6, 13)], 16, flags=_lib.BRUSH_UNCUT, window=(1, 120))),
        Case("paint the label the cuts hide", B([(8, 4, 4), (28, 17, 14)], 12, to=every(MS.HIDDEN[0]))),
        Case("dry run", B([(18, 10, 9)], 30, flags=_lib.BRUSH_DRY_RUN)),
        Case("identity table", B([(18, 10, 9)], 30, to=np.arange(256)), trivial=True),
        Case("empty box", B([(18, 10, 9)], 30, box=MS.BOXES["empty"]), trivial=True),
        Case("a box the hull misses", B([(3, 3, 3)], 4, box=((20, 10, 10), (30, 20, 18))), trivial=True),
    ]


def scene_small():
    host = RS.Host(SMALL_DIMS)
    nx, ny, nz = SMALL_DIMS
    host.labels = np.repeat(np.arange(nz, dtype=np.uint8) // 3, nx * ny)
    return host


def small_cases():
    """the strokes over the small scene"""
    from volym_amd import scene
    nx, ny, nz = SMALL_DIMS
    mid = (nx // 2, ny // 2, nz // 2)
    along_z = [(mid[0], mid[1], 0), (mid[0], mid[1], nz - 1)]

    def B(points, r2, **kw):
        return scene.Brush(points, r2, to=every(7), dims=SMALL_DIMS, **kw)

    return [Case("ball of r2 2 at the centre", B([mid], 2)), Case("capsule along z, r2 1", B(along_z, 1)),
            Case("capsule along z, r2 1, a window 64..192", B(along_z, 1, window=(64, 192)))]


def rows_shared(dims, old, new):
    """how many changed texels have y > 0 and lie in a 16-byte chunk of the linear layout whose first texel has y = 0"""
    nx, ny = dims[0], dims[1]
    at = np.flatnonzero(np.asarray(old).ravel() != np.asarray(new).ravel())
    return int((((at // nx) % ny > 0) & ((((at >> 4) << 4) // nx) % ny == 0)).sum())


def expect(host, case, brush=None):
    """the twin's (new_labels [flat], result) of `case` in the state `host` is in"""
    from volym_amd import scene
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, result = scene.brush_volume(now, host.dims, brush or case.brush, host.labels, uncut=host.vol)
    return new.ravel(), result
