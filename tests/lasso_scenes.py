"""The scenes, views, polygons and requests of the lasso tests, shared by tests/test_lasso_host.py (which pins the twin to exact
fractions and to a plain triple loop and asserts on it the conditions the device tests rely on) and tests/test_gpu_lasso.py (which
compares the device with the twin).

Scenes A and B are those of tests/relabel_scenes.py: 37 x 22 x 19, random density bytes 1..255, five labels in blocks (A) or random
labels over all 256 values (B).  No axis is a multiple of 4 and a row is no multiple of 16, so linear chunks wrap rows and slices.
The ragged scene is 97 x 80 x 71, a shell (1), a core (2) and a blob (5) in air (0).  The frame is 96 x 64.

The views are integer views of four cameras (scene.lasso_view, the library's one quantisation): the pose of the relabel tests; an eye
inside the volume, with texels behind it and D near 0; fovy 20, which leaves most of the volume off screen; a camera rolled by 30
degrees.  A Case is a request and what the host test asserts about it: `count` is what the twin changes in scene A (every case has
one; 0 only where `trivial` says the case is there for its no-op).

The small scene is that of tests/brush_scenes.py, 5 x 3 x 9: every linear chunk spans several rows and two slices.  Its two requests
(small_cases) are a triangle and its OUTSIDE twin under the default camera at a 64 x 64 frame, which looks along z.
"""
import numpy as np

from tests import free_camera_cases as FC
from tests import brush_scenes as BS
from tests import measure_scenes as MS
from tests import relabel_scenes as RS

DIMS = MS.DIMS
RAGGED_DIMS = RS.RAGGED_DIMS
SCENES = {"a": RS.scene_a, "b": RS.scene_b, "ragged": RS.scene_ragged}
W, H = 96, 64
POSE = (35.0, 20.0, 0.0)            # tests/test_gpu_relabel.POSE

CAMERAS = {
    "inside": dict(position=(0.52, 0.47, 0.55), target=(0.1, 0.3, 0.0)),
    "narrow": dict(position=(1.5, 1.1, 1.7), target=(0.5, 0.5, 0.5), fovy=20.0),
    "rolled": dict(position=(1.4, 1.2, 1.6), target=(0.5, 0.5, 0.5), up=FC._roll((1.4, 1.2, 1.6), (0.5, 0.5, 0.5), 30.0)),
}


class Case:
    def __init__(self, name, lasso, count, trivial=False):
        self.name, self.lasso, self.count, self.trivial = name, lasso, count, trivial


def every(value):
    """the table that sends every label to `value`"""
    return np.full(256, value, np.int64)


def swap_1_2():
    to = np.arange(256, dtype=np.int64)
    to[1], to[2] = 2, 1
    return to


def camera_uniforms(O, which):
    """the _lib.CameraUniforms of view `which` ("pose" or a key of CAMERAS) at W x H"""
    from volym_amd import _lib
    if which == "pose":
        u = O.benchmark_camera_uniforms(W / H, *POSE)
    else:
        u = FC.Case(which, "octant", (W, H), CAMERAS[which], FC.Z).uniforms(O)
    return _lib.CameraUniforms.from_buffer_copy(bytes(u))


def view(O, which, dims):
    from volym_amd import scene
    return scene.lasso_view(camera_uniforms(O, which), W, H, dims)


def walk(n=1024, seed=11):
    """a closed random walk of n vertices about the middle of the frame, steps of at most 3 pixels"""
    rng = np.random.default_rng(seed)
    steps = rng.integers(-3, 4, (n, 2))
    steps -= np.round(steps.sum(axis=0) / n).astype(np.int64)       # (nearly closed: the last edge is short)
    p = np.cumsum(steps, axis=0) + np.array([W // 2, H // 2])
    return [(int(x), int(y)) for x, y in p]


RECT = [(30, 10), (60, 10), (60, 50), (30, 50)]
STAR = [(48, 2), (56, 24), (90, 26), (62, 38), (74, 62), (48, 46), (22, 62), (34, 38), (6, 26), (40, 24)]
POLYGONS = {
    "rect": RECT,
    "triangle, one vertex far off screen": [(30, 8), (100000, 40), (30, 60)],
    "star": STAR,
    "bow-tie": [(10, 10), (86, 54), (86, 10), (10, 54)],
    "sliver": [(10, 20), (90, 20), (90, 20), (10, 20)],
    "walk": None,                                               # walk(): built once below
    "off screen": [(-50, -40), (-10, -40), (-10, -5), (-50, -5)],
    "frame": [(-5, -5), (W + 5, -5), (W + 5, H + 5), (-5, H + 5)],
    "one word": [(32, 12), (64, 12), (64, 52), (32, 52)],
    "a word and a pixel": [(31, 12), (64, 30), (31, 52)],
}


def cases(O, dims=DIMS):
    """the requests of the issue for a scene of `dims`; the counts are scene A's"""
    from volym_amd import _lib, scene
    a = dims == DIMS
    views = {k: view(O, k, dims) for k in ["pose"] + list(CAMERAS)}
    polys = dict(POLYGONS, walk=walk())
    nx, ny, nz = dims

    def L(poly, which="pose", depth=None, **kw):
        kw.setdefault("to", every(7))
        v = views[which]
        if depth is not None:
            v = scene.lasso_view_depth(v, *depth)
        return scene.Lasso(polys[poly], v, dims=dims, **kw)

    def n(count):
        return count if a else None

    out = [
        Case("rect", L("rect"), n(COUNTS["rect"])),
        Case("triangle, one vertex far off screen", L("triangle, one vertex far off screen"), n(COUNTS["triangle"])),
        Case("star", L("star"), n(COUNTS["star"])),
        Case("bow-tie", L("bow-tie"), n(COUNTS["bow-tie"])),
        Case("sliver (empty mask)", L("sliver"), n(0), trivial=True),
        Case("1024-vertex walk", L("walk"), n(COUNTS["walk"])),
        Case("off screen", L("off screen"), n(0), trivial=True),
        Case("frame", L("frame"), n(COUNTS["frame"])),
        Case("one word", L("one word"), n(COUNTS["one word"])),
        Case("a word and a pixel", L("a word and a pixel"), n(COUNTS["a word and a pixel"])),
        Case("star, eye inside", L("star", "inside"), n(COUNTS["star, eye inside"])),
        Case("frame, eye inside", L("frame", "inside"), n(COUNTS["frame, eye inside"])),
        Case("rect, fovy 20", L("rect", "narrow"), n(COUNTS["rect, fovy 20"])),
        Case("bow-tie, rolled", L("bow-tie", "rolled"), n(COUNTS["bow-tie, rolled"])),
        Case("star, outside", L("star", flags=_lib.LASSO_OUTSIDE), n(COUNTS["star, outside"])),
        Case("rect, fovy 20, outside", L("rect", "narrow", flags=_lib.LASSO_OUTSIDE), n(COUNTS["rect, fovy 20, outside"])),
        Case("off screen, outside", L("off screen", flags=_lib.LASSO_OUTSIDE), n(nx * ny * nz)),
        Case("walk, eye inside, outside", L("walk", "inside", flags=_lib.LASSO_OUTSIDE), n(COUNTS["walk, eye inside, outside"])),
        Case("rect, the front half", L("rect", depth=(0.0, DEPTH_MID)), n(COUNTS["rect, the front half"])),
        Case("frame, a slab one texel thick", L("frame", depth=(DEPTH_MID, DEPTH_MID + 1.0 / 37)), n(COUNTS["frame, a slab one texel thick"])),
        Case("frame, in front of the volume", L("frame", depth=(0.0, 0.15)), n(0), trivial=True),
        Case("frame, in front of the volume, outside", L("frame", depth=(0.0, 0.15), flags=_lib.LASSO_OUTSIDE), n(nx * ny * nz)),
        Case("star, a sub-box", L("star", box=((5, 3, 2), (30, 20, 15))), n(COUNTS["star, a sub-box"])),
        Case("rect, a window 100..180", L("rect", window=(100, 180)), n(COUNTS["rect, a window 100..180"])),
        Case("star, 1 <-> 2", L("star", to=swap_1_2()), n(COUNTS["star, 1 <-> 2"])),
        Case("rect, uncut bytes, window 1..120", L("rect", flags=_lib.LASSO_UNCUT, window=(1, 120)), n(COUNTS["rect, uncut bytes, window 1..120"])),
        Case("star, dry run", L("star", flags=_lib.LASSO_DRY_RUN), n(COUNTS["star"])),
        Case("rect into the label the cuts hide", L("rect", to=every(MS.HIDDEN[0])), n(COUNTS["rect into the label the cuts hide"])),
        Case("identity table", L("star", to=np.arange(256)), n(0), trivial=True),
        Case("empty box", L("star", box=MS.BOXES["empty"]), n(0), trivial=True),
    ]
    return out


SMALL_DIMS = BS.SMALL_DIMS
scene_small = BS.scene_small
rows_shared = BS.rows_shared
SMALL_FRAME = 64
SMALL_TRIANGLE = [(12, 8), (50, 30), (20, 56)]


def small_cases():
    """the requests over the small scene: the view is the library's quantisation of the default camera, host arithmetic"""
    from volym_amd import _lib, scene
    state = scene.State.with_parameters(1.0, scene.StateParameters())
    state.update()
    view = scene.lasso_view(state.camera_uniforms(), SMALL_FRAME, SMALL_FRAME, SMALL_DIMS)
    inside = scene.Lasso(SMALL_TRIANGLE, view, to=every(7), dims=SMALL_DIMS)
    return [Case("triangle", inside, None), Case("triangle, outside", inside.replace(flags=_lib.LASSO_OUTSIDE), None)]


DEPTH_MID = 1.0                     # the distance of the volume's middle along the view axis of POSE, in world units (the host test checks it)

# what the twin changes in scene A (tests/test_lasso_host.py asserts each, and that none is trivial)
COUNTS = {
    "rect": 11909, "triangle": 14753, "star": 11921, "bow-tie": 4551, "walk": 2276, "frame": 15422, "one word": 13012, "a word and a pixel": 8144,
    "star, eye inside": 1589, "frame, eye inside": 3448, "rect, fovy 20": 2157, "bow-tie, rolled": 5214, "star, outside": 3545,
    "rect, fovy 20, outside": 13309, "walk, eye inside, outside": 15083, "rect, the front half": 5028, "frame, a slab one texel thick": 533,
    "star, a sub-box": 5056, "rect, a window 100..180": 3688, "star, 1 <-> 2": 4855, "rect, uncut bytes, window 1..120": 5669,
    "rect into the label the cuts hide": 9480,
}


def expect(host, case, lasso=None):
    """the twin's (new_labels [flat], result) of `case` in the state `host` is in"""
    from volym_amd import scene
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    new, result = scene.lasso_volume(now, host.dims, lasso or case.lasso, host.labels, uncut=host.vol)
    return new.ravel(), result
