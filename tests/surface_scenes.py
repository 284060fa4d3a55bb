"""The scenes, boxes, cut states, select tables and thresholds of the surface tests, shared by tests/test_surface_host.py (which
asserts on the host twin the conditions the device tests rely on) and tests/test_gpu_surface.py (which compares the device with the
twin).  Scenes, boxes and cut states are those of tests/measure_scenes.py: Scene A is 37 x 22 x 19 with random density bytes 1..255
and five labels in blocks, Scene B the same density under random labels over all 256 values.
"""
import functools

import numpy as np

from tests import measure_scenes as M

DIMS, NX, NY, NZ = M.DIMS, M.NX, M.NY, M.NZ
BOX, PLANE, HIDDEN = M.BOX, M.PLANE, M.HIDDEN
# the boxes of the measure tests, and one of 16 x 16 = 256 rows: an exact multiple of the scan's block
BOXES = dict(M.BOXES, **{"256 rows": ((2, 3, 1), (35, 19, 17))})
CUTS = M.CUTS
scene_a, scene_b = M.scene_a, M.scene_b
MIN_BYTES = (1, 128, 255)

# Rows longer than a wave, on the 97 x 80 x 71 scene of tests/test_gpu_crop_box._ragged (a shell, a core and a blob, labels 1, 2, 5,
# noise bytes 0..5 elsewhere): a wave walks a row in chunks of 64 texels and carries a solid run from one chunk into the next.
# name -> (lo, hi): two chunks with a ragged second one, exactly one chunk, one chunk and a single texel, a first texel then a full
# chunk and a single texel, and 94 texels from an odd offset
LONG_DIMS = (97, 80, 71)
LONG_BOXES = {
    "97": ((0, 0, 0), LONG_DIMS),
    "64": ((0, 5, 3), (64, 70, 60)),
    "65": ((10, 0, 8), (75, 80, 40)),
    "66 from 1": ((1, 2, 0), (67, 79, 71)),
    "94 from 3": ((3, 1, 1), (97, 80, 70)),
}

# More rows than one workgroup of the offset scan's second phase has threads times the rows of a block: 4 x 257 x 256 of noise, and a
# box of 257 x 256 = 65792 rows, 257 scan blocks, so that a thread of that one workgroup owns two block sums, not one.
# The scan is one for the surface and the components pass (box_pass.hip); both walk this box.
SCAN_DIMS = (4, 257, 256)
SCAN_BOX = ((1, 0, 0), (3, 257, 256))
SCAN_MIN_BYTE, SCAN_LABELS = 128, (1, 2)


def scan_scene():
    """(dims, vol, labels): random density bytes 0..255 and, from the same generator next, labels 0..3"""
    rng = np.random.default_rng(20261020)
    n = SCAN_DIMS[0] * SCAN_DIMS[1] * SCAN_DIMS[2]
    vol = rng.integers(0, 256, n, dtype=np.uint8)
    return SCAN_DIMS, vol, rng.integers(0, 4, n, dtype=np.uint8)


@functools.lru_cache(None)
def scan_surface():
    """(scene.Surface over SCAN_BOX, the twin's (summary, faces) of scan_scene): computed once, left unchanged"""
    from volym_amd import scene
    dims, vol, labels = scan_scene()
    s = scene.Surface(SCAN_BOX, 0, SCAN_MIN_BYTE, scene.surface_select(SCAN_LABELS))
    return s, scene.surface_volume(vol, dims, s, labels=labels)


def selects():
    """name -> select table: every label, none, one label, a mix"""
    mix = np.zeros(256, np.int64)
    mix[0], mix[1], mix[4] = 1, 7, 255
    mix[100:200:3] = 1
    one = np.zeros(256, np.int64)
    one[3] = 1
    return {"all": np.ones(256, np.int64), "none": np.zeros(256, np.int64), "one": one, "mix": mix}


def every_surface(flags=0):
    """(name, scene.Surface): every box with every select table at every min_byte"""
    from volym_amd import scene
    return [("%s / %s / %d" % (b, n, m), scene.Surface(box, flags, m, sel)) for b, box in BOXES.items() for n, sel in selects().items() for m in MIN_BYTES]


def surfaces(flags=0):
    """(name, scene.Surface): the short list for every cut state -- every box with a rotating select table and min_byte, and the
    whole volume with every select table and every min_byte"""
    from volym_amd import scene
    sel = selects()
    turn = ("mix", "all", "one")
    out = [("%s / %s / %d" % (b, turn[k % 3], MIN_BYTES[(k // 2) % 3]), scene.Surface(box, flags, MIN_BYTES[(k // 2) % 3], sel[turn[k % 3]]))
           for k, (b, box) in enumerate(BOXES.items())]
    out += [("whole / %s / 128" % n, scene.Surface(BOXES["whole"], flags, 128, sel[n])) for n in sel]
    out += [("whole / all / %d" % m, scene.Surface(BOXES["whole"], flags, m, sel["all"])) for m in MIN_BYTES if m != 128]
    return out


def expect(host, s, labels=True):
    """the twin's (summary, faces) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.surface_volume(now, host.dims, s, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 24584 bytes of struct volym_surface_summary, then the face records"""
    summary, faces = result
    return summary.tobytes() + np.ascontiguousarray(faces).tobytes()


def rows(box):
    """rows of a request's box: pairs (y, z); an empty box has none"""
    (x0, y0, z0), (x1, y1, z1) = box
    return (y1 - y0) * (z1 - z0) if x1 > x0 and y1 > y0 and z1 > z0 else 0


def face_keys(faces):
    """the canonical sort key of every record: ((z * 4096 + y) * 4096 + x) * 8 + dir"""
    f = np.asarray(faces)
    return ((f["z"].astype(np.int64) * 4096 + f["y"]) * 4096 + f["x"]) * 8 + f["dir"]
