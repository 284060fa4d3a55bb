"""The scenes, boxes, cut states and group tables of the measure tests, shared by tests/test_measure_host.py (which asserts on the
host twin the conditions the device tests rely on) and tests/test_gpu_measure.py (which compares the device with the twin).

Scene A is tests/test_gpu_slice.Host: 37 x 22 x 19, random density bytes 1..255, five labels in blocks.  No axis is a multiple of 4
and a row is no multiple of 16, so linear chunks wrap rows and slices.  Scene B has the same density and random labels over all 256
values: every texel breaks a run.
"""
import numpy as np

from tests.test_gpu_slice import BOX, DIMS, HIDDEN, PLANE, Host

NX, NY, NZ = DIMS

# name -> (lo, hi): the whole volume (one run), full rows of a y range (a run per z), two x ranges at odd offsets (a run per row), a
# single texel, an empty box
BOXES = {
    "whole": ((0, 0, 0), DIMS),
    "rows": ((0, 5, 2), (NX, 17, 15)),
    "x 3..8": ((3, 1, 2), (8, 20, 16)),
    "x 5..30": ((5, 3, 1), (30, 19, 18)),
    "texel": ((17, 9, 11), (18, 10, 12)),
    "empty": ((4, 4, 4), (4, 9, 9)),
}

# (name, box, plane, hidden): every cut alone, all three, each lifted again
CUTS = [("none", None, None, None), ("box", BOX, None, None), ("box lifted", None, None, None), ("plane", None, PLANE, None),
        ("plane lifted", None, None, None), ("hidden", None, None, HIDDEN), ("hidden lifted", None, None, None),
        ("all three", BOX, PLANE, HIDDEN), ("all lifted", None, None, None)]


def groups():
    """name -> group table: all in group 0, spread over 8, none, a mix"""
    mix = np.full(256, 255, np.int64)
    mix[0], mix[1], mix[2], mix[4] = 3, 0, 3, 7
    mix[100:200:3] = 5
    return {"one": np.zeros(256, np.int64), "eight": np.arange(256, dtype=np.int64) % 8, "none": np.full(256, 255, np.int64), "mix": mix}


def scene_a():
    return Host()


def scene_b():
    h = Host()
    h.labels = np.random.default_rng(23).integers(0, 256, NX * NY * NZ).astype(np.uint8)
    return h


def measures(flags=0):
    """(name, scene.Measure): every box with a rotating group table, and every group table on the whole volume"""
    from volym_amd import scene
    g = groups()
    names = list(g)
    out = [("%s / %s" % (b, names[k % 4]), scene.Measure(box, flags, g[names[k % 4]])) for k, (b, box) in enumerate(BOXES.items())]
    out += [("whole / %s" % n, scene.Measure(BOXES["whole"], flags, g[n])) for n in names[1:]]
    return out


def expect(host, m, labels=True):
    """the twin's (records, hist) for the state `host` is in; labels False: the context holds no labels of the volume's dimensions"""
    from volym_amd import scene
    lab = host.labels if labels else None
    now = scene.cut_volume(host.vol, host.dims, host.cut, lab)
    return scene.measure_volume(now, host.dims, m, labels=lab, cut=host.cut, uncut=host.vol if host.ever_cut else None)


def as_bytes(result):
    """the 36864 bytes of struct volym_measurement"""
    rec, hist = result
    return rec.tobytes() + np.ascontiguousarray(hist, np.uint64).tobytes()


def linear_runs(box, dims=DIMS):
    """(start, length) of the runs of the linear walk over `box`: a row of the box, whole rows merged per z, whole slices into one"""
    (x0, y0, z0), (x1, y1, z1) = box
    nx, ny, _ = dims
    if x0 == 0 and x1 == nx:
        if y0 == 0 and y1 == ny:
            return [(nx * ny * z0, nx * ny * (z1 - z0))]
        return [(nx * (y0 + ny * z), nx * (y1 - y0)) for z in range(z0, z1)]
    return [(x0 + nx * (y + ny * z), x1 - x0) for z in range(z0, z1) for y in range(y0, y1)]


def shared_chunks(box, dims=DIMS):
    """how many 16-byte chunks hold texels of two consecutive runs of the linear walk: the double-count trap"""
    runs = linear_runs(box, dims)
    return sum(1 for (s, n), (t, _) in zip(runs, runs[1:]) if (s + n - 1) >> 4 == t >> 4)
