"""Scenes and helpers of the projection tests (inputs and a second march for counting ties; no expected values live here).
Shared by tests/test_project_host.py (no GPU) and tests/test_gpu_project.py."""
import numpy as np

from tests import common

SCENES = {"bonsai32": (96, 64), "cut": (72, 40)}                # name -> frame size
POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0)]                    # the benchmark pose; yawed and pitched
STEPS = (0.01, 0.0025, 0.0007)
BACKGROUND = (9, 80, 200, 33)
# every legal (mode, flags)
COMBOS = [(0, f) for f in range(8)] + [(1, f) for f in (0, 1, 4, 5)]
# crop boxes that leave macro cells empty at 4 and at 32 cells per axis (a cell at 4 per axis spans a quarter of an axis plus a voxel of slack)
BOXES = {"bonsai32": ((11, 3, 2), (29, 30, 22)), "cut": ((12, 2, 3), (38, 22, 40))}
F = np.float32

_bytes = {}


def scene_bytes(name):
    """(dims, prepared density, prepared labels) of a scene"""
    from volym_amd import scene
    if name not in _bytes:
        if name == "bonsai32":
            raw, lab = common.bonsai(32)
            dims = (32, 32, 32)
            _bytes[name] = (dims, scene.prepare_volume(raw, dims, True), scene.prepare_volume(lab, dims, True))
        else:
            raw, lab = common.bonsai(64)
            cut = lambda a: np.ascontiguousarray(scene.prepare_volume(a, (64, 64, 64), True).reshape(64, 64, 64)[4:60, 22:46, 12:52]).ravel()
            _bytes[name] = ((40, 24, 56), cut(raw), cut(lab))
    return _bytes[name]


def palette():
    pal = np.random.default_rng(5).integers(0, 256, (256, 4)).astype(np.uint8)
    pal[3, 3], pal[4, 3] = 0, 255
    return pal


def empty_cells(vol, dims, mc):
    """how many cells of the mc^3 grid have maximum 0: a cell spans the voxels floor(c * n / mc) - 1 .. ceil((c + 1) * n / mc) + 1 of an
    axis, clipped to it (csrc/scene_kernels.h)"""
    v = np.asarray(vol).reshape(dims[2], dims[1], dims[0])
    spans = [[(max(c * n // mc - 1, 0), min(((c + 1) * n + mc - 1) // mc + 1, n)) for c in range(mc)] for n in dims]
    occupied = np.array([[[v[z0:z1, y0:y1, x0:x1].any() for x0, x1 in spans[0]] for y0, y1 in spans[1]] for z0, z1 in spans[2]])
    return int((~occupied).sum())


def tie_fraction(vol, dims, cam, w, h, step, rec):
    """the fraction of the hit rays whose maximum is attained at two or more samples: the samples marched once more, counted
    against the records' max"""
    from volym_amd import scene
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    o, d, t_entry, t_exit, hit = scene.project_rays(cam, w, h, gx.ravel(), gy.ravel())
    best = rec["max"].ravel().astype(np.int64)
    at_max = np.zeros(hit.size, np.int64)
    nx, ny, nz = dims
    idx, k = np.flatnonzero(hit), 0
    while idx.size:
        t = t_entry[idx] + F(k) * F(step)
        keep = t < t_exit[idx]
        idx, t = idx[keep], t[keep]
        ix, iy, iz = scene._project_texels(o, d[idx], t, dims)
        at_max[idx] += vol[ix + nx * (iy + ny * iz)] == best[idx]
        k += 1
    return float((at_max[hit] >= 2).mean())
