"""Segment visibility on the device (volym_set_segment_visibility): the parts that need no GPU -- the NumPy statement of the
definition, validation, the rule that picks the boxes an edit rewrites, the library's answers without a context, and the
oracle's word that hidden importances must be zeroed along with the density."""
import ctypes as C

import numpy as np
import pytest

GRID = (5, 4, 3)          # nx, ny, nz of the exhaustive box test
MAX_BOXES = 8             # VOLYM_VISIBILITY_MAX_BOXES


def test_hide_segments_is_the_mask(volym_lib):
    from volym_amd import scene
    rng = np.random.default_rng(11)
    dims = (13, 9, 7)
    n = 13 * 9 * 7
    vol = rng.integers(1, 256, size=n).astype(np.uint8)
    labels = rng.integers(0, 6, size=n).astype(np.uint8)
    for hidden in ([], [2], [0], [1, 4], [0, 1, 2, 3, 4, 5], [200], list(range(1, 40)), list(range(3, 256))):
        visible = np.ones(256, np.uint8)
        visible[hidden] = 0
        want = np.array([v if l not in hidden else 0 for v, l in zip(vol.tolist(), labels.tolist())], np.uint8)
        got = scene.hide_segments(vol, labels, visible)
        assert got.dtype == np.uint8 and got.shape == vol.shape and np.array_equal(got, want), hidden
        assert got is not vol and vol.min() >= 1                        # a copy: the input keeps its bytes
        assert np.array_equal(scene.hide_segments(vol, labels, visible.astype(bool)), want)
        assert np.array_equal(scene.hide_segments(vol, labels, (visible * 7).tolist()), want)      # nonzero means visible
        # commutes with the crop box
        lo, hi = (1, 2, 3), (12, 9, 5)
        a = scene.crop_volume(scene.hide_segments(vol, labels, visible), dims, lo, hi)
        b = scene.hide_segments(scene.crop_volume(vol, dims, lo, hi), labels, visible)
        assert np.array_equal(a, b), hidden
        assert np.array_equal(scene.visibility_mask(hidden), visible)
    with pytest.raises(ValueError):
        scene.hide_segments(vol, labels[:-1], np.ones(256, np.uint8))


def test_check_segment_visibility(volym_lib):
    from volym_amd import scene
    v = scene.check_segment_visibility([1] * 256)
    assert v.dtype == np.uint8 and v.shape == (256,) and v.all()
    v = scene.check_segment_visibility(np.arange(256))
    assert v[0] == 0 and v[1:].all() and v.max() == 1                   # 0 / 1 whatever the nonzero value
    assert not scene.check_segment_visibility(np.zeros(256, bool)).any()
    for bad in ([1] * 255, [1] * 257, np.ones((16, 16), np.uint8), "1" * 256, "1" * 3, None, 1, ["a"] * 256, [None] * 256,
                np.ones(256, np.complex64)):
        with pytest.raises(ValueError):
            scene.check_segment_visibility(bad)
    with pytest.raises(ValueError):
        scene.visibility_mask([256])


def _stats(labels, dims):
    """Voxel count and texel AABB (hi inclusive) per label value, as the volym_set_labels pass reports them."""
    nx, ny, nz = dims
    lab = labels.reshape(nz, ny, nx)
    counts = np.zeros(256, np.uint64)
    boxes = np.zeros((256, 6), np.int32)
    boxes[:, :3] = np.iinfo(np.int32).max
    boxes[:, 3:] = -1
    for l in np.unique(lab):
        z, y, x = np.nonzero(lab == l)
        counts[l] = x.size
        boxes[l] = (x.min(), y.min(), z.min(), x.max(), y.max(), z.max())
    return counts, boxes


def _call(flipped, counts, boxes, lo, hi):
    from volym_amd import _lib
    u3 = C.c_uint32 * 3
    out = (C.c_uint32 * (6 * MAX_BOXES))()
    n = C.c_uint32(99)
    f = np.ascontiguousarray(flipped, np.uint8)
    rc = _lib.lib().volym_visibility_boxes(f.ctypes.data_as(C.POINTER(C.c_uint8)), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           boxes.ctypes.data_as(C.POINTER(C.c_int32)), u3(*lo), u3(*hi), out, C.byref(n))
    assert rc == _lib.OK
    assert n.value <= MAX_BOXES
    return [tuple(out[6 * i:6 * i + 6]) for i in range(n.value)]


def test_visibility_boxes_cover_the_flipped_texels(volym_lib):
    """Label volumes on a 5 x 4 x 3 grid, every crop box of the grid (the empty ones included) and sets of flipped labels, against
    brute force: every texel of a flipped label inside the crop box lies in a returned box; the boxes lie inside the crop box,
    are not empty and are at most VOLYM_VISIBILITY_MAX_BOXES; a label without voxels adds nothing; and while there is room the
    boxes together hold no more texels than the flipped labels' own boxes do (joining never reads more than not joining)."""
    nx, ny, nz = GRID
    rng = np.random.default_rng(2)
    spans = [[(a, b) for a in range(n + 1) for b in range(a, n + 1)] for n in GRID]
    crops = [((x[0], y[0], z[0]), (x[1], y[1], z[1])) for x in spans[0] for y in spans[1] for z in spans[2]]
    assert len(crops) == 21 * 15 * 10
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    volumes = [
        rng.integers(0, 4, size=nx * ny * nz).astype(np.uint8),                               # 4 labels, all boxes overlap
        (x // 2 + 3 * (y // 2) + 6 * (z // 2)).astype(np.uint8).ravel(),                      # 12 blocks: disjoint boxes, more than 8
        np.where((x == 2) & (y == 1), 7, np.where(z == 0, 1, 250)).astype(np.uint8).ravel(),  # nested and thin
        np.arange(nx * ny * nz, dtype=np.uint8),                                              # 60 labels of one texel each
    ]
    checked = 0
    for labels in volumes:
        counts, boxes = _stats(labels, GRID)
        present = [int(l) for l in np.nonzero(counts)[0]]
        subsets = [[l] for l in present[:6]] + [present, present[::2], present[1::3], present[:9], present + [255, 99]]
        lab3 = labels.reshape(nz, ny, nx)
        for flipped_labels in subsets:
            flipped = np.zeros(256, np.uint8)
            flipped[flipped_labels] = 1
            is_flipped = flipped[lab3] != 0
            for lo, hi in crops[::3] if len(present) > 20 else crops:
                got = _call(flipped, counts, boxes, lo, hi)
                inside = np.zeros((nz, ny, nx), bool)
                inside[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
                covered = np.zeros((nz, ny, nx), bool)
                for b in got:
                    assert all(lo[a] <= b[a] < b[3 + a] <= hi[a] for a in range(3)), (flipped_labels, lo, hi, b)
                    covered[b[2]:b[5], b[1]:b[4], b[0]:b[3]] = True
                assert not (is_flipped & inside & ~covered).any(), (flipped_labels, lo, hi, got)
                own = 0
                cut = 0
                for l in flipped_labels:
                    if counts[l] == 0:
                        continue
                    e = [max(0, min(int(boxes[l][3 + a]) + 1, hi[a]) - max(int(boxes[l][a]), lo[a])) for a in range(3)]
                    if min(e) > 0:
                        own += e[0] * e[1] * e[2]
                        cut += 1
                if cut <= MAX_BOXES:
                    assert sum((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]) for b in got) <= own, (flipped_labels, lo, hi, got)
                if cut == 0:
                    assert got == []
                if cut == 1:
                    assert len(got) == 1
                checked += 1
    assert checked >= 40000


def test_visibility_boxes_cost_rule(volym_lib):
    """The cases the rule is for, at the size of a real volume."""
    from volym_amd import _lib
    counts = np.zeros(256, np.uint64)
    boxes = np.zeros((256, 6), np.int32)
    full = ((0, 0, 0), (1024, 1024, 1024))
    # a small segment inside the box of a large one: one launch over the large box, not two
    counts[2], boxes[2] = 5, (100, 100, 100, 899, 899, 899)
    counts[3], boxes[3] = 5, (400, 400, 400, 449, 449, 449)
    f = np.zeros(256, np.uint8)
    f[[2, 3]] = 1
    assert _call(f, counts, boxes, *full) == [(100, 100, 100, 900, 900, 900)]
    # two small segments in opposite corners stay two launches: their hull is the whole volume
    counts[4], boxes[4] = 5, (0, 0, 0, 49, 49, 49)
    counts[5], boxes[5] = 5, (960, 960, 960, 1023, 1023, 1023)
    f[:] = 0
    f[[4, 5]] = 1
    assert sorted(_call(f, counts, boxes, *full)) == [(0, 0, 0, 50, 50, 50), (960, 960, 960, 1024, 1024, 1024)]
    # ... cut to the crop box, and a label outside it costs nothing
    assert _call(f, counts, boxes, (0, 0, 0), (1024, 1024, 512)) == [(0, 0, 0, 50, 50, 50)]
    assert _call(f, counts, boxes, (10, 0, 0), (10, 1024, 1024)) == []
    # 200 labels scattered over the volume: at most eight launches, all of them covered
    rng = np.random.default_rng(4)
    counts[:] = 0
    for l in range(200):
        p = rng.integers(0, 1000, 3)
        counts[l], boxes[l] = 1, (*p, *(p + rng.integers(1, 24, 3)))
    f[:] = 0
    f[:200] = 1
    got = _call(f, counts, boxes, *full)
    assert 1 <= len(got) <= MAX_BOXES
    for l in range(200):
        assert any(all(b[a] <= boxes[l][a] and boxes[l][3 + a] < b[3 + a] for a in range(3)) for b in got), l
    # nothing flipped, or only labels without voxels
    f[:] = 0
    assert _call(f, counts, boxes, *full) == []
    f[[250, 251]] = 1
    assert _call(f, counts, boxes, *full) == []
    # invalid input
    u3 = C.c_uint32 * 3
    out, n = (C.c_uint32 * 48)(), C.c_uint32(0)
    fp, cp, bp = f.ctypes.data_as(C.POINTER(C.c_uint8)), counts.ctypes.data_as(C.POINTER(C.c_uint64)), boxes.ctypes.data_as(C.POINTER(C.c_int32))
    L = _lib.lib()
    assert L.volym_visibility_boxes(None, cp, bp, u3(0, 0, 0), u3(1, 1, 1), out, C.byref(n)) == _lib.E_INVALID
    assert L.volym_visibility_boxes(fp, cp, bp, u3(2, 0, 0), u3(1, 1, 1), out, C.byref(n)) == _lib.E_INVALID
    assert L.volym_visibility_boxes(fp, cp, bp, u3(0, 0, 0), u3(1, 1, 1), out, None) == _lib.E_INVALID


def test_library_without_a_context(volym_lib):
    """NULL context: VOLYM_E_INVALID from all three calls; the symbols are exported and bound."""
    from volym_amd import _lib, mgpu
    L = _lib.lib()
    table = (C.c_uint8 * 256)(*([1] * 256))
    assert L.volym_set_segment_visibility(None, table) == _lib.E_INVALID
    assert L.volym_get_segment_visibility(None, table) == _lib.E_INVALID
    assert mgpu.lib().volym_mgpu_set_segment_visibility(None, table) == _lib.E_INVALID
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("volym_set_segment_visibility", "volym_get_segment_visibility", "volym_visibility_boxes", "volym_mgpu_set_segment_visibility"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES or name in mgpu.SIGNATURES, name
    assert L.volym_abi_version() == 2


def _ragged():
    """The 97 x 80 x 71 scene of tests/test_gpu_crop_box.py::_ragged: a shell (label 1) with a core (2) and a blob at a corner (5)."""
    dims = (97, 80, 71)
    zz, yy, xx = np.meshgrid(*(np.linspace(0.0, 1.0, d) for d in dims[::-1]), indexing="ij")
    r = np.sqrt((xx - 0.5) ** 2 + (yy - 0.5) ** 2 + (zz - 0.5) ** 2)
    shell = np.abs(r - 0.38) < 0.06
    core = np.sqrt((xx - 0.45) ** 2 + (yy - 0.55) ** 2 + (zz - 0.5) ** 2) < 0.13
    blob = np.sqrt((xx - 0.85) ** 2 + (yy - 0.2) ** 2 + (zz - 0.8) ** 2) < 0.1
    rng = np.random.default_rng(5)
    vol = (np.where(shell, 110, 0) + np.where(core, 200, 0) + np.where(blob, 150, 0) + rng.integers(0, 6, shell.shape)).clip(0, 255)
    labels = np.where(blob, 5, np.where(core, 2, np.where(shell, 1, 0)))
    return dims, vol.astype(np.uint8).ravel(), labels.astype(np.uint8).ravel()


def test_hidden_importances_must_be_zeroed(oracle, volym_lib):
    """The semantic pin, on the oracle alone: hiding the important core of the ragged scene with its importances zeroed gives a
    different picture than zeroing its density alone (the hidden core would go on suppressing the shell in front of it): at
    least 1 % of the pixels with the cone check.  A twin test cannot pass with the wrong rule."""
    from volym_amd import scene
    W, H = 96, 64
    dims, vol, labels = _ragged()
    table = np.zeros(256, np.uint8)
    table[2] = 255
    imp = table[labels]
    visible = scene.visibility_mask([2])
    hvol, himp = scene.hide_segments(vol, labels, visible), scene.hide_segments(imp, labels, visible)
    assert not himp.any() and hvol.any()
    cam = oracle.benchmark_camera_uniforms(W / H, 35.0, 20.0, 0.0)
    lut = oracle.tf_default_lut()
    for name, least, kw in (("cone", 0.01, dict(use_cone_importance_check=1)), ("straight", 0.0, dict())):
        par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01, use_importance_rendering=1,
                                     importance_check_ahead_steps=15, **kw)
        right = oracle.render(hvol, himp, dims, lut, cam, par, W, H, want_f32=False)[1]
        density_only = oracle.render(hvol, imp, dims, lut, cam, par, W, H, want_f32=False)[1]
        differ = int((right != density_only).any(axis=-1).sum())
        print("%s check: zeroing the hidden importances changes %d of %d pixels" % (name, differ, W * H))
        assert differ > least * W * H, (name, differ)
