"""Crop box on the device (volym_set_crop_box): the parts that need no GPU -- the slab arithmetic of an edit, the NumPy
statement of the definition, validation and rounding, and the library's answers without a context."""
import ctypes as C
import itertools

import numpy as np
import pytest

GRID = (5, 4, 3)          # nx, ny, nz of the exhaustive slab test


def _boxes(dims):
    """Every box lo <= hi <= n of a grid, the empty ones (lo == hi on some axis) included."""
    spans = [[(a, b) for a in range(n + 1) for b in range(a, n + 1)] for n in dims]
    return [((x[0], y[0], z[0]), (x[1], y[1], z[1])) for x in spans[0] for y in spans[1] for z in spans[2]]


def _mask(lo, hi, dims):
    """The texels of a box as one Python int, bit (z * ny + y) * nx + x (NumPy makes the set, the int makes it fast to combine)."""
    m = np.zeros(dims[::-1], bool)
    m[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    return int.from_bytes(np.packbits(m.ravel(), bitorder="little").tobytes(), "little")


def test_crop_slabs_cover_the_symmetric_difference(volym_lib):
    """Every ordered pair of the 900 non-empty boxes of a 5 x 4 x 3 grid, plus pairs with an empty box on either side or both
    (the 2250 empty boxes thinned by a fixed stride): the slabs' union holds the symmetric difference, every slab
    lies inside the volume and is not empty, at most six, none when the boxes are equal."""
    from volym_amd import _lib
    fn = _lib.lib().volym_crop_slabs
    u3 = C.c_uint32 * 3
    boxes = _boxes(GRID)
    solid = [b for b in boxes if all(l < h for l, h in zip(*b))]
    empty = [b for b in boxes if not all(l < h for l, h in zip(*b))]
    # lo <= hi per axis: (n + 1)(n + 2) / 2 spans, n + 1 of them empty: 21 * 15 * 10 boxes, 15 * 10 * 6 with lo < hi on every axis
    assert len(boxes) == 21 * 15 * 10 and len(solid) == 900
    # all 900 x 900 ordered pairs of non-empty boxes, and the empty boxes (thinned by a fixed stride) against every box
    arr = {b: (u3(*b[0]), u3(*b[1])) for b in boxes}
    mask = {b: _mask(b[0], b[1], GRID) for b in boxes}
    by_extent = {(b[0] + b[1]): mask[b] for b in boxes}
    slabs = (C.c_uint32 * 36)()
    n = C.c_uint32(0)
    pairs = itertools.chain(itertools.product(solid, solid), itertools.product(empty[::7], solid), itertools.product(solid, empty[::7]),
                            itertools.product(empty[::7], empty[::5]))
    checked = 0
    for old, new in pairs:
        assert fn(arr[old][0], arr[old][1], arr[new][0], arr[new][1], slabs, C.byref(n)) == _lib.OK
        k = n.value
        assert k <= 6, (old, new, k)
        union = 0
        for i in range(k):
            s = tuple(slabs[6 * i:6 * i + 6])
            assert all(s[a] < s[3 + a] <= GRID[a] for a in range(3)), (old, new, s)
            union |= by_extent[s]
        diff = mask[old] ^ mask[new]
        assert diff & ~union == 0, (old, new, [tuple(slabs[6 * i:6 * i + 6]) for i in range(k)])
        if old == new:
            assert k == 0, (old, k)
        checked += 1
    assert checked >= 810000


def test_crop_slabs_one_face_is_one_thin_slab(volym_lib):
    """Dragging one face touches the texels between the two planes and nothing else: the cost argument of the incremental edit."""
    from volym_amd import _lib
    u3 = C.c_uint32 * 3
    slabs = (C.c_uint32 * 36)()
    n = C.c_uint32(0)
    rc = _lib.lib().volym_crop_slabs(u3(0, 0, 0), u3(1024, 1024, 1024), u3(0, 0, 0), u3(1024, 1024, 1016), slabs, C.byref(n))
    assert rc == _lib.OK and n.value == 1
    assert tuple(slabs[0:6]) == (0, 0, 1016, 1024, 1024, 1024)
    rc = _lib.lib().volym_crop_slabs(u3(8, 0, 0), u3(1024, 1024, 1024), u3(16, 0, 0), u3(1024, 1024, 1024), slabs, C.byref(n))
    assert rc == _lib.OK and n.value == 1 and tuple(slabs[0:6]) == (8, 0, 0, 16, 1024, 1024)
    # invalid input
    assert _lib.lib().volym_crop_slabs(u3(2, 0, 0), u3(1, 1, 1), u3(0, 0, 0), u3(1, 1, 1), slabs, C.byref(n)) == _lib.E_INVALID
    assert _lib.lib().volym_crop_slabs(None, u3(1, 1, 1), u3(0, 0, 0), u3(1, 1, 1), slabs, C.byref(n)) == _lib.E_INVALID


def test_crop_volume_is_the_mask(volym_lib):
    from volym_amd import scene
    rng = np.random.default_rng(3)
    dims = (13, 9, 7)
    vol = rng.integers(1, 256, size=13 * 9 * 7).astype(np.uint8)
    for lo, hi in [((0, 0, 0), dims), ((1, 2, 3), (12, 9, 5)), ((4, 4, 4), (5, 5, 5)), ((3, 0, 0), (3, 9, 7)), ((0, 0, 6), (13, 9, 7))]:
        z, y, x = np.meshgrid(np.arange(7), np.arange(9), np.arange(13), indexing="ij")
        inside = (x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2])
        want = np.where(inside.ravel(), vol, 0).astype(np.uint8)
        got = scene.crop_volume(vol, dims, lo, hi)
        assert got.dtype == np.uint8 and got.shape == vol.shape and np.array_equal(got, want), (lo, hi)
        assert got is not vol and vol.min() >= 1                       # a copy: the input keeps its bytes


def test_check_crop_box_and_rounding(volym_lib):
    from volym_amd import scene
    dims = (64, 32, 10)
    assert scene.check_crop_box((0, 0, 0), dims, dims) == ((0, 0, 0), dims)
    assert scene.check_crop_box([5, 5, 5], [5, 6, 7], dims) == ((5, 5, 5), (5, 6, 7))      # empty on x: valid
    for lo, hi in [((3, 0, 0), (2, 32, 10)), ((0, 0, 0), (65, 32, 10)), ((0, 0, 0), (64, 32, 11)), ((0, 0), (64, 32, 10)),
                   ((0, 0, 0), (64, 32, 10, 1)), ((-1, 0, 0), (64, 32, 10)), (0, (64, 32, 10))]:
        with pytest.raises(ValueError):
            scene.check_crop_box(lo, hi, dims)
    # texel = floor(p * n + 0.5) clamped to [0, n]
    assert scene.crop_box_texels((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims) == ((0, 0, 0), dims)
    assert scene.crop_box_texels((-0.5, 0.0, 0.0), (1.5, 1.0, 1.0), dims) == ((0, 0, 0), dims)
    # a half-texel boundary: p * n = k + 0.5 rounds up to k + 1, anything below it down to k
    lo, hi = scene.crop_box_texels((10.5 / 64, 0.0, 0.0), (np.nextafter(20.5 / 64, 0.0), 1.0, 0.25), dims)
    assert lo == (11, 0, 0) and hi == (20, 32, 3)                      # 0.25 * 10 + 0.5 = 3.0 -> 3
    assert scene.crop_box_texels((0.0, 0.0, 0.0), (1.0 / 3.0, 0.5, 0.5), dims)[1] == (21, 16, 5)
    with pytest.raises(ValueError):
        scene.crop_box_texels((0.6, 0.0, 0.0), (0.4, 1.0, 1.0), dims)   # lo > hi after rounding


def test_library_without_a_context(volym_lib):
    """NULL context: VOLYM_E_INVALID, as every other call answers; the symbols and their multi-GPU forward are exported."""
    from volym_amd import _lib, mgpu
    L = _lib.lib()
    u3 = C.c_uint32 * 3
    assert L.volym_set_crop_box(None, u3(0, 0, 0), u3(1, 1, 1)) == _lib.E_INVALID
    assert L.volym_get_crop_box(None, u3(), u3()) == _lib.E_INVALID
    assert mgpu.lib().volym_mgpu_set_crop_box(None, u3(0, 0, 0), u3(1, 1, 1)) == _lib.E_INVALID
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("volym_set_crop_box", "volym_get_crop_box", "volym_crop_slabs", "volym_mgpu_set_crop_box"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES or name in mgpu.SIGNATURES, name
