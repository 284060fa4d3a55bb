"""Oblique clip plane on the device (volym_set_clip_plane): the parts that need no GPU -- the box an edit walks, the NumPy
statement of the definition, validation and the unit-cube-to-integer rule, why the importances must be clipped with the
density (pinned on the oracle), and the library's answers without a context."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import common

GRID = (5, 4, 3)          # nx, ny, nz of the exhaustive box test
NONE = ((0, 0, 0), 0)


def _planes():
    ns = [n for n in itertools.product((-2, -1, 0, 1, 3), (-1, 0, 2), (-3, 0, 1)) if n != (0, 0, 0)]
    return [(n, d) for n in ns for d in (-3, 0, 2, 5)] + [NONE]


def _bits(m):
    return int.from_bytes(np.packbits(np.ascontiguousarray(m).ravel(), bitorder="little").tobytes(), "little")


def _kept(plane, dims):
    (a, b, c), d = plane
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    return a * x + b * y + c * z <= d


def _box_bits(dims):
    """{(x0, y0, z0, x1, y1, z1): the texels of that box as one Python int} for every non-empty box of the grid"""
    out = {}
    spans = [[(a, b) for a in range(n) for b in range(a + 1, n + 1)] for n in dims]
    for x, y, z in itertools.product(*spans):
        m = np.zeros(dims[::-1], bool)
        m[z[0]:z[1], y[0]:y[1], x[0]:x[1]] = True
        out[(x[0], y[0], z[0], x[1], y[1], z[1])] = _bits(m)
    return out


def test_clip_plane_box_exhaustive(volym_lib):
    """All 177 x 177 ordered pairs of planes over the 5 x 4 x 3 grid and two sub-boxes of it: the box lies in [lo, hi) and is
    not empty, covers every texel the planes classify differently (brute force), is absent exactly when there is no such
    texel, and no outer slice of it is one over which both predicates are constant and equal."""
    from volym_amd import _lib
    fn = _lib.lib().volym_clip_plane_box
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3
    planes = _planes()
    assert len(planes) == 177
    kept = {p: _bits(_kept(p, GRID)) for p in planes}
    arr = {p: i3(*p[0]) for p in planes}
    bits = _box_bits(GRID)
    box, n = (C.c_uint32 * 6)(), C.c_uint32(0)
    checked = with_box = alike_not_equal = 0
    for lo, hi in (((0, 0, 0), GRID), ((1, 1, 0), (4, 3, 3)), ((2, 0, 1), (5, 4, 2))):
        region = bits[lo + hi]
        clo, chi = u3(*lo), u3(*hi)
        for old, new in itertools.product(planes, planes):
            assert fn(arr[old], old[1], arr[new], new[1], clo, chi, box, C.byref(n)) == _lib.OK
            diff = (kept[old] ^ kept[new]) & region
            checked += 1
            if diff == 0:
                assert n.value == 0, (lo, hi, old, new, tuple(box))
                alike_not_equal += old != new
                continue
            assert n.value == 1, (lo, hi, old, new)
            b = tuple(box)
            assert all(lo[a] <= b[a] < b[3 + a] <= hi[a] for a in range(3)), (lo, hi, old, new, b)
            assert diff & ~bits[b] == 0, (lo, hi, old, new, b)
            for a in range(3):
                for at in (b[a], b[3 + a] - 1):
                    s = list(b)
                    s[a], s[3 + a] = at, at + 1
                    s = bits[tuple(s)]
                    ko, kn = kept[old] & s, kept[new] & s
                    assert not ((ko == 0 and kn == 0) or (ko == s and kn == s)), (lo, hi, old, new, b, a, at)
            with_box += 1
    assert checked == 3 * 31329
    assert with_box > 30000 and alike_not_equal > 1000        # both kinds of pair are there in numbers


def test_clip_plane_box_one_step_is_one_layer(volym_lib):
    """Dragging an axis-aligned plane by one step touches one layer of texels: the cost argument of the incremental edit."""
    from volym_amd import _lib
    fn = _lib.lib().volym_clip_plane_box
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3
    box, n = (C.c_uint32 * 6)(), C.c_uint32(0)
    lo, hi = u3(0, 0, 0), u3(1024, 1024, 1024)
    assert fn(i3(0, 0, 1), 500, i3(0, 0, 1), 501, lo, hi, box, C.byref(n)) == _lib.OK
    assert n.value == 1 and tuple(box) == (0, 0, 501, 1024, 1024, 502)
    assert fn(i3(-4096, 0, 0), -4096 * 300, i3(-4096, 0, 0), -4096 * 299, lo, hi, box, C.byref(n)) == _lib.OK
    assert n.value == 1 and tuple(box) == (299, 0, 0, 300, 1024, 1024)
    # from no plane to an axis-aligned one: the half that goes
    assert fn(i3(0, 0, 0), 0, i3(0, 1, 0), 99, lo, hi, box, C.byref(n)) == _lib.OK
    assert n.value == 1 and tuple(box) == (0, 100, 0, 1024, 1024, 1024)
    # an oblique plane moved by one step: a band, cut to the volume
    assert fn(i3(1, 1, 0), 100, i3(1, 1, 0), 101, lo, hi, box, C.byref(n)) == _lib.OK
    assert n.value == 1 and tuple(box) == (0, 0, 0, 102, 102, 1024)
    # the same texels kept by different coefficients: nothing to do
    assert fn(i3(3, 0, 0), 2, i3(1, 0, 0), 0, lo, hi, box, C.byref(n)) == _lib.OK and n.value == 0
    assert fn(i3(1, 2, 3), 7, i3(1, 2, 3), 7, lo, hi, box, C.byref(n)) == _lib.OK and n.value == 0
    # an empty [lo, hi)
    assert fn(i3(0, 0, 1), 5, i3(0, 0, 1), 9, u3(3, 3, 3), u3(3, 9, 9), box, C.byref(n)) == _lib.OK and n.value == 0


def test_clip_plane_box_invalid(volym_lib):
    from volym_amd import _lib
    fn = _lib.lib().volym_clip_plane_box
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3
    box, n = (C.c_uint32 * 6)(), C.c_uint32(0)
    lo, hi, p = u3(0, 0, 0), u3(8, 8, 8), i3(1, 0, 0)
    assert fn(p, 1, i3(4096, -4096, 0), 2, lo, hi, box, C.byref(n)) == _lib.OK
    for bad in (lambda: fn(None, 1, p, 2, lo, hi, box, C.byref(n)),
                lambda: fn(p, 1, None, 2, lo, hi, box, C.byref(n)),
                lambda: fn(p, 1, p, 2, None, hi, box, C.byref(n)),
                lambda: fn(p, 1, p, 2, lo, None, box, C.byref(n)),
                lambda: fn(p, 1, p, 2, lo, hi, None, C.byref(n)),
                lambda: fn(p, 1, p, 2, lo, hi, box, None),
                lambda: fn(i3(4097, 0, 0), 1, p, 2, lo, hi, box, C.byref(n)),
                lambda: fn(p, 1, i3(0, -4097, 0), 2, lo, hi, box, C.byref(n)),
                lambda: fn(i3(0, 0, 0), 1, p, 2, lo, hi, box, C.byref(n)),
                lambda: fn(p, 1, i3(0, 0, 0), -1, lo, hi, box, C.byref(n)),
                lambda: fn(p, 1, p, 2, u3(9, 0, 0), hi, box, C.byref(n))):
        assert bad() == _lib.E_INVALID


def test_clip_volume_is_the_mask(volym_lib):
    from volym_amd import scene
    rng = np.random.default_rng(3)
    dims = (13, 9, 7)
    vol = rng.integers(1, 256, size=13 * 9 * 7).astype(np.uint8)
    z, y, x = np.meshgrid(np.arange(7), np.arange(9), np.arange(13), indexing="ij")
    some = 0
    for n, d in [NONE, ((0, 0, 1), 3), ((1, 1, 1), 12), ((-1, -1, -1), -12), ((3, -2, 5), 20), ((4096, 1, 0), 4096 * 6), ((-7, 0, 2), -20), ((1, 0, 0), -1)]:
        keep = (n[0] * x + n[1] * y + n[2] * z <= d).ravel()
        want = np.where(keep, vol, 0).astype(np.uint8)
        got = scene.clip_volume(vol, dims, n, d)
        assert got.dtype == np.uint8 and got.shape == vol.shape and np.array_equal(got, want), (n, d)
        assert got is not vol and not np.shares_memory(got, vol) and vol.min() >= 1        # a copy: the input keeps its bytes
        some += 0 < int(keep.sum()) < keep.size
    assert some >= 5
    assert not scene.clip_volume(vol, dims, (1, 0, 0), -1).any()
    assert np.array_equal(scene.clip_volume(vol, dims, *NONE), vol)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_aligned_plane_is_a_crop_face(volym_lib, axis):
    """normal e_axis through 0.625 at 64^3 keeps exactly the texels below 40 on that axis -- crop_box_texels' far face there --
    and the negative normal keeps the others."""
    from volym_amd import scene
    dims = (64, 64, 64)
    vol = np.random.default_rng(11).integers(1, 256, size=64 ** 3).astype(np.uint8)
    normal, point = [0.0, 0.0, 0.0], [0.5, 0.5, 0.5]
    normal[axis], point[axis] = 1.0, 0.625
    n, d = scene.clip_plane_texels(normal, point, dims)
    want_n = [0, 0, 0]
    want_n[axis] = 4096
    assert (n, d) == (tuple(want_n), 161792)
    lo, hi = scene.crop_box_texels((0.0, 0.0, 0.0), tuple(0.625 if a == axis else 1.0 for a in range(3)), dims)
    assert hi[axis] == 40
    assert np.array_equal(scene.clip_volume(vol, dims, n, d), scene.crop_volume(vol, dims, lo, hi))
    normal[axis] = -1.0
    n, d = scene.clip_plane_texels(normal, point, dims)
    lo, hi = scene.crop_box_texels(tuple(0.625 if a == axis else 0.0 for a in range(3)), (1.0, 1.0, 1.0), dims)
    assert lo[axis] == 40
    assert np.array_equal(scene.clip_volume(vol, dims, n, d), scene.crop_volume(vol, dims, lo, hi))


def test_check_clip_plane_and_rounding(volym_lib):
    from volym_amd import scene
    assert scene.check_clip_plane((0, 0, 0), 0) == NONE
    assert scene.check_clip_plane([4096, -4096, 7], -2 ** 31) == ((4096, -4096, 7), -2 ** 31)
    assert scene.check_clip_plane(np.array([1, 2, 3], np.int32), np.int64(5)) == ((1, 2, 3), 5)
    for n, d in [((4097, 0, 0), 0), ((0, -4097, 0), 0), ((0, 0, 0), 1), ((0, 0, 0), -1), ((1, 0), 0), ((1, 0, 0, 0), 0), (1, 0), ((1, 0, 0), 2 ** 31),
                 ((1.5, 0, 0), 0), ((1, 0, 0), 0.5), ((1, 0, 0), None)]:
        with pytest.raises(ValueError):
            scene.check_clip_plane(n, d)
    # the stated value: the z face between texels 39 and 40
    assert scene.clip_plane_texels((0, 0, 1), (0.5, 0.5, 0.625), (64, 64, 64)) == ((0, 0, 4096), 161792)
    # half-texel boundaries: a plane through a texel centre keeps that texel (normal . (centre - point) == 0), one just
    # before the centre does not
    n, d = scene.clip_plane_texels((1, 0, 0), (10.5 / 64, 0.3, 0.3), (64, 32, 10))
    assert (n, d) == ((4096, 0, 0), 4096 * 10)
    n, d = scene.clip_plane_texels((1, 0, 0), (np.nextafter(10.5 / 64, 0.0), 0.3, 0.3), (64, 32, 10))
    assert n == (4096, 0, 0) and 4096 * 9 <= d < 4096 * 10
    # the length of the normal does not matter, its direction per axis length does (non-cubic dims): g = normal / dims
    assert scene.clip_plane_texels((2, 2, 0), (0.5, 0.5, 0.5), (64, 32, 10))[0] == (2048, 4096, 0)
    assert scene.clip_plane_texels((1e-9, 1e-9, 0), (0.5, 0.5, 0.5), (64, 32, 10))[0] == (2048, 4096, 0)
    n, d = scene.clip_plane_texels((1, -1, 0.5), (0.5, 0.5, 0.5), (64, 32, 10))
    assert n == (1280, -2560, 4096)                  # g = (1/64, -1/32, 1/20), k = 4096 * 20
    assert d == 1280 * 63 // 2 - 2560 * 31 // 2 + 4096 * 9 // 2 == 19072
    for a in n:
        assert abs(a) <= 4096
    # the kept side is normal . (centre - point) <= 0
    dims = (7, 5, 6)
    z, y, x = np.meshgrid(np.arange(6), np.arange(5), np.arange(7), indexing="ij")
    normal, point = (0.3, -0.8, 0.5), (0.45, 0.52, 0.4)
    n, d = scene.clip_plane_texels(normal, point, dims)
    side = sum(normal[i] * ((c + 0.5) / dims[i] - point[i]) for i, c in enumerate((x, y, z)))
    kept = n[0] * x + n[1] * y + n[2] * z <= d
    clear = np.abs(side) > 1e-3                      # (the integers round the normal: texels on the plane may go either way)
    assert np.array_equal(kept[clear], (side <= 0)[clear]) and 0 < kept.sum() < kept.size
    for normal in ((0, 0, 0), (0.0, -0.0, 0.0), (float("nan"), 1, 0), (float("inf"), 1, 0)):
        with pytest.raises(ValueError):
            scene.clip_plane_texels(normal, (0.5, 0.5, 0.5), (64, 64, 64))
    with pytest.raises(ValueError):
        scene.clip_plane_texels((1, 0), (0.5, 0.5, 0.5), (64, 64, 64))


IMP_PLANES = [((0, 1, 0), 31), ((1, 3, 0), 128), ((-1, 4, 1), 128)]


@pytest.mark.parametrize("plane", IMP_PLANES, ids=[str(p) for p in IMP_PLANES])
def test_importances_matter(oracle, volym_lib, plane):
    """Why the plane clips the importances too: with the pot important and seen from below, oracle(clipped density, clipped
    importances) differs from oracle(clipped density, FULL importances) in more than 1 % of the pixels -- an important structure
    that is cut away must stop suppressing what lies in front of it.  (80 of 6144 pixels straight, 160 cone, on each plane.)"""
    from volym_amd import scene
    W, H = 96, 64
    raw, labels = common.bonsai(64)
    dims = (64, 64, 64)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)
    table = np.zeros(256, np.uint8)
    table[4] = 255
    imp = table[lab]
    n, d = plane
    cvol, cimp = scene.clip_volume(vol, dims, n, d), scene.clip_volume(imp, dims, n, d)
    cam = oracle.benchmark_camera_uniforms(W / H, 0.0, -80.0, 0.0)
    for name, kw in (("straight", {}), ("cone", dict(use_cone_importance_check=1))):
        par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01, use_importance_rendering=1, importance_check_ahead_steps=15, **kw)
        both = oracle.render(cvol, cimp, dims, oracle.tf_default_lut(), cam, par, W, H)[1]
        density_only = oracle.render(cvol, imp, dims, oracle.tf_default_lut(), cam, par, W, H)[1]
        differing = int((both != density_only).any(axis=-1).sum())
        print("%s, %s: clipping the importances changes %d of %d pixels" % (plane, name, differing, W * H))
        assert differing > 0.01 * W * H, (plane, name, differing)


def test_library_without_a_context(volym_lib):
    """NULL context: VOLYM_E_INVALID, as every other call answers; the symbols and their multi-GPU forward are exported."""
    from volym_amd import _lib, mgpu
    L = _lib.lib()
    i3 = C.c_int32 * 3
    d = C.c_int32(0)
    assert L.volym_set_clip_plane(None, i3(0, 0, 1), 5) == _lib.E_INVALID
    assert L.volym_get_clip_plane(None, i3(), C.byref(d)) == _lib.E_INVALID
    assert mgpu.lib().volym_mgpu_set_clip_plane(None, i3(0, 0, 1), 5) == _lib.E_INVALID
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("volym_set_clip_plane", "volym_get_clip_plane", "volym_clip_plane_box", "volym_mgpu_set_clip_plane"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES or name in mgpu.SIGNATURES, name


def test_cli_clip_plane_argument():
    from volym_amd.__main__ import _clip_plane_arg
    assert _clip_plane_arg("1,0.5,1,0.5,0.5,0.5") == ((1.0, 0.5, 1.0), (0.5, 0.5, 0.5))
    assert _clip_plane_arg("0,0,-1,0,0,.625") == ((0.0, 0.0, -1.0), (0.0, 0.0, 0.625))
    for bad in ("0,0,0,0.5,0.5,0.5", "1,0,0", "1,0,0,0.5,0.5,0.5,1", "a,0,0,0.5,0.5,0.5", "", "nan,0,1,0.5,0.5,0.5", "1,0,0,inf,0.5,0.5"):
        with pytest.raises(SystemExit):
            _clip_plane_arg(bad)
