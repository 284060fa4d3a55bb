"""The slice pass on the host (no GPU): its rule, its host arithmetic and its C boundary.

scene.slice_frame is the definition the device agrees with in every byte (tests/test_gpu_slice.py).  Here it is held against the
header's rule written as a plain Python triple loop, for every mode and flag combination, and against closed forms; the C helpers
(volym_slice_check, volym_slice_axis, volym_slice_texel) are held against their Python versions.  Every comparison is over every
byte of every pixel: the rule is integer.
"""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("volym_slice_pass", "volym_read_slice", "volym_slice_device_ptr", "volym_slice_check", "volym_slice_axis", "volym_slice_texel")
# volym_slice of include/volym_hip.h: (field, offset, size)
LAYOUT = [("origin", 0, 12), ("du", 12, 12), ("dv", 24, 12), ("width", 36, 4), ("height", 40, 4), ("mode", 44, 4), ("flags", 48, 4),
          ("background", 52, 4), ("cut_rgba", 56, 4), ("palette", 60, 1024)]
DIMS = (7, 5, 3)
BACKGROUND, CUT_RGBA = (9, 80, 200, 33), (250, 30, 60, 140)
CUT = {"box": ((1, 0, 0), (6, 4, 3)), "plane": ((3, -2, 5), 9), "visible": None}      # "visible" is filled in below
E_INVALID = -1


def scene_of(seed=3):
    """density, labels, importances, lut, palette and cut state of a 7 x 5 x 3 scene"""
    from volym_amd import scene
    rng = np.random.default_rng(seed)
    n = DIMS[0] * DIMS[1] * DIMS[2]
    vol = rng.integers(1, 256, n).astype(np.uint8)              # no zero byte: a cut texel is told from a kept one by its byte
    lab = rng.integers(0, 5, n).astype(np.uint8)
    imp = rng.integers(0, 256, n).astype(np.uint8)
    lut = rng.integers(0, 256, (7, 4)).astype(np.uint8)
    pal = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    pal[1, 3], pal[2, 3] = 0, 255                               # both ends of the blend
    cut = dict(CUT, visible=scene.visibility_mask([3]))
    return vol, lab, imp, lut, pal, cut


def oblique(**kw):
    """a slice that crosses the 7 x 5 x 3 volume at an angle, with fractional steps, a negative du component, and pixels outside"""
    from volym_amd import scene
    return scene.Slice((-70000, 400000, 20000), (45000, -30011, 9000), (20000, 7001, 30500), 13, 9, background=BACKGROUND, cut_rgba=CUT_RGBA, **kw)


def blend1(src, col, a):
    return (src * (255 - a) + col * a + 127) // 255


def blend(px, col):
    return [blend1(px[0], col[0], col[3]), blend1(px[1], col[1], col[3]), blend1(px[2], col[2], col[3]), blend1(px[3], 255, col[3])]


def brute(s, vol_now, vol_uncut, lab, imp, lut, cut):
    """the rule of the header, pixel by pixel, on Python integers"""
    from volym_amd import _lib
    nx, ny, nz = DIMS
    out = np.zeros((s.height, s.width, 4), np.uint8)
    for j in range(s.height):
        for i in range(s.width):
            t = [(s.origin[a] + i * s.du[a] + j * s.dv[a]) // 65536 for a in range(3)]       # floor division
            if not all(0 <= t[a] < DIMS[a] for a in range(3)):
                out[j, i] = s.background
                continue
            at = (t[2] * ny + t[1]) * nx + t[0]
            if s.mode == _lib.SLICE_IMPORTANCE:
                m = int(imp[at])
                px = [m, m, m, 255]
            else:
                b = int((vol_uncut if s.flags & _lib.SLICE_UNCUT and vol_uncut is not None else vol_now)[at])
                px = [b, b, b, 255] if s.mode == _lib.SLICE_DENSITY else [int(v) for v in lut[(b * len(lut)) >> 8][:3]] + [255]
            if s.flags & _lib.SLICE_LABELS:
                px = blend(px, [int(v) for v in s.palette[int(lab[at])]])
            if s.flags & _lib.SLICE_MARK_CUT and cut is not None:
                lo, hi = cut["box"]
                n, d = cut["plane"]
                removed = not all(lo[a] <= t[a] < hi[a] for a in range(3))
                removed = removed or n[0] * t[0] + n[1] * t[1] + n[2] * t[2] > d
                removed = removed or cut["visible"][int(lab[at])] == 0
                if removed:
                    px = blend(px, s.cut_rgba)
            out[j, i] = px
    return out


# ---- the twin against the rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("flags", range(8))
def test_twin_equals_the_rule_pixel_by_pixel(mode, flags):
    from volym_amd import _lib, scene
    vol, lab, imp, lut, pal, cut = scene_of()
    now = scene.cut_volume(vol, DIMS, cut, lab)
    imp_now = scene.cut_volume(imp, DIMS, cut, lab)
    assert (now == 0).any() and (now != 0).any()
    if mode == _lib.SLICE_IMPORTANCE and flags & _lib.SLICE_UNCUT:         # refused: the importances' uncut source is not one buffer
        with pytest.raises(ValueError):
            scene.slice_frame(now, DIMS, oblique(mode=mode, flags=flags, palette=pal), lut, lab, imp_now, cut, vol)
        with pytest.raises(ValueError):
            scene.slice_axis("y", 2, DIMS, mode=mode, flags=flags)
        return
    slices = (oblique(mode=mode, flags=flags, palette=pal),
              scene.slice_axis("y", 2, DIMS, mode=mode, flags=flags, palette=pal, background=BACKGROUND, cut_rgba=CUT_RGBA))
    for k, s in enumerate(slices):
        got = scene.slice_frame(now, DIMS, s, lut=lut, labels=lab, importances=imp_now, cut=cut, uncut=vol)
        want = brute(s, now, vol, lab, imp_now, lut, cut)
        assert got.dtype == np.uint8 and got.shape == (s.height, s.width, 4)
        assert np.array_equal(got, want), (mode, flags, np.argwhere((got != want).any(-1))[:4])
        outside = (want == np.array(BACKGROUND, np.uint8)).all(-1)
        assert outside.any() == (k == 0) and not outside.all()               # the oblique one shows background and volume


def test_uncut_without_an_uncut_copy_shows_the_scene_as_it_stands():
    from volym_amd import _lib, scene
    vol, lab, imp, lut, pal, cut = scene_of()
    s = oblique(flags=_lib.SLICE_UNCUT)
    assert np.array_equal(scene.slice_frame(vol, DIMS, s), scene.slice_frame(vol, DIMS, s.replace(flags=0)))
    assert np.array_equal(scene.slice_frame(vol, DIMS, s), brute(s, vol, None, lab, imp, lut, None))


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_axis_slice_in_density_is_the_plane_of_the_prepared_array(axis):
    from volym_amd import scene
    vol = scene_of()[0]
    grid = vol.reshape(DIMS[2], DIMS[1], DIMS[0])               # [z, y, x]
    a = "xyz".index(axis)
    for index in range(DIMS[a]):
        got = scene.slice_frame(vol, DIMS, scene.slice_axis(axis, index, DIMS))
        plane = grid[index, :, :] if axis == "z" else grid[:, index, :] if axis == "y" else grid[:, :, index]      # rows v, columns u
        assert got.shape[:2] == plane.shape
        assert np.array_equal(got[..., 0], plane) and np.array_equal(got[..., 1], plane) and np.array_equal(got[..., 2], plane)
        assert (got[..., 3] == 255).all()


def test_labels_with_an_all_zero_alpha_palette_is_the_identity():
    from volym_amd import _lib, scene
    vol, lab, imp, lut, pal, cut = scene_of()
    pal = pal.copy()
    pal[:, 3] = 0
    for mode in (0, 1, 2):
        s = oblique(mode=mode, palette=pal)
        plain = scene.slice_frame(vol, DIMS, s, lut, lab, imp)
        assert np.array_equal(scene.slice_frame(vol, DIMS, s.replace(flags=_lib.SLICE_LABELS), lut, lab, imp), plain)


def test_mark_cut_without_a_cut_is_the_identity():
    from volym_amd import _lib, scene
    vol, lab, imp, lut, pal, cut = scene_of()
    nothing = {"box": ((0, 0, 0), DIMS), "plane": ((0, 0, 0), 0), "visible": np.ones(256, np.uint8)}
    for mode in (0, 1, 2):
        s = oblique(mode=mode, palette=pal)
        plain = scene.slice_frame(vol, DIMS, s, lut, lab, imp)
        for c in (None, nothing):
            assert np.array_equal(scene.slice_frame(vol, DIMS, s.replace(flags=_lib.SLICE_MARK_CUT), lut, lab, imp, cut=c), plain)


def test_mark_cut_marks_by_the_predicate_not_by_the_bytes():
    from volym_amd import _lib, scene
    vol, lab, imp, lut, pal, cut = scene_of()
    s = scene.slice_axis("z", 1, DIMS, flags=_lib.SLICE_MARK_CUT | _lib.SLICE_UNCUT, cut_rgba=(0, 255, 0, 255))
    got = scene.slice_frame(scene.cut_volume(vol, DIMS, cut, lab), DIMS, s, labels=lab, cut=cut, uncut=vol)
    kept = scene.cut_volume(np.ones_like(vol), DIMS, cut, lab).reshape(DIMS[2], DIMS[1], DIMS[0])[1] != 0
    assert np.array_equal((got == (0, 255, 0, 255)).all(-1), ~kept) and (~kept).any() and kept.any()
    assert np.array_equal(got[kept][:, 0], vol.reshape(DIMS[2], DIMS[1], DIMS[0])[1][kept])


def test_slice_through_shows_the_plane_it_is_given():
    from volym_amd import scene
    dims = (40, 30, 20)
    n, d = scene.clip_plane_texels((1.0, 0.5, 1.0), (0.5, 0.5, 0.5), dims)
    s = scene.slice_through((20.0, 15.0, 10.0), n, (0, 1, 0), (31, 21), 0.5)
    assert (s.width, s.height) == (31, 21)
    assert all(abs(t - c) <= 1 for t, c in zip(scene.slice_texel(s, 15, 10), (20, 15, 10)))      # the point is the centre of the output
    nn = np.array(n, np.float64) / np.sqrt(float(sum(v * v for v in n)))
    for v in (s.du, s.dv):                                     # in the plane up to the 16.16 rounding, 0.5 texel long
        assert abs(float(np.dot(nn, v))) <= 1.0 and abs(np.sqrt(float(sum(c * c for c in v))) - 32768.0) <= 2.0
    assert abs(float(np.dot(s.du, s.dv))) <= 4.0 * 32768.0
    with pytest.raises(ValueError):
        scene.slice_through((0, 0, 0), (0, 1, 0), (0, 2, 0), (8, 8))


# ---- the C helpers against their Python versions ------------------------------------------------------------------------------------
def corner_cases():
    """(slice, valid): the corners at exactly +-2^30 and one beyond, sizes, modes and flags at and beyond their ends"""
    from volym_amd import scene
    L = 1 << 30
    S = scene.Slice
    yield S((0, 0, 0), (65536, 0, 0), (0, 65536, 0), 1, 1), True
    yield S((-L, -L, -L), (0, 0, 0), (0, 0, 0), 8192, 8192), True                       # exactly -2^30: inside
    yield S((-L - 1, 0, 0), (0, 0, 0), (0, 0, 0), 4, 4), False                          # one beyond
    yield S((0, L - 1, 0), (0, 0, 0), (0, 0, 0), 4, 4), True                            # 2^30 - 1: the last one inside
    yield S((0, L, 0), (0, 0, 0), (0, 0, 0), 4, 4), False                               # exactly 2^30: outside
    yield S((0, 0, L - 1 - 3 * 7), (0, 0, 7), (0, 0, 0), 4, 2), True                    # the far corner of u lands on 2^30 - 1
    yield S((0, 0, L - 3 * 7), (0, 0, 7), (0, 0, 0), 4, 2), False                       # ... on 2^30
    yield S((0, 0, 0), (0, 0, 0), (-(L // 4), 0, 0), 2, 5), True                        # the far corner of v lands on -2^30
    yield S((-1, 0, 0), (0, 0, 0), (-(L // 4), 0, 0), 2, 5), False
    yield S((L - 1, 0, 0), (-131000, 0, 0), (0, 0, 0), 8192, 1), True                   # products beyond 32 bits stay valid when the corners are
    yield S((L - 1, 0, 0), (-(1 << 18), 0, 0), (0, 0, 0), 8192, 1), True                # (2^30 - 1) - 8191 * 2^18 = -2^30 + 2^18 - 1: the span is almost 2^31
    yield S((L - 1, 0, 0), (-(1 << 18) - 33, 0, 0), (0, 0, 0), 8192, 1), False          # ... and 33 * 8191 further down: beyond -2^30
    yield S((0, 0, 0), (1 << 17, 0, 0), (0, 0, 0), 8192, 1), True                       # 8191 * 2^17 < 2^30
    yield S((0, 0, 0), ((1 << 17) + 17, 0, 0), (0, 0, 0), 8192, 1), False               # 8191 * (2^17 + 17) >= 2^30
    yield S((2 ** 31 - 1, 0, 0), (2 ** 31 - 1, 0, 0), (2 ** 31 - 1, 0, 0), 8192, 8192), False   # far beyond 64k * 32 bits: needs 64-bit sums
    for w, h, ok in ((0, 1, False), (1, 0, False), (8192, 8192, True), (8193, 1, False), (1, 8193, False), (2 ** 32 - 1, 1, False)):
        yield S((0, 0, 0), (0, 0, 0), (0, 0, 0), w, h), ok
    for mode, flags, ok in ((0, 7, True), (1, 7, True), (2, 6, True), (2, 1, False), (2, 7, False), (3, 0, False), (0, 8, False), (0, 1 << 31, False),
                            (2 ** 32 - 1, 0, False)):
        yield S((0, 0, 0), (0, 0, 0), (0, 0, 0), 3, 3, mode=mode, flags=flags), ok


def test_check_agrees_with_python_on_every_corner_case(volym_lib):
    from volym_amd import scene
    n = 0
    for s, ok in corner_cases():
        rc = volym_lib.volym_slice_check(C.byref(s.to_c()))
        assert rc == (0 if ok else E_INVALID), (vars(s), ok, rc)
        if ok:
            assert scene.check_slice(s) is s
        else:
            with pytest.raises(ValueError):
                scene.check_slice(s)
        n += 1
    assert n > 25
    assert volym_lib.volym_slice_check(None) == E_INVALID


def test_axis_agrees_with_python(volym_lib):
    from volym_amd import _lib, scene
    for dims in ((7, 5, 3), (1, 1, 1), (8192, 4096, 2), (37, 22, 19)):
        d3 = (C.c_uint32 * 3)(*dims)
        for axis, name in enumerate("xyz"):
            for index in sorted({0, dims[axis] // 2, dims[axis] - 1}):
                c = _lib.Slice()
                c.mode, c.flags = 1, 6
                c.background, c.cut_rgba = (C.c_uint8 * 4)(1, 2, 3, 4), (C.c_uint8 * 4)(5, 6, 7, 8)
                c.palette[200][2] = 99
                assert volym_lib.volym_slice_axis(axis, index, d3, C.byref(c)) == 0
                got, want = scene.Slice.from_c(c), scene.slice_axis(name, index, dims)
                assert (got.origin, got.du, got.dv, got.width, got.height) == (want.origin, want.du, want.dv, want.width, want.height)
                # mode, flags and colours are left alone
                assert (got.mode, got.flags, got.background, got.cut_rgba, int(got.palette[200, 2])) == (1, 6, (1, 2, 3, 4), (5, 6, 7, 8), 99)
                assert volym_lib.volym_slice_check(C.byref(c)) == 0
                # through texel centres, one texel per pixel
                u, v = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
                t = [0, 0, 0]
                t[axis], t[u], t[v] = index, want.width - 1, want.height - 1
                assert scene.slice_texel(want, want.width - 1, want.height - 1) == tuple(t)
            c = _lib.Slice()
            assert volym_lib.volym_slice_axis(axis, dims[axis], d3, C.byref(c)) == E_INVALID
            with pytest.raises(ValueError):
                scene.slice_axis(name, dims[axis], dims)
    d3 = (C.c_uint32 * 3)(4, 4, 4)
    c = _lib.Slice()
    assert volym_lib.volym_slice_axis(3, 0, d3, C.byref(c)) == E_INVALID
    assert volym_lib.volym_slice_axis(-1, 0, d3, C.byref(c)) == E_INVALID
    assert volym_lib.volym_slice_axis(0, 0, None, C.byref(c)) == E_INVALID
    assert volym_lib.volym_slice_axis(0, 0, d3, None) == E_INVALID
    with pytest.raises(ValueError):
        scene.slice_axis("w", 0, (4, 4, 4))


def test_texel_agrees_with_python_and_floors(volym_lib):
    from volym_amd import scene
    L = 1 << 30
    cases = [oblique(),
             scene.Slice((-1, -65536, -65537), (0, 0, 0), (0, 0, 0), 1, 1),               # floor: -1, -1, -2; truncation would give 0, -1, -1
             scene.Slice((-L, L - 1, 0), (1 << 17, -(1 << 17), 0), (0, 0, 0), 8192, 1),
             scene.Slice((32768, 32768, 32768), (-16384, 16385, 0), (0, -16384, 229376), 70, 9)]
    assert scene.slice_texel(cases[1], 0, 0) == (-1, -1, -2)
    for s in cases:
        c = s.to_c()
        for i, j in itertools.product(sorted({0, 1, s.width // 2, s.width - 1}), sorted({0, s.height // 2, s.height - 1})):
            if i >= s.width:
                continue
            t = (C.c_int32 * 3)()
            assert volym_lib.volym_slice_texel(C.byref(c), i, j, t) == 0
            want = tuple((s.origin[a] + i * s.du[a] + j * s.dv[a]) // 65536 for a in range(3))
            assert tuple(t) == want == scene.slice_texel(s, i, j), (i, j)
        t = (C.c_int32 * 3)()
        assert volym_lib.volym_slice_texel(C.byref(c), s.width, 0, t) == E_INVALID
        assert volym_lib.volym_slice_texel(C.byref(c), 0, s.height, t) == E_INVALID
        assert volym_lib.volym_slice_texel(None, 0, 0, t) == E_INVALID
        assert volym_lib.volym_slice_texel(C.byref(c), 0, 0, None) == E_INVALID
        with pytest.raises(ValueError):
            scene.slice_texel(s, s.width, 0)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_library_exports_the_six_calls(volym_lib):
    from volym_amd import _lib
    for name in CALLS:
        assert hasattr(volym_lib, name), name
        assert name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2                  # the calls are additions: the ABI version stays


def test_every_declared_symbol_is_exported(volym_lib):
    from volym_amd import _lib
    for header in ("volym_hip.h", "volym_host.h"):
        code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        names = re.findall(r"\b(volym_\w+)\s*\(", code)
        assert names
        for name in names:
            assert hasattr(volym_lib, name), name
            assert name in _lib.SIGNATURES, name


def test_header_declares_them_the_struct_and_the_enums():
    text = open(os.path.join(ROOT, "include", "volym_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "} volym_slice;" in code
    assert re.search(r"VOLYM_SLICE_DENSITY = 0, VOLYM_SLICE_TF = 1, VOLYM_SLICE_IMPORTANCE = 2", code)
    assert re.search(r"VOLYM_SLICE_UNCUT = 1, VOLYM_SLICE_LABELS = 2, VOLYM_SLICE_MARK_CUT = 4", code)
    assert re.search(r"#define VOLYM_ABI_VERSION 2\b", code)
    assert "multi-GPU loop has no forward" in text[text.index("int   volym_slice_pass") - 3000:text.index("int   volym_slice_pass")]


def test_struct_is_1084_bytes_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Slice) == 1084
    for f, off, size in LAYOUT:
        d = getattr(_lib.Slice, f)
        assert (d.offset, d.size) == (off, size), f
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n  printf("%zu", sizeof(volym_slice));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_slice, %s));\n' % f for f, _, _ in LAYOUT) +
                   '  printf(" %d %d %d %d %d %d", VOLYM_SLICE_DENSITY, VOLYM_SLICE_TF, VOLYM_SLICE_IMPORTANCE, VOLYM_SLICE_UNCUT, VOLYM_SLICE_LABELS, VOLYM_SLICE_MARK_CUT);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [1084] + [off for _, off, _ in LAYOUT] + [0, 1, 2, 1, 2, 4], out
    assert (_lib.SLICE_DENSITY, _lib.SLICE_TF, _lib.SLICE_IMPORTANCE, _lib.SLICE_UNCUT, _lib.SLICE_LABELS, _lib.SLICE_MARK_CUT) == (0, 1, 2, 1, 2, 4)


def test_python_faces_exist():
    from volym_amd import demo, scene
    for name in ("slice_pass", "read_slice", "slice_device_ptr"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("slice", "slices_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("check_slice", "slice_axis", "slice_texel", "slice_through", "slice_frame"):
        assert callable(getattr(scene, name))
