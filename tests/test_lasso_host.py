"""The lasso without a GPU: the C structs and constants, volym_lasso_check and volym_lasso_rect against their twins in scene, the
polygon's mask against a crossing count in exact fractions, the host twin scene.lasso_volume against a plain triple loop over Python
integers, the library's integer view against the float64 projection and against the picks of the march, and the conditions
tests/test_gpu_lasso.py relies on, asserted on the twin.
"""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import lasso_scenes as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

REQUEST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("to", 36, 256), ("n_points", 292, 4), ("view", 296, 88),
                  ("points", 384, 8192)]
VIEW_LAYOUT = [("m", 0, 36), ("width", 36, 4), ("height", 40, 4), ("scale_log2", 44, 4), ("c", 48, 24), ("depth", 72, 16)]
POINT_LAYOUT = [("x", 0, 4), ("y", 4, 4)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Lasso) == 8576 and C.sizeof(_lib.LassoView) == 88 and C.sizeof(_lib.LassoPoint) == 8
    for struct, layout in ((_lib.Lasso, REQUEST_LAYOUT), (_lib.LassoView, VIEW_LAYOUT), (_lib.LassoPoint, POINT_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
    consts = [_lib.LASSO_UNCUT, _lib.LASSO_DRY_RUN, _lib.LASSO_OUTSIDE, _lib.LASSO_MAX_POINTS, _lib.LASSO_MAX_FRAME, _lib.LASSO_VERTEX_MAX]
    assert consts == [1, 16, 32, 1024, 16384, 1 << 20] and (_lib.LASSO_UNCUT, _lib.LASSO_DRY_RUN) == (_lib.RELABEL_UNCUT, _lib.RELABEL_DRY_RUN)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu", sizeof(volym_lasso), sizeof(struct volym_lasso_view), sizeof(struct volym_lasso_point), sizeof(struct volym_relabel_result));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_lasso, %s));\n' % f for f, _, _ in REQUEST_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_lasso_view, %s));\n' % f for f, _, _ in VIEW_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_lasso_point, %s));\n' % f for f, _, _ in POINT_LAYOUT) +
                   '  printf(" %d %d %d %u %u %d", VOLYM_LASSO_UNCUT, VOLYM_LASSO_DRY_RUN, VOLYM_LASSO_OUTSIDE, VOLYM_LASSO_MAX_POINTS, VOLYM_LASSO_MAX_FRAME, VOLYM_LASSO_VERTEX_MAX);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    p = subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [8576, 88, 8, 4128] + [o for _, o, _ in REQUEST_LAYOUT] + [o for _, o, _ in VIEW_LAYOUT] + [o for _, o, _ in POINT_LAYOUT] + consts
    assert got == want


def _good(oracle):
    from volym_amd import scene
    return scene.Lasso(LS.STAR, LS.view(oracle, "pose", LS.DIMS), to=LS.every(7), dims=LS.DIMS)


def _bad_requests(good):
    """(what, request) that both checks must refuse"""
    v = good.view
    out = []
    for a in range(3):
        hi = list(LS.DIMS); hi[a] += 1
        out.append(("box past the volume", good.replace(box=((0, 0, 0), tuple(hi)))))
        lo = [0, 0, 0]; lo[a] = 5; hi = list(LS.DIMS); hi[a] = 4
        out.append(("box lo > hi", good.replace(box=(tuple(lo), tuple(hi)))))
    for flags in (2, 4, 8, 64, 1 << 31):
        out.append(("flags %d" % flags, good.replace(flags=flags)))
    for window in ((9, 8), (0, 256)):
        out.append(("window %r" % (window,), good.replace(window=window)))
    out.append(("two vertices", good.replace(points=LS.STAR[:2])))
    out.append(("1025 vertices", good.replace(points=[(i % 90, i // 90) for i in range(1025)])))
    for p in ((2 ** 20 + 1, 0), (0, -2 ** 20 - 1)):
        out.append(("vertex %r" % (p,), good.replace(points=LS.STAR[:3] + [p])))
    m = [list(r) for r in v.m]; m[1][2] = -2 ** 31
    out.append(("m = -2^31", good.replace(view=v.replace(m=m))))
    for c in (2 ** 46, -2 ** 46):
        out.append(("c = %d" % c, good.replace(view=v.replace(c=(v.c[0], c, v.c[2])))))
    out.append(("depth[0] = 0", good.replace(view=v.replace(depth=(0, 5)))))
    out.append(("depth[0] > depth[1]", good.replace(view=v.replace(depth=(6, 5)))))
    for w, h in ((0, 64), (96, 0), (16385, 64), (96, 16385)):
        out.append(("frame %d x %d" % (w, h), good.replace(view=v.replace(width=w, height=h))))
    return out


def test_check_lasso_and_volym_lasso_check_refuse_the_same_requests(oracle, volym_lib):
    from volym_amd import _lib, scene
    good = _good(oracle)
    dims = (C.c_uint32 * 3)(*LS.DIMS)
    rect = (C.c_uint32 * 4)()
    for case in LS.cases(oracle):
        assert scene.check_lasso(case.lasso, LS.DIMS) is case.lasso
        assert volym_lib.volym_lasso_check(C.byref(case.lasso.to_c()), dims) == _lib.OK, case.name
        assert volym_lib.volym_lasso_rect(C.byref(case.lasso.to_c()), rect) == _lib.OK and tuple(rect) == scene.lasso_rect(case.lasso), case.name
    # the edges of what is valid
    v = good.view
    for ok in (good.replace(points=LS.STAR[:3] + [(2 ** 20, -2 ** 20)]), good.replace(view=v.replace(c=(2 ** 46 - 1, 1 - 2 ** 46, 0))),
               good.replace(view=v.replace(m=[[2 ** 31 - 1, 1 - 2 ** 31, 0]] * 3)), good.replace(view=v.replace(depth=(1, 1))),
               good.replace(view=v.replace(width=16384, height=1)), good.replace(flags=1 | 16 | 32), good.replace(box=((3, 3, 3), (3, 9, 9)))):
        scene.check_lasso(ok, LS.DIMS)
        assert volym_lib.volym_lasso_check(C.byref(ok.to_c()), dims) == _lib.OK
    for what, bad in _bad_requests(good):
        with pytest.raises(ValueError):
            scene.check_lasso(bad, LS.DIMS)
        c = bad.to_c() if len(bad.points) <= 1024 else None
        if c is None:
            c = good.to_c()
            c.n_points = 1025
        assert volym_lib.volym_lasso_check(C.byref(c), dims) == E_INVALID, what
    assert volym_lib.volym_lasso_check(None, dims) == E_INVALID and volym_lib.volym_lasso_check(C.byref(good.to_c()), None) == E_INVALID
    assert volym_lib.volym_lasso_rect(None, rect) == E_INVALID and volym_lib.volym_lasso_rect(C.byref(good.to_c()), None) == E_INVALID
    c = good.to_c()
    c.n_points = 2
    assert volym_lib.volym_lasso_rect(C.byref(c), rect) == E_INVALID
    assert scene.lasso_rect(good.replace(points=LS.POLYGONS["off screen"])) == (0, 0, 0, 0)
    assert scene.lasso_rect(good.replace(points=LS.POLYGONS["a word and a pixel"])) == (31, 12, 64, 52)
    assert scene.lasso_rect(good.replace(points=LS.POLYGONS["frame"])) == (0, 0, LS.W, LS.H)


def test_the_view_helpers_refuse_what_they_cannot_quantise(oracle, volym_lib):
    from volym_amd import _lib, scene
    u = LS.camera_uniforms(oracle, "pose")
    out = _lib.LassoView()
    dims = (C.c_uint32 * 3)(*LS.DIMS)
    f = volym_lib.volym_lasso_view_from_camera
    assert f(C.byref(u), 96, 64, dims, 0.0, C.byref(out)) == _lib.OK and out.depth[0] == 1 and out.depth[1] == 2 ** 63 - 1 and (out.width, out.height) == (96, 64)
    assert f(None, 96, 64, dims, 0.0, C.byref(out)) == E_INVALID and f(C.byref(u), 96, 64, None, 0.0, C.byref(out)) == E_INVALID
    assert f(C.byref(u), 96, 64, dims, 0.0, None) == E_INVALID
    for w, h in ((0, 64), (96, 0), (16385, 64), (96, 16385)):
        assert f(C.byref(u), w, h, dims, 0.0, C.byref(out)) == E_INVALID
    assert f(C.byref(u), 96, 64, (C.c_uint32 * 3)(37, 0, 19), 0.0, C.byref(out)) == E_INVALID
    assert f(C.byref(u), 96, 64, (C.c_uint32 * 3)(37, 4097, 19), 0.0, C.byref(out)) == E_INVALID
    bad = _lib.CameraUniforms.from_buffer_copy(bytes(u))
    bad.view_matrix[1][2] = float("nan")
    assert f(C.byref(bad), 96, 64, dims, 0.0, C.byref(out)) == E_INVALID
    v = scene.lasso_view(u, 96, 64, LS.DIMS, near=0.25)
    assert v.depth == (round(0.25 * 2 ** v.scale_log2), 2 ** 63 - 1)
    w = scene.lasso_view_depth(v, 0.5, 1.5)
    assert w.depth == (2 ** (v.scale_log2 - 1), 3 * 2 ** (v.scale_log2 - 1)) and (w.m, w.c) == (v.m, v.c)
    assert scene.lasso_view_depth(v, -3.0).depth == (1, 2 ** 63 - 1)
    for front, back in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("nan")), (-2.0, -1.0)):
        with pytest.raises(ValueError):
            scene.lasso_view_depth(v, front, back)
    assert volym_lib.volym_lasso_view_depth(None, 0.0, 1.0) == E_INVALID


# ---- the polygon's mask ---------------------------------------------------------------------------------------------------------
_exact = {}


def exact_mask(points, width=LS.W, height=LS.H):
    """the even-odd mask by a crossing count in exact fractions: an edge counts for pixel (px, py) iff it spans the row, half-open
    ((y0 <= py) != (y1 <= py)), and its x at that row, x0 + (py - y0) (x1 - x0) / (y1 - y0), lies strictly right of px"""
    key = (tuple(points), width, height)
    if key not in _exact:
        mask = np.zeros((height, width), bool)
        n = len(points)
        for py in range(height):
            at = []
            for i in range(n):
                (x0, y0), (x1, y1) = points[i], points[(i + 1) % n]
                if (y0 <= py) != (y1 <= py):
                    at.append(x0 + Fraction((py - y0) * (x1 - x0), y1 - y0))
            for px in range(width):
                mask[py, px] = sum(1 for x in at if px < x) % 2 == 1
        _exact[key] = mask
    return _exact[key]


@pytest.mark.parametrize("name", list(LS.POLYGONS))
def test_the_mask_is_the_crossing_count_in_exact_fractions(name):
    from volym_amd import scene
    points = LS.POLYGONS[name] or LS.walk()
    got = scene.lasso_mask(points, LS.W, LS.H)
    assert got.shape == (LS.H, LS.W) and got.dtype == bool
    assert np.array_equal(got, exact_mask(points)), name
    rect, words = scene.lasso_mask_words(points, LS.W, LS.H)
    x0, y0, x1, y1 = rect
    assert not got[:y0].any() and not got[y1:].any() and not got[:, :x0].any() and not got[:, x1:].any()        # nothing outside the rect
    stride = (x1 - x0 + 31) // 32
    assert words.size == stride * (y1 - y0) and words.dtype == np.uint32
    for py in range(y0, y1):
        for px in range(x0, x1):
            assert bool((int(words[(py - y0) * stride + (px - x0) // 32]) >> ((px - x0) & 31)) & 1) == bool(got[py, px])
    if name in ("sliver", "off screen"):
        assert not got.any()
    else:
        assert got.sum() > 50


def test_the_four_properties_of_the_rule():
    from volym_amd import scene
    M = lambda p: scene.lasso_mask(p, LS.W, LS.H)
    # two polygons that share an edge never both claim a pixel and never both miss one: a fan of triangles about an inner point
    # tiles the star, an oblique cut tiles the rectangle
    hub = (47, 33)
    fan = [M([hub, LS.STAR[i], LS.STAR[(i + 1) % len(LS.STAR)]]) for i in range(len(LS.STAR))]
    assert np.array_equal(np.sum(fan, axis=0), M(LS.STAR).astype(np.int64))
    a, b = M([(30, 10), (60, 10), (37, 50), (30, 50)]), M([(60, 10), (60, 50), (37, 50)])
    assert not (a & b).any() and np.array_equal(a | b, M(LS.RECT))
    # an axis-aligned rectangle covers exactly x0 <= px < x1, y0 <= py < y1
    want = np.zeros((LS.H, LS.W), bool)
    want[10:50, 30:60] = True
    assert np.array_equal(M(LS.RECT), want)
    want[:] = False
    want[0:7, 90:96] = True
    assert np.array_equal(M([(90, -3), (200, -3), (200, 7), (90, 7)]), want)
    # the vertex order does not matter
    for name, p in LS.POLYGONS.items():
        p = p or LS.walk()
        assert np.array_equal(M(p), M(p[::-1])), name
        assert np.array_equal(M(p), M(p[3:] + p[:3])), name
    # a bow-tie is two triangles; a polygon that overlaps itself twice is empty there
    bow = M(LS.POLYGONS["bow-tie"])
    assert bow[32, 20] and bow[32, 76] and not bow[12, 48] and not bow[52, 48]
    twice = M([(10, 10), (50, 10), (50, 50), (10, 50), (10, 10), (50, 10), (50, 50), (10, 50)])
    assert not twice.any()
    over = M([(10, 10), (50, 10), (50, 50), (10, 50), (10, 10), (30, 10), (30, 50), (10, 50)])
    want[:] = False
    want[10:50, 30:50] = True
    assert np.array_equal(over, want)


def test_below_is_exact_where_the_product_does_not_fit_64_bits():
    from volym_amd import scene
    rng = np.random.default_rng(3)
    X = rng.integers(-2 ** 52, 2 ** 52, 4000)
    D = rng.integers(-2 ** 52, 2 ** 52, 4000)
    X[:1000] = D[:1000] * rng.integers(0, 3, 1000) + rng.integers(-1, 2, 1000)
    for r in (0, 1, 2, 31, 96, 4097, 16383, 16384):
        X[1000:2000] = np.clip(D[1000:2000], -2 ** 37, 2 ** 37) * r + rng.integers(-1, 2, 1000)
        got = scene._lasso_below(X, r, D)
        assert got.tolist() == [int(x) < r * int(d) for x, d in zip(X, D)]


# ---- the twin against a triple loop ---------------------------------------------------------------------------------------------
def loop_volume(prepared, dims, l, labels, uncut):
    """the rule of include/volym_hip.h, texel by texel on Python integers; the mask is the exact one"""
    nx, ny, nz = dims
    v = l.view
    mask = exact_mask(l.points, v.width, v.height)
    outside = bool(l.flags & 32)
    src = uncut if l.flags & 1 else prepared
    new = [int(b) for b in labels]
    changed, left, arrived, box = 0, [0] * 256, [0] * 256, None
    (x0, y0, z0), (x1, y1, z1) = l.box
    to = [int(t) for t in l.to]
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                h = (2 * x + 1, 2 * y + 1, 2 * z + 1)
                X, Y, D = (sum(v.m[r][a] * h[a] for a in range(3)) + v.c[r] for r in range(3))
                inside = v.depth[0] <= D <= v.depth[1] and 0 <= X < v.width * D and 0 <= Y < v.height * D and bool(mask[Y // D, X // D])
                i = x + nx * (y + ny * z)
                old = int(labels[i])
                if inside == outside or to[old] == old or not l.window[0] <= int(src[i]) <= l.window[1]:
                    continue
                changed += 1
                left[old] += 1
                arrived[to[old]] += 1
                box = (x, y, z, x + 1, y + 1, z + 1) if box is None else tuple(min(p, q) for p, q in zip(box[:3], (x, y, z))) + tuple(max(p, q + 1) for p, q in zip(box[3:], (x, y, z)))
                if not l.flags & 16:
                    new[i] = to[old]
    return np.array(new, np.uint8), changed, left, arrived, box or (0,) * 6


def _same(got, want, what):
    new, res = got
    assert np.array_equal(new.ravel(), want[0]), what
    assert int(res["changed"]) == want[1] and res["left"].tolist() == want[2] and res["arrived"].tolist() == want[3] and tuple(int(b) for b in res["box"]) == tuple(want[4]), what


def test_the_twin_equals_a_triple_loop_on_a_small_volume(oracle):
    from volym_amd import scene
    dims = (7, 5, 3)
    rng = np.random.default_rng(8)
    vol = rng.integers(0, 256, 7 * 5 * 3).astype(np.uint8)
    cut = np.where(rng.random(vol.size) < 0.3, 0, vol).astype(np.uint8)
    labels = rng.integers(0, 4, vol.size).astype(np.uint8)
    to = np.arange(256); to[0], to[1], to[2] = 1, 2, 0
    n = 0
    for which in ["pose"] + list(LS.CAMERAS):
        v = LS.view(oracle, which, dims)
        ortho = v.replace(m=(v.m[0], v.m[1], (0, 0, 0)), c=(v.c[0], v.c[1], 2 ** 30))      # an orthographic view: D does not depend on the texel
        for view in (v, ortho, scene.lasso_view_depth(v, 0.9, 1.4)):
            for poly in (LS.STAR, LS.POLYGONS["bow-tie"], LS.POLYGONS["frame"]):
                for flags in (0, 32, 1, 16 | 32):
                    for box, window in ((None, (0, 255)), (((1, 0, 1), (6, 4, 3)), (60, 200))):
                        l = scene.Lasso(poly, view, box, flags, window, to, dims=dims)
                        got = scene.lasso_volume(cut, dims, l, labels, uncut=vol)
                        _same(got, loop_volume(cut, dims, l, labels, vol), (which, flags, box))
                        n += int(got[1]["changed"])
    assert n > 2000


def test_the_twin_equals_a_triple_loop_on_scene_a_and_gives_each_case_its_count(oracle):
    from volym_amd import scene
    host = LS.SCENES["a"]()
    cut = np.where(np.random.default_rng(9).random(host.vol.size) < 0.3, 0, host.vol.ravel()).astype(np.uint8)       # (what UNCUT must not read)
    total = 0
    for case in LS.cases(oracle):
        got = scene.lasso_volume(cut, host.dims, case.lasso, host.labels, uncut=host.vol)
        _same(got, loop_volume(cut, host.dims, case.lasso, host.labels, host.vol), case.name)
        plain = LS.expect(host, case)[1]
        assert int(plain["changed"]) == case.count, (case.name, int(plain["changed"]))
        assert case.trivial == (case.count == 0), case.name
        assert case.trivial or case.count > 50, case.name
        if not case.lasso.flags & 16:
            total += case.count
    assert total >= 1000
    # the depth the cases cut the volume at is its middle along the view axis
    lands, _, _ = scene.lasso_texels(scene.lasso_view_depth(LS.view(oracle, "pose", LS.DIMS), 0.0, LS.DEPTH_MID), LS.DIMS)
    assert 0.4 < lands.mean() < 0.6


def test_the_ragged_scene_changes_texels_in_every_case_that_is_not_trivial(oracle):
    host = LS.SCENES["ragged"]()
    for case in LS.cases(oracle, host.dims):
        changed = int(LS.expect(host, case)[1]["changed"])
        assert case.trivial == (changed == 0), (case.name, changed)


# ---- the view -------------------------------------------------------------------------------------------------------------------
def float_projection(u, W, H, dims, x, y, z):
    """screen position (sx, sy) and clip w of the centres of texels (x, y, z) in float64, from the uniforms' f32 matrices"""
    P = np.array([[u.projection_matrix[c][r] for c in range(4)] for r in range(4)], np.float64)
    V = np.array([[u.view_matrix[c][r] for c in range(4)] for r in range(4)], np.float64)
    p = np.stack([(np.asarray(x) + 0.5) / dims[0], (np.asarray(y) + 0.5) / dims[1], (np.asarray(z) + 0.5) / dims[2], np.ones(np.shape(x))], 0)
    clip = (P @ V) @ p
    return (clip[0] / clip[3] + 1.0) * 0.5 * W, (1.0 - clip[1] / clip[3]) * 0.5 * H, clip[3]


@pytest.mark.parametrize("which", ["pose"] + list(LS.CAMERAS))
def test_the_integer_view_is_within_a_64th_of_a_pixel_of_the_float64_projection(oracle, which):
    """Each rounded row entry is off by at most 1/2 where the largest entry of the three rows is at least 2^30 (|m|) or 2^45 (|c|):
    relative 2^-30 of the rows' scale, which a frame of W pixels and h < 2^13 turn into far less than 1/64 pixel for D >= depth[0]
    at the distances of these views.  px is floor(sx + 1/2): the nearest ray's pixel."""
    from volym_amd import _lib, scene
    for dims, (W, H), n in ((LS.DIMS, (LS.W, LS.H), None), ((1024, 1024, 1024), (3840, 2160), 200000)):
        u = LS.camera_uniforms(oracle, which)
        v = scene.lasso_view(u, W, H, dims)
        assert 20 <= v.scale_log2 <= 40
        if n is None:
            z, y, x = (a.ravel() for a in np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij"))
        else:
            rng = np.random.default_rng(4)
            x, y, z = (rng.integers(0, d, n) for d in dims)
        X, Y, D = (v.m[r][0] * (2 * x + 1) + v.m[r][1] * (2 * y + 1) + v.m[r][2] * (2 * z + 1) + v.c[r] for r in range(3))
        assert max(int(np.abs(a).max()) for a in (X, Y, D)) < 2 ** 45           # (the rule holds them below 2^51)
        sx, sy, w = float_projection(u, W, H, dims, x, y, z)
        front = w * 2.0 ** v.scale_log2 >= 2 ** (v.scale_log2 - 6)               # (clip w >= 1/64: what the bound is derived for)
        on = front & (sx > -0.5) & (sx < W - 0.5) & (sy > -0.5) & (sy < H - 0.5)
        assert on.sum() > 1000
        ex, ey = X[on] / D[on] - 0.5 - sx[on], Y[on] / D[on] - 0.5 - sy[on]
        assert max(np.abs(ex).max(), np.abs(ey).max()) <= 1.0 / 64, (which, dims, float(np.abs(ex).max()), float(np.abs(ey).max()))
        lands, px, py = (a.ravel() for a in scene.lasso_texels(v, dims)) if n is None else (None, None, None)
        if n is None:
            clear = on & (np.abs(sx + 0.5 - np.round(sx + 0.5)) > 1.0 / 64) & (np.abs(sy + 0.5 - np.round(sy + 0.5)) > 1.0 / 64)
            assert lands[clear].all()
            assert np.array_equal(px[clear], np.floor(sx[clear] + 0.5).astype(np.int64)) and np.array_equal(py[clear], np.floor(sy[clear] + 0.5).astype(np.int64))


def test_a_picked_texel_lands_on_the_pixel_that_picked_it(oracle, volym_lib):
    """The march's ray of pixel gx passes through the pixel's corner gx / W and the picked sample lies inside the picked texel: the
    texel's centre projects within a texel's projected half-diagonal of (gx, gy), and floor(sx + 1/2) within one more pixel.  A y
    flip or a centre convention in place of the corner's fails this."""
    from tests import pick_reference as R
    from tests.test_gpu_crop_box import CANOPY, PARAMS, _bonsai, _uniforms
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = oracle.tf_default_lut()
    seen = 0
    for pose in ((35.0, 20.0, 0.0), (200.0, -25.0, 0.0)):
        cam, par, cu, _ = _uniforms(oracle, LS.W, LS.H, pose, **PARAMS["no opacity"])
        rows = np.arange(2, LS.H, 3)
        got = R.frame(vol, CANOPY[labels], dims, lut, cam, par, LS.W, LS.H, 0.3, labels=labels, rows=rows)
        p = got["picks"]
        hit = p["status"] == 2
        gy, gx = np.meshgrid(rows, np.arange(LS.W), indexing="ij")
        x, y, z = (p[k][hit].astype(np.int64) for k in ("x", "y", "z"))
        view = scene.lasso_view(cu, LS.W, LS.H, dims)
        lands, px, py = scene.lasso_texels(view, dims)
        assert lands[z, y, x].all()
        # the projected half-diagonal of each picked texel, in pixels, in float64
        sx, sy, _ = float_projection(cu, LS.W, LS.H, dims, x, y, z)
        half = np.zeros(x.size)
        for dx in (-0.5, 0.5):
            for dy in (-0.5, 0.5):
                for dz in (-0.5, 0.5):
                    cx, cy, _ = float_projection(cu, LS.W, LS.H, dims, x + dx, y + dy, z + dz)
                    half = np.maximum(half, np.hypot(cx - sx, cy - sy))
        assert half.max() < 2.0
        ex, ey = px[z, y, x] - gx[hit], py[z, y, x] - gy[hit]
        assert (np.hypot(ex, ey) <= half + 1.0).all(), (pose, float(np.hypot(ex, ey).max()))
        assert (np.hypot(sx - gx[hit], sy - gy[hit]) <= half + 1e-3).all()
        assert abs(ex.mean()) < 0.25 and abs(ey.mean()) < 0.25              # no half-pixel bias either way
        seen += int(hit.sum())
    assert seen > 250


def test_the_small_scene_shares_rows_within_chunks(volym_lib):
    """what tests/test_gpu_lasso.py's small-shape test relies on: the triangle and its OUTSIDE twin each change a texel but not all,
    between them every texel, and a changed texel lies in a row above the first of a chunk that starts in row 0"""
    host = LS.scene_small()
    nx, ny, nz = host.dims
    assert host.dims == (5, 3, 9) and nx * ny < 16
    inside, outside = LS.small_cases()
    assert outside.lasso.flags == 32 and inside.lasso.flags == 0 and inside.lasso.view.width == inside.lasso.view.height == 64
    total = 0
    for case in (inside, outside):
        new, res = LS.expect(host, case)
        assert 1 <= int(res["changed"]) < nx * ny * nz, case.name
        assert LS.rows_shared(host.dims, host.labels, new) >= 1, case.name
        total += int(res["changed"])
    assert total == nx * ny * nz
