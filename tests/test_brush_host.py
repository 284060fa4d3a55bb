"""The brush without a GPU: the C structs and constants, volym_brush_check and volym_brush_box against their twins in scene, the
integer rule against closest-point distances in exact fractions, the host twin scene.brush_volume against a plain triple loop over
Python integers, the closed forms, and the conditions tests/test_gpu_brush.py relies on, asserted on the twin.
"""
import ctypes as C
import itertools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import brush_scenes as BS
from tests import relabel_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

REQUEST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("to", 36, 256), ("weight", 292, 12), ("r2", 304, 4),
                  ("n_points", 308, 4), ("points", 312, 2048)]
POINT_LAYOUT = [("x", 0, 2), ("y", 2, 2), ("z", 4, 2), ("flags", 6, 2)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Brush) == 2360 and C.sizeof(_lib.BrushPoint) == 8
    for struct, layout in ((_lib.Brush, REQUEST_LAYOUT), (_lib.BrushPoint, POINT_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
    consts = [_lib.BRUSH_UNCUT, _lib.BRUSH_DRY_RUN, _lib.BRUSH_LIFT, _lib.BRUSH_MAX_POINTS, _lib.DISTANCE_WEIGHT_MAX]
    assert consts == [1, 16, 1, 256, 64] and (_lib.BRUSH_UNCUT, _lib.BRUSH_DRY_RUN) == (_lib.RELABEL_UNCUT, _lib.RELABEL_DRY_RUN)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(volym_brush), sizeof(struct volym_brush_point), sizeof(struct volym_relabel_result));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_brush, %s));\n' % f for f, _, _ in REQUEST_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_brush_point, %s));\n' % f for f, _, _ in POINT_LAYOUT) +
                   '  printf(" %d %d %d %u %u", VOLYM_BRUSH_UNCUT, VOLYM_BRUSH_DRY_RUN, VOLYM_BRUSH_LIFT, VOLYM_BRUSH_MAX_POINTS, VOLYM_DISTANCE_WEIGHT_MAX);\n'
                   '  printf(" %d %d", VOLYM_BRUSH_UNCUT == VOLYM_RELABEL_UNCUT, VOLYM_BRUSH_DRY_RUN == VOLYM_RELABEL_DRY_RUN);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [2360, 8, 4128] + [o for _, o, _ in REQUEST_LAYOUT] + [o for _, o, _ in POINT_LAYOUT] + consts + [1, 1], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_brush_labels", "volym_brush_check", "volym_brush_box"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert callable(demo.GpuContext.brush_labels)
    for name in ("brush_at", "stroke"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Brush", "check_brush", "brush_box", "brush_volume"):
        assert callable(getattr(scene, name))
    assert "each call is an undo step" in " ".join(demo.Simple.stroke.__doc__.lower().split())
    header = " ".join(open(os.path.join(ROOT, "include", "volym_hip.h")).read().split())
    section = header[header.index("--- brush:"):header.index("int volym_brush_labels(")]
    assert "exact in unsigned 64-bit arithmetic" in section and "has no forward for this call" in section


def _check_rows():
    """(name, request, dims, valid)"""
    from volym_amd import scene
    d = (9, 7, 5)
    whole = ((0, 0, 0), d)

    def F(points=((4, 3, 2),), r2=4, **kw):
        kw.setdefault("box", whole)
        return scene.Brush(points, r2, **kw)

    rows = [("one point", F(), d, True), ("empty box", F(box=((3, 0, 0), (3, 7, 5))), d, True), ("r2 0", F(r2=0), d, True), ("r2 2^32 - 1", F(r2=2 ** 32 - 1), d, True),
            ("both flags", F(flags=17), d, True), ("flag 2", F(flags=2), d, False), ("flag 32", F(flags=32), d, False), ("flag 2^31", F(flags=1 << 31), d, False),
            ("window 0..0", F(window=(0, 0)), d, True), ("window 7..6", F(window=(7, 6)), d, False), ("window 0..256", F(window=(0, 256)), d, False),
            ("weights 64", F(weight=(64, 64, 64)), d, True), ("256 points", F([(1, 1, 1)] * 256), d, True),
            ("the far corner", F([(8, 6, 4)]), d, True), ("a lift on the first point", F([(1, 1, 1, 1), (2, 2, 2, 1)]), d, True),
            ("point flag 2", F([(1, 1, 1, 2)]), d, False), ("point flag 3", F([(1, 1, 1), (1, 1, 1, 3)]), d, False),
            ("no point", F([]), d, False),
            ("the largest volume", F([(4095, 4095, 4095), (0, 0, 0)], box=((0, 0, 0), (4096, 4096, 4096))), (4096, 4096, 4096), True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, F(box=((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, F(box=(tuple(lo), tuple(hi))), d, False))
        p = [1, 1, 1]; p[a] = d[a]
        rows.append(("a point outside on axis %d" % a, F([(1, 1, 1), tuple(p)]), d, False))
        for w in (0, 65):
            wt = [1, 1, 1]; wt[a] = w
            rows.append(("weight %d on axis %d" % (w, a), F(weight=tuple(wt)), d, False))
    return rows


def test_the_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    box = (C.c_uint32 * 6)()
    for name, b, dims, valid in _check_rows():
        cd = (C.c_uint32 * 3)(*dims)
        rc = volym_lib.volym_brush_check(C.byref(b.to_c()), cd)
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        assert volym_lib.volym_brush_box(C.byref(b.to_c()), cd, box) == rc, name
        if valid:
            assert scene.check_brush(b, dims) is b, name
        else:
            with pytest.raises(ValueError):
                scene.check_brush(b, dims)
    one = scene.Brush([(0, 0, 0)], 1, dims=(1, 1, 1))
    assert volym_lib.volym_brush_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_brush_check(C.byref(one.to_c()), None) == E_INVALID
    assert volym_lib.volym_brush_box(C.byref(one.to_c()), (C.c_uint32 * 3)(1, 1, 1), None) == E_INVALID
    c = one.to_c()
    c.n_points = 257                                                   # (what the Python face cannot say)
    assert volym_lib.volym_brush_check(C.byref(c), (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    with pytest.raises(ValueError):
        scene.Brush([(1, 1, 1)] * 257, 1, dims=(2, 2, 2)).to_c()
    with pytest.raises(ValueError):
        scene.Brush([(70000, 1, 1)], 1, dims=(2, 2, 2)).to_c()
    with pytest.raises(ValueError):
        scene.Brush([(1, 1, 1)], 2 ** 32, dims=(2, 2, 2)).to_c()
    assert one.replace(r2=9).r2 == 9 and one.replace(r2=9).points == one.points
    with pytest.raises(TypeError):
        one.replace(ids=(1, 1))


def _random_brush(rng, dims, n_points=None, r2_max=100, box=True):
    from volym_amd import _lib, scene
    n = int(rng.integers(1, 7)) if n_points is None else n_points
    pts = [tuple(int(rng.integers(0, d)) for d in dims) + (int(rng.integers(0, 4) == 0),) for _ in range(n)]
    lo = [int(rng.integers(0, d + 1)) for d in dims] if box else [0, 0, 0]
    hi = [int(rng.integers(l, d + 1)) for l, d in zip(lo, dims)] if box else list(dims)
    weight = tuple(int(v) for v in rng.choice([1, 1, 2, 4, 9, 25, 64], 3))
    return scene.Brush(pts, int(rng.integers(0, r2_max + 1)), (tuple(lo), tuple(hi)), 0, (0, 255), rng.integers(0, 256, 256), weight)


def test_the_box_and_its_twin_agree_and_hold_the_stroke(volym_lib):
    from volym_amd import scene
    rng = np.random.default_rng(11)
    out = (C.c_uint32 * 6)()
    met = 0
    for k in range(300):
        dims = tuple(int(v) for v in rng.integers(1, 40, 3)) if k % 3 else (4096, 4096, 4096)
        b = _random_brush(rng, dims, r2_max=(2 ** 32 - 1 if k % 7 == 0 else 400))
        assert volym_lib.volym_brush_box(C.byref(b.to_c()), (C.c_uint32 * 3)(*dims), out) == 0
        lo, hi = scene.brush_box(b, dims)
        assert list(out) == list(lo) + list(hi), (k, list(out), lo, hi)
        met += lo != hi
        if dims[0] < 4096:                                             # no texel of the box within the stroke lies outside the cut box
            inside = scene.brush_mask(b, dims)
            (x0, y0, z0), (x1, y1, z1) = b.box
            boxed = np.zeros_like(inside)
            boxed[z0:z1, y0:y1, x0:x1] = inside[z0:z1, y0:y1, x0:x1]
            boxed[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = False
            assert not boxed.any(), (k, b.points, b.r2, b.weight)
    assert 50 < met < 300
    for r2, w, want in ((0, 1, 0), (24, 1, 4), (25, 1, 5), (25, 25, 1), (24, 25, 0), (2 ** 32 - 1, 1, 65535), (2 ** 32 - 1, 64, 8191)):
        assert scene.brush_reach(r2, w) == want and w * (want + 1) ** 2 > r2 >= w * want * want


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def _exact_d2(t, a, b, weight):
    """the squared weighted distance from t to the closest point of segment (a, b), as a Fraction"""
    dot = lambda u, v: sum(Fraction(weight[k]) * u[k] * v[k] for k in range(3))
    d = [Fraction(b[k] - a[k]) for k in range(3)]
    w = [Fraction(t[k] - a[k]) for k in range(3)]
    dd = dot(d, d)
    s = Fraction(0) if dd == 0 else min(max(dot(w, d) / dd, Fraction(0)), Fraction(1))
    u = [w[k] - s * d[k] for k in range(3)]
    return dot(u, u)


def test_the_integer_rule_is_the_closest_point_distance_in_exact_fractions():
    from volym_amd import scene
    rng = np.random.default_rng(3)
    dims = (9, 8, 7)
    texels = list(itertools.product(range(dims[0]), range(dims[1]), range(dims[2])))
    inside = 0
    for k in range(200):
        a = tuple(int(rng.integers(0, d)) for d in dims)
        b = a if k % 10 == 0 else tuple(int(rng.integers(0, d)) for d in dims)
        weight = tuple(int(v) for v in rng.integers(1, 65, 3))
        r2 = int(rng.integers(0, 101))
        for t in texels:
            got = scene.brush_within(t, a, b, weight, r2)
            assert got == (_exact_d2(t, a, b, weight) <= r2), (t, a, b, weight, r2)
            inside += got
    assert inside > 2000
    # the largest operands the header allows: every product stays below 2^64
    far, w = (4095, 4095, 4095), (64, 64, 64)
    dd = 3 * 64 * 4095 ** 2
    assert dd < 2 ** 32 and (2 ** 32 - 1) * dd < 2 ** 64 and dd * dd < 2 ** 64
    assert scene.brush_within((0, 4095, 0), (0, 0, 0), far, w, 2 ** 32 - 1) == (_exact_d2((0, 4095, 0), (0, 0, 0), far, w) <= 2 ** 32 - 1)


def _by_the_rule(vol, uncut, dims, b, labels):
    """the rule of include/volym_hip.h, a texel at a time over Python integers"""
    from volym_amd import _lib, scene
    nx, ny, nz = dims
    new = np.array(labels, np.uint8).reshape(nz, ny, nx).copy()
    old = new.copy()
    src = (uncut if b.flags & _lib.BRUSH_UNCUT else vol).reshape(nz, ny, nx)
    segments = scene.brush_segments(b)
    changed, left, arrived, hull = 0, [0] * 256, [0] * 256, None
    (x0, y0, z0), (x1, y1, z1) = b.box
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                l = int(old[z, y, x])
                to = int(b.to[l])
                if to == l or not b.window[0] <= int(src[z, y, x]) <= b.window[1]:
                    continue
                if not any(scene.brush_within((x, y, z), p, q, b.weight, b.r2) for p, q in segments):
                    continue
                changed += 1
                left[l] += 1
                arrived[to] += 1
                hull = (x, y, z, x + 1, y + 1, z + 1) if hull is None else tuple(min(h, v) for h, v in zip(hull[:3], (x, y, z))) + tuple(max(h, v + 1) for h, v in zip(hull[3:], (x, y, z)))
                if not b.flags & _lib.BRUSH_DRY_RUN:
                    new[z, y, x] = to
    return new, changed, left, arrived, hull or (0,) * 6


def test_the_twin_is_the_rule_on_random_requests_over_every_flag_combination():
    from volym_amd import _lib, scene
    rng = np.random.default_rng(17)
    dims = (11, 7, 6)
    n = dims[0] * dims[1] * dims[2]
    total = 0
    for k in range(80):
        vol, uncut = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
        labels = rng.integers(0, 6, n).astype(np.uint8)
        lo = rng.integers(0, 200)
        b = _random_brush(rng, dims, r2_max=60, box=k % 8 >= 4).replace(flags=(0, 1, 16, 17)[k % 4], window=(int(lo), int(rng.integers(lo, 256))) if k % 3 else (0, 255))
        new, res = scene.brush_volume(vol, dims, b, labels, uncut=uncut)
        want, changed, left, arrived, hull = _by_the_rule(vol, uncut, dims, b, labels)
        assert np.array_equal(new, want), k
        assert int(res["changed"]) == changed and res["left"].tolist() == left and res["arrived"].tolist() == arrived and res["box"].tolist() == list(hull), k
        assert sum(left) == sum(arrived) == changed
        if b.flags & _lib.BRUSH_DRY_RUN:
            assert np.array_equal(new.ravel(), labels)
        total += changed
    assert total > 500


def test_closed_forms():
    from volym_amd import _lib, scene
    host = RS.scene_a()
    dims = host.dims
    uncut = np.random.default_rng(1).integers(0, 256, host.vol.size).astype(np.uint8)
    # an r2 that covers the box: the relabel of the same table, window and box
    for box, window, flags in ((BS.MS.BOXES["x 5..30"], (40, 200), 0), (BS.MS.BOXES["whole"], (0, 255), _lib.BRUSH_UNCUT)):
        b = scene.Brush([(18, 10, 9)], 3 * 37 * 37, box, flags, window, {0: 3, 1: 3, 4: 2})
        r = scene.Relabel(box, flags, window, {0: 3, 1: 3, 4: 2})
        got, want = scene.brush_volume(host.vol, dims, b, host.labels, uncut=uncut), scene.relabel_volume(host.vol, dims, r, host.labels, uncut=uncut)
        assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and int(got[1]["changed"]) > 1000
    for case in BS.cases():
        new, res = BS.expect(host, case)
        assert int(res["left"].sum()) == int(res["arrived"].sum()) == int(res["changed"]), case.name
        # the same stroke with its points reversed (a LIFT moves to the other end of the gap it marks)
        pts = case.brush.points
        rev = [pts[i][:3] + ((pts[i + 1][3] if i + 1 < len(pts) else 0),) for i in range(len(pts) - 1, -1, -1)]
        back, res_back = BS.expect(host, case, case.brush.replace(points=rev))
        assert np.array_equal(new, back) and res.tobytes() == res_back.tobytes(), case.name
    # a LIFT on every point: the union of the balls
    pts = [(5, 5, 5), (9, 8, 6), (20, 12, 10), (22, 12, 10)]
    lifted = scene.Brush([p + (1,) for p in pts], 10, to=BS.every(7), dims=dims)
    union = np.zeros(host.labels.size, bool)
    for p in pts:
        union |= scene.brush_volume(host.vol, dims, scene.Brush([p], 10, to=BS.every(7), dims=dims), host.labels)[0].ravel() == 7
    assert np.array_equal(scene.brush_volume(host.vol, dims, lifted, host.labels)[0].ravel() == 7, union) and union.sum() > 300
    assert (scene.brush_volume(host.vol, dims, lifted.replace(points=pts), host.labels)[0].ravel() == 7).sum() > union.sum()


# ---- what the device tests rely on ----------------------------------------------------------------------------------------------
def test_the_counts_of_the_issue():
    from volym_amd import scene
    for case in BS.cases():
        if case.count is not None:
            assert int(scene.brush_mask(case.brush, BS.DIMS).sum()) == case.count, case.name
    assert sum(c.count is not None for c in BS.cases()) == 5


@pytest.mark.parametrize("which", list(BS.SCENES))
def test_the_cases_do_what_the_device_tests_need(which):
    host = BS.SCENES[which]()
    seen = set()
    for case in BS.cases(host.dims):
        new, res = BS.expect(host, case)
        dry = case.name == "dry run"
        # (scene B's random labels and the ragged scene's far-off shell and core give the swap of 1 and 2 little to do, and the ragged
        # scene's density the windows: there the strokes without a window whose table moves every label carry the weight)
        plain = not case.name.startswith("two crossing") and case.brush.window == (0, 255)
        if not case.trivial and (which == "a" or plain):
            assert int(res["changed"]) >= 50, (which, case.name, int(res["changed"]))
        if case.trivial and case.name != "single texel":
            assert int(res["changed"]) == 0, case.name
        if dry:
            assert np.array_equal(new, host.labels)
        if case.ragged and which == "ragged":
            assert RS.wrapping_chunks(host.dims, host.labels, new) > 0, case.name
        seen.add(case.name)
    assert len(seen) == 20
    if which == "a":
        # the swap: texels under both capsules exist, and each is swapped once
        from volym_amd import scene
        case = next(c for c in BS.cases() if c.name.startswith("two crossing"))
        a, b = case.brush.replace(points=case.brush.points[:2]), case.brush.replace(points=[p[:3] for p in case.brush.points[2:]])
        both = scene.brush_mask(a, host.dims) & scene.brush_mask(b, host.dims)
        lab = host.labels.reshape(both.shape)
        under = both & ((lab == 1) | (lab == 2))
        assert under.sum() >= 5
        new, _ = BS.expect(host, case)
        assert np.array_equal(new.reshape(both.shape)[under], 3 - lab[under])


def test_the_small_scene_shares_rows_within_chunks():
    """what tests/test_gpu_brush.py's small-shape test relies on: a slice is smaller than a chunk, every stroke changes a texel but
    not all, and a changed texel lies in a row above the first of a chunk that starts in row 0"""
    host = BS.scene_small()
    nx, ny, nz = host.dims
    assert host.dims == (5, 3, 9) and nx * ny < 16 and (nx * ny * nz) % 16 != 0
    assert host.vol.min() >= 1 and sorted(set(host.labels.tolist())) == [0, 1, 2]
    assert [c.name for c in BS.small_cases()] == ["ball of r2 2 at the centre", "capsule along z, r2 1", "capsule along z, r2 1, a window 64..192"]
    changed = []
    for case in BS.small_cases():
        new, res = BS.expect(host, case)
        assert 1 <= int(res["changed"]) < nx * ny * nz, case.name
        assert BS.rows_shared(host.dims, host.labels, new) >= 1, case.name
        changed.append(int(res["changed"]))
    assert changed[2] < changed[1]                                      # the window leaves texels of the capsule out
