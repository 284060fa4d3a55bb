"""The measure pass without a GPU: the C structs and constants, volym_measure_check against scene.check_measure, the host twin
scene.measure_volume against a plain triple loop, closed forms and identities, scene.segment_summary against NumPy, and the
conditions on the scenes that tests/test_gpu_measure.py relies on (asserted here on the twin, where they cost nothing).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import measure_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
INT32_MAX = 2 ** 31 - 1

STATS_LAYOUT = [("count", 0, 8), ("sum", 8, 8), ("sum_sq", 16, 8), ("sum_x", 24, 8), ("sum_y", 32, 8), ("sum_z", 40, 8), ("box", 48, 24), ("min", 72, 4),
                ("max", 76, 4)]
MEASURE_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("group", 28, 256)]


class NoContext:
    """stands where a GpuContext stands in Host.set_cut: the host record alone changes"""
    def set_crop_box(self, lo, hi): pass
    def set_clip_plane(self, n, d): pass
    def set_segment_visibility(self, v): pass


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Measure) == 284 and C.sizeof(_lib.SegmentStats) == 80 and C.sizeof(_lib.Measurement) == 36864
    assert _lib.SEGMENT_STATS_DTYPE.itemsize == 80
    for f, off, size in STATS_LAYOUT:
        d = getattr(_lib.SegmentStats, f)
        assert (d.offset, d.size) == (off, size), f
        assert _lib.SEGMENT_STATS_DTYPE.fields[f][1] == off, f
    for f, off, size in MEASURE_LAYOUT:
        d = getattr(_lib.Measure, f)
        assert (d.offset, d.size) == (off, size), f
    assert _lib.Measurement.hist.offset == 20480
    assert (_lib.MEASURE_UNCUT, _lib.MEASURE_GROUPS, _lib.MEASURE_NO_GROUP) == (1, 8, 255)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(volym_measure), sizeof(struct volym_segment_stats), sizeof(struct volym_measurement));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_measure, %s));\n' % f for f, _, _ in MEASURE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_segment_stats, %s));\n' % f for f, _, _ in STATS_LAYOUT) +
                   '  printf(" %zu", offsetof(struct volym_measurement, hist));\n'
                   '  printf(" %d %d %d %d", VOLYM_MEASURE_UNCUT, VOLYM_MEASURE_GROUPS, VOLYM_MEASURE_NO_GROUP, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [284, 80, 36864] + [o for _, o, _ in MEASURE_LAYOUT] + [o for _, o, _ in STATS_LAYOUT] + [20480, 1, 8, 255, 2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_measure_pass", "volym_read_measure", "volym_measure_device_ptr", "volym_measure_check"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("measure_pass", "read_measure", "measure_device_ptr"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("measure", "histogram", "measure_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Measure", "check_measure", "measure_volume", "segment_summary"):
        assert callable(getattr(scene, name))


def _check_rows():
    """(name, measure, dims, valid)"""
    from volym_amd import scene
    d = (9, 7, 5)
    M = scene.Measure
    g = np.zeros(256, np.int64)
    rows = [("whole", M(((0, 0, 0), d)), d, True), ("empty on x", M(((3, 0, 0), (3, 7, 5))), d, True), ("empty at the far corner", M((d, d)), d, True),
            ("one texel", M(((8, 6, 4), d)), d, True), ("uncut", M(((0, 0, 0), d), 1), d, True), ("flag 2", M(((0, 0, 0), d), 2), d, False),
            ("flag 3", M(((0, 0, 0), d), 3), d, False), ("flag 2^31", M(((0, 0, 0), d), 1 << 31), d, False)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond axis %d" % a, M(((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 3; hi = list(d); hi[a] = 2
        rows.append(("lo above hi on axis %d" % a, M((tuple(lo), tuple(hi))), d, False))
    for v, ok in ((0, True), (7, True), (8, False), (9, False), (128, False), (254, False), (255, True)):
        for at in (0, 131, 255):
            t = g.copy(); t[at] = v
            rows.append(("group[%d] = %d" % (at, v), M(((1, 1, 1), (4, 4, 4)), 0, t), d, ok))
    rows.append(("4096 cubed", M(((0, 0, 0), (4096, 4096, 4096))), (4096, 4096, 4096), True))
    return rows


def test_check_agrees_with_python_on_every_row(volym_lib):
    from volym_amd import scene
    rows = _check_rows()
    assert sum(ok for *_, ok in rows) >= 10 and sum(not ok for *_, ok in rows) >= 15
    for name, m, dims, ok in rows:
        rc = volym_lib.volym_measure_check(C.byref(m.to_c()), (C.c_uint32 * 3)(*dims))
        assert rc == (0 if ok else E_INVALID), name
        if ok:
            assert scene.check_measure(m, dims) is m, name
        else:
            with pytest.raises(ValueError):
                scene.check_measure(m, dims)
    ok = scene.Measure(((0, 0, 0), (1, 1, 1))).to_c()
    assert volym_lib.volym_measure_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_measure_check(C.byref(ok), None) == E_INVALID
    with pytest.raises(ValueError):
        scene.Measure(((0, 0, 0), (1, 1, 1)), 0, np.full(256, 256)).to_c()
    with pytest.raises(ValueError):
        scene.Measure(((0, 0, 0), (1, 1, 1)), 0, np.zeros(255)).to_c()


# ---- the twin against the rule ------------------------------------------------------------------------------------------------
def _loop(vol, dims, m, labels, cut, uncut):
    """the rule of include/volym_hip.h as a plain triple loop over Python integers"""
    nx, ny, nz = dims
    seg = [dict(count=0, sum=0, sum_sq=0, sum_x=0, sum_y=0, sum_z=0, box=[INT32_MAX] * 3 + [-1] * 3, min=255, max=0) for _ in range(256)]
    hist = [[0] * 256 for _ in range(8)]
    whole = bool(m.flags & 1)
    src = uncut if (whole and uncut is not None) else vol
    (x0, y0, z0), (x1, y1, z1) = m.box
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                at = (z * ny + y) * nx + x
                l = int(labels[at]) if labels is not None else 0
                if not whole and cut:
                    if cut.get("box") is not None:
                        lo, hi = cut["box"]
                        if not all(lo[a] <= t < hi[a] for a, t in enumerate((x, y, z))):
                            continue
                    if cut.get("plane") is not None:
                        n, d = cut["plane"]
                        if n[0] * x + n[1] * y + n[2] * z > d:
                            continue
                    if cut.get("visible") is not None and labels is not None and not cut["visible"][l]:
                        continue
                b = int(src[at])
                s = seg[l]
                s["count"] += 1; s["sum"] += b; s["sum_sq"] += b * b
                s["sum_x"] += x; s["sum_y"] += y; s["sum_z"] += z
                s["min"], s["max"] = min(s["min"], b), max(s["max"], b)
                for a, t in enumerate((x, y, z)):
                    s["box"][a], s["box"][3 + a] = min(s["box"][a], t), max(s["box"][3 + a], t)
                g = int(m.group[l])
                if g != 255:
                    hist[g][b] += 1
    return seg, hist


def _equal_to_loop(got, want):
    rec, hist = got
    seg, h = want
    for l in range(256):
        for k in ("count", "sum", "sum_sq", "sum_x", "sum_y", "sum_z", "min", "max"):
            assert int(rec[k][l]) == seg[l][k], (l, k)
        assert [int(v) for v in rec["box"][l]] == seg[l]["box"], l
    assert hist.dtype == np.uint64 and hist.shape == (8, 256)
    assert hist.tolist() == h


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("with_labels", [True, False])
def test_twin_equals_the_rule_texel_by_texel(flags, with_labels):
    from volym_amd import scene
    dims = (9, 7, 5)
    rng = np.random.default_rng(3)
    n = dims[0] * dims[1] * dims[2]
    uncut = rng.integers(0, 256, n).astype(np.uint8)
    labels = rng.integers(0, 12, n).astype(np.uint8) if with_labels else None
    cut = {"box": ((1, 0, 1), (8, 6, 5)), "plane": ((2, -1, 3), 11), "visible": scene.visibility_mask([4])}
    now = scene.cut_volume(uncut, dims, cut, labels)
    group = np.full(256, 255, np.int64)
    group[:12] = np.arange(12) % 8
    group[3] = 255
    seen = set()
    for box in (((0, 0, 0), dims), ((2, 1, 0), (7, 7, 4)), ((4, 3, 2), (5, 4, 3)), ((3, 3, 3), (3, 7, 5))):
        m = scene.Measure(box, flags, group)
        got = scene.measure_volume(now, dims, m, labels=labels, cut=cut, uncut=uncut)
        _equal_to_loop(got, _loop(now, dims, m, labels, cut, uncut))
        seen.add(S.as_bytes(got))
        # without an uncut copy UNCUT reads the bytes as they stand
        _equal_to_loop(scene.measure_volume(now, dims, m, labels=labels, cut=cut), _loop(now, dims, m, labels, cut, None))
    assert len(seen) == 4
    assert len(S.as_bytes(got)) == 36864


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def _is_empty(rec, l):
    return (int(rec["count"][l]), int(rec["sum"][l]), int(rec["sum_sq"][l]), int(rec["sum_x"][l]), int(rec["sum_y"][l]), int(rec["sum_z"][l]),
            int(rec["min"][l]), int(rec["max"][l]), rec["box"][l].tolist()) == (0, 0, 0, 0, 0, 0, 255, 0, [INT32_MAX] * 3 + [-1] * 3)


@pytest.mark.parametrize("c", [0, 1, 200, 255])
def test_a_constant_cube(c):
    from volym_amd import scene
    dims = (6, 5, 4)
    n = 6 * 5 * 4
    rec, hist = scene.measure_volume(np.full(n, c, np.uint8), dims, scene.Measure(dims=dims))
    r = rec[0]
    assert (int(r["count"]), int(r["sum"]), int(r["sum_sq"])) == (n, c * n, c * c * n)
    assert [2 * int(r[k]) for k in ("sum_x", "sum_y", "sum_z")] == [n * (d - 1) for d in dims]
    assert (int(r["min"]), int(r["max"]), r["box"].tolist()) == (c, c, [0, 0, 0, 5, 4, 3])
    assert int(hist[0][c]) == n and int(hist.sum()) == n
    assert all(_is_empty(rec, l) for l in range(1, 256))


def test_one_bright_voxel_and_an_empty_box():
    from volym_amd import scene
    dims = (6, 5, 4)
    vol = np.zeros(6 * 5 * 4, np.uint8)
    labels = np.zeros_like(vol)
    at = (3 * 5 + 2) * 6 + 4                 # texel (4, 2, 3)
    vol[at], labels[at] = 201, 9
    rec, hist = scene.measure_volume(vol, dims, scene.Measure(dims=dims, group=scene.measure_groups([0], [9])), labels=labels)
    r = rec[9]
    assert (int(r["count"]), int(r["sum"]), int(r["sum_sq"]), int(r["sum_x"]), int(r["sum_y"]), int(r["sum_z"])) == (1, 201, 201 * 201, 4, 2, 3)
    assert (int(r["min"]), int(r["max"]), r["box"].tolist()) == (201, 201, [4, 2, 3, 4, 2, 3])
    assert int(rec["count"][0]) == 119 and int(rec["max"][0]) == 0 and int(rec["min"][0]) == 0
    assert int(hist[1][201]) == 1 and int(hist[1].sum()) == 1 and int(hist[0][0]) == 119 and int(hist[2:].sum()) == 0
    rec, hist = scene.measure_volume(vol, dims, scene.Measure(((2, 2, 2), (2, 5, 4))), labels=labels)
    assert all(_is_empty(rec, l) for l in range(256)) and int(hist.sum()) == 0
    assert S.as_bytes((rec, hist)) == S.as_bytes(scene.empty_measurement())


# ---- identities ---------------------------------------------------------------------------------------------------------------
def _identities(rec, hist, group):
    values = np.arange(256, dtype=np.uint64)
    for g in range(8):
        members = np.flatnonzero(np.asarray(group) == g)
        assert int(hist[g].sum()) == int(rec["count"][members].sum()), g
        assert int((hist[g] * values).sum()) == int(rec["sum"][members].sum()), g
        assert int((hist[g] * values * values).sum()) == int(rec["sum_sq"][members].sum()), g


def test_histograms_and_records_agree_in_every_group():
    from volym_amd import scene
    for host in (S.scene_a(), S.scene_b()):
        host.set_cut(NoContext(), S.BOX, S.PLANE, S.HIDDEN)
        for name, m in S.measures():
            rec, hist = S.expect(host, m)
            _identities(rec, hist, m.group)


def test_uncut_over_the_whole_volume_counts_what_the_label_statistics_count():
    """count == the voxel count per label and box == its texel box: what volym_label_counts and the label boxes hold"""
    from volym_amd import scene
    for host in (S.scene_a(), S.scene_b()):
        host.set_cut(NoContext(), S.BOX, S.PLANE, S.HIDDEN)
        rec, _ = S.expect(host, scene.Measure(dims=S.DIMS, flags=1))
        assert rec["count"].tolist() == np.bincount(host.labels, minlength=256).tolist()
        lab = host.labels.reshape(S.NZ, S.NY, S.NX)
        for l in np.flatnonzero(rec["count"]):
            z, y, x = np.nonzero(lab == l)
            assert rec["box"][l].tolist() == [x.min(), y.min(), z.min(), x.max(), y.max(), z.max()], l


# ---- the summary --------------------------------------------------------------------------------------------------------------
def test_segment_summary_against_numpy():
    from volym_amd import scene
    host = S.scene_a()
    rec, _ = S.expect(host, scene.Measure(S.BOXES["x 5..30"]))
    (x0, y0, z0), (x1, y1, z1) = S.BOXES["x 5..30"]
    vol = host.vol.reshape(S.NZ, S.NY, S.NX)[z0:z1, y0:y1, x0:x1].astype(np.float64)
    lab = host.labels.reshape(S.NZ, S.NY, S.NX)[z0:z1, y0:y1, x0:x1]
    spacing = (0.5, 0.25, 2.0)
    rel = lambda a, b: abs(a - b) <= 1e-12 * abs(b)
    for l in range(5):
        s = scene.segment_summary(rec[l], spacing)
        sel = lab == l
        z, y, x = np.nonzero(sel)
        assert s["count"] == int(sel.sum()) and isinstance(s["count"], int)
        assert rel(s["mean"], float(vol[sel].mean())) and rel(s["std"], float(vol[sel].std())) and isinstance(s["mean"], float)
        assert (s["min"], s["max"]) == (int(vol[sel].min()), int(vol[sel].max()))
        for a, (v, o) in enumerate(((x, x0), (y, y0), (z, z0))):
            assert rel(s["centroid"][a], float((v + o).mean()))
            assert rel(s["centre"][a], (float((v + o).mean()) + 0.5) * spacing[a])
        assert s["box"] == ((x.min() + x0, y.min() + y0, z.min() + z0), (x.max() + x0, y.max() + y0, z.max() + z0))
        assert rel(s["volume"], sel.sum() * 0.25)
    assert scene.segment_summary(rec[77]) is None
    # a constant segment: the deviation is exactly 0, not the square root of a rounding error
    rec, _ = scene.measure_volume(np.full(1000, 173, np.uint8), (10, 10, 10), scene.Measure(dims=(10, 10, 10)))
    assert scene.segment_summary(rec[0])["std"] == 0.0


# ---- the conditions the device tests rely on ----------------------------------------------------------------------------------
def test_the_scenes_of_the_device_tests_are_what_those_tests_need():
    from volym_amd import scene
    a, b = S.scene_a(), S.scene_b()
    assert a.dims == S.DIMS == (37, 22, 19) and all(d % 4 for d in S.DIMS) and S.NX % 16 and (S.NX * S.NY) % 16
    assert a.vol.min() >= 1 and np.array_equal(a.vol, b.vol)
    assert sorted(np.unique(a.labels)) == [0, 1, 2, 3, 4]
    assert (np.bincount(b.labels, minlength=256) > 0).sum() >= 250
    rec, _ = S.expect(b, scene.Measure(dims=S.DIMS))
    assert (rec["count"] > 0).sum() >= 250
    # the walks: one run, a run per z, a run per row
    assert len(S.linear_runs(S.BOXES["whole"])) == 1 and len(S.linear_runs(S.BOXES["rows"])) == 13 and len(S.linear_runs(S.BOXES["x 3..8"])) == 19 * 14
    # The double-count trap: a chunk that holds texels of two consecutive runs.  Two rows of a box lie nx - width bytes apart, so a
    # 16-byte chunk can hold the end of one and the start of the next only when nx - width <= 14: at x in [5, 30) (12 apart), never at
    # x in [3, 8) of a 37-texel row (32 apart), where the trap cannot spring and the assertion asked for it cannot hold.
    assert S.shared_chunks(S.BOXES["x 5..30"]) >= 1
    assert S.shared_chunks(S.BOXES["x 3..8"]) == 0
    # every cut removes at least a tenth of the texels and leaves at least a tenth
    total = S.NX * S.NY * S.NZ
    for name, box, plane, hidden in S.CUTS:
        a.set_cut(NoContext(), box, plane, hidden)
        rec, hist = S.expect(a, scene.Measure(dims=S.DIMS))
        kept = int(rec["count"].sum())
        assert kept == int(hist[0].sum())
        if box or plane or hidden:
            assert total // 10 <= kept <= total - total // 10, (name, kept, total)
        else:
            assert kept == total, name
    # no two requests of the list give the same result, so a result that carried over from another pass would show
    a.set_cut(NoContext(), S.BOX, S.PLANE, S.HIDDEN)
    results = [S.as_bytes(S.expect(a, m)) for _, m in S.measures()]
    assert len(set(results)) == len(results)
