"""The label edit without a GPU: the C structs and constants, volym_relabel_check against scene.check_relabel, the host twin
scene.relabel_volume against a plain triple loop over Python integers, the closed forms that tie an edit to the distance and the
components passes, and the conditions tests/test_gpu_relabel.py relies on, asserted on the twin.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import relabel_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

REQUEST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("to", 36, 256), ("id_lo", 292, 4), ("id_hi", 296, 4),
                  ("d2_lo", 300, 4), ("d2_hi", 304, 4)]
RESULT_LAYOUT = [("changed", 0, 8), ("left", 8, 2048), ("arrived", 2056, 2048), ("box", 4104, 24)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Relabel) == 308 and C.sizeof(_lib.RelabelResult) == 4128 and _lib.RELABEL_RESULT_DTYPE.itemsize == 4128
    for struct, dtype, layout in ((_lib.Relabel, None, REQUEST_LAYOUT), (_lib.RelabelResult, _lib.RELABEL_RESULT_DTYPE, RESULT_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    consts = [_lib.RELABEL_UNCUT, _lib.RELABEL_IDS, _lib.RELABEL_IDS_EXCEPT, _lib.RELABEL_DISTANCE, _lib.RELABEL_DRY_RUN]
    assert consts == [1, 2, 4, 8, 16]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(volym_relabel), sizeof(struct volym_relabel_result));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_relabel, %s));\n' % f for f, _, _ in REQUEST_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_relabel_result, %s));\n' % f for f, _, _ in RESULT_LAYOUT) +
                   '  printf(" %d %d %d %d %d %d", VOLYM_RELABEL_UNCUT, VOLYM_RELABEL_IDS, VOLYM_RELABEL_IDS_EXCEPT, VOLYM_RELABEL_DISTANCE,\n'
                   '         VOLYM_RELABEL_DRY_RUN, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [308, 4128] + [o for _, o, _ in REQUEST_LAYOUT] + [o for _, o, _ in RESULT_LAYOUT] + consts + [2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_edit_labels", "volym_relabel_check", "volym_read_labels"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("edit_labels", "read_labels"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("relabel", "split_at", "keep_largest", "grow", "shrink", "paint", "save_labels"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Relabel", "check_relabel", "relabel_table", "relabel_volume"):
        assert callable(getattr(scene, name))
    header = open(os.path.join(ROOT, "include", "volym_hip.h")).read()
    assert "volym_mgpu_*) has no forward for this call" in header


def _check_rows():
    """(name, request, dims, valid)"""
    from volym_amd import scene
    d = (9, 7, 5)
    F = scene.Relabel
    whole = ((0, 0, 0), d)
    rows = [("whole", F(whole), d, True), ("empty on x", F(((3, 0, 0), (3, 7, 5))), d, True), ("empty at the far corner", F((d, d)), d, True),
            ("one texel", F(((8, 6, 4), d)), d, True), ("the largest volume", F(((0, 0, 0), (4096, 4096, 4096))), (4096, 4096, 4096), True),
            ("every flag", F(whole, 31), d, True), ("dry run alone", F(whole, 16), d, True), ("uncut alone", F(whole, 1), d, True),
            ("flag 32", F(whole, 32), d, False), ("flag 2^31", F(whole, 1 << 31), d, False),
            ("except without ids", F(whole, 4), d, False), ("except with ids", F(whole, 6), d, True), ("except with distance only", F(whole, 12), d, False),
            ("window 0..0", F(whole, window=(0, 0)), d, True), ("window 255..255", F(whole, window=(255, 255)), d, True),
            ("window 7..6", F(whole, window=(7, 6)), d, False), ("window 0..256", F(whole, window=(0, 256)), d, False),
            ("window 256..300", F(whole, window=(256, 300)), d, False),
            ("ids 5..5", F(whole, 2, ids=(5, 5)), d, True), ("ids 6..5", F(whole, 2, ids=(6, 5)), d, False), ("ids 6..5 without the flag", F(whole, 0, ids=(6, 5)), d, True),
            ("ids up to 2^32 - 1", F(whole, 2, ids=(0, 2 ** 32 - 1)), d, True),
            ("d2 9..9", F(whole, 8, d2=(9, 9)), d, True), ("d2 10..9", F(whole, 8, d2=(10, 9)), d, False), ("d2 10..9 without the flag", F(whole, 2, d2=(10, 9)), d, True),
            ("a table onto one label", F(whole, to=np.full(256, 255)), d, True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, F(((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, F((tuple(lo), tuple(hi))), d, False))
    return rows


def test_the_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    for name, r, dims, valid in _check_rows():
        rc = volym_lib.volym_relabel_check(C.byref(r.to_c()), (C.c_uint32 * 3)(*dims))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_relabel(r, dims) is r, name
        else:
            with pytest.raises(ValueError):
                scene.check_relabel(r, dims)
    assert volym_lib.volym_relabel_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_relabel_check(C.byref(scene.Relabel(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    with pytest.raises(ValueError):
        scene.Relabel(dims=(2, 2, 2), to=np.full(256, 256)).to_c()
    with pytest.raises(ValueError):
        scene.Relabel(dims=(2, 2, 2), to=np.zeros(255)).to_c()
    with pytest.raises(ValueError):
        scene.relabel_table({3: 256})
    assert scene.relabel_table({3: 9, 9: 3}).tolist() == [9 if l == 3 else 3 if l == 9 else l for l in range(256)]
    r = scene.Relabel(dims=(2, 2, 2), to={1: 2})
    assert r.replace(window=(3, 4)).window == (3, 4) and r.replace(window=(3, 4)).to.tolist() == r.to.tolist()
    with pytest.raises(TypeError):
        r.replace(weight=(1, 1, 1))


# ---- the twin against the rule --------------------------------------------------------------------------------------------------
def _by_the_rule(vol, uncut, dims, r, labels, ids, ids_box, dmap, dmap_box):
    """the rule of include/volym_hip.h, a texel at a time over Python integers"""
    from volym_amd import _lib
    nx, ny, nz = dims
    (x0, y0, z0), (x1, y1, z1) = r.box
    new = [int(v) for v in labels]
    src = uncut if r.flags & _lib.RELABEL_UNCUT else vol
    changed, left, arrived = 0, [0] * 256, [0] * 256
    hull = None
    to = [int(v) for v in r.to]

    def at(snap, box, x, y, z):
        (a0, b0, c0), (a1, b1, _c1) = box
        return int(snap.ravel()[(x - a0) + (a1 - a0) * ((y - b0) + (b1 - b0) * (z - c0))])

    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                i = x + nx * (y + ny * z)
                l = int(labels[i])
                if to[l] == l or not r.window[0] <= int(src[i]) <= r.window[1]:
                    continue
                if r.flags & _lib.RELABEL_IDS:
                    k = at(ids, ids_box, x, y, z)
                    ranged = r.ids[0] <= k <= r.ids[1]
                    if k == _lib.COMPONENT_NONE or ranged == bool(r.flags & _lib.RELABEL_IDS_EXCEPT):
                        continue
                if r.flags & _lib.RELABEL_DISTANCE:
                    dd = at(dmap, dmap_box, x, y, z)
                    if dd == _lib.DISTANCE_NONE or not r.d2[0] <= dd <= r.d2[1]:
                        continue
                changed += 1
                left[l] += 1
                arrived[to[l]] += 1
                hull = (x, y, z, x + 1, y + 1, z + 1) if hull is None else tuple(min(a, b) for a, b in zip(hull[:3], (x, y, z))) + tuple(
                    max(a, b) for a, b in zip(hull[3:], (x + 1, y + 1, z + 1)))
                if not r.flags & _lib.RELABEL_DRY_RUN:
                    new[i] = to[l]
    return new, changed, left, arrived, list(hull or (0,) * 6)


def test_the_twin_is_the_rule_texel_by_texel():
    from volym_amd import _lib, scene
    rng = np.random.default_rng(41)
    seen = set()
    total = 0
    for k in range(128):
        dims = tuple(int(v) for v in rng.integers(1 if k % 8 == 0 else 3, 9, 3))
        nx, ny, nz = dims
        n = nx * ny * nz
        vol, uncut = rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8)
        labels = rng.integers(0, 5, n).astype(np.uint8)
        snap_lo = tuple(int(rng.integers(0, max(d - 3, 1))) for d in dims)
        snap_box = (snap_lo, dims)
        shape = tuple(dims[a] - snap_lo[a] for a in (2, 1, 0))
        ids = rng.integers(0, 6, shape).astype(np.uint32)
        ids[rng.random(shape) < 0.3] = _lib.COMPONENT_NONE
        dmap = rng.integers(0, 30, shape).astype(np.uint32)
        dmap[rng.random(shape) < 0.2] = _lib.DISTANCE_NONE
        lo = tuple(int(rng.integers(snap_lo[a], min(snap_lo[a] + 2, dims[a]) + 1)) for a in range(3))
        hi = tuple(int(rng.integers(max(lo[a], dims[a] - 2), dims[a] + 1)) for a in range(3))
        flags = int(rng.integers(0, 32))
        if flags & 4 and not flags & 2:
            flags |= 2
        to = rng.integers(0, 7, 256)
        to[::3] = np.arange(256)[::3]                          # (every third label stays)
        a, b = int(rng.integers(0, 100)), int(rng.integers(150, 256))
        i0, i1 = int(rng.integers(0, 3)), int(rng.integers(2, 6))
        d0, d1 = int(rng.integers(0, 10)), int(rng.integers(12, 30))
        r = scene.Relabel((lo, hi), flags, (a, b) if k % 4 else (0, 255), to, (i0, i1), (d0, d1))
        new, res = scene.relabel_volume(vol, dims, r, labels, ids, snap_box, dmap, snap_box, uncut=uncut)
        w_new, w_changed, w_left, w_arrived, w_box = _by_the_rule(vol, uncut, dims, r, labels, ids, snap_box, dmap, snap_box)
        assert new.ravel().tolist() == w_new and int(res["changed"]) == w_changed, (k, r.box, flags)
        assert res["left"].tolist() == w_left and res["arrived"].tolist() == w_arrived and res["box"].tolist() == w_box, (k, r.box, flags)
        assert new.shape == (nz, ny, nx) and new.dtype == np.uint8
        seen.add(flags)
        total += w_changed
    assert len(seen) >= 16 and total > 300


def test_the_twin_refuses_a_box_outside_a_snapshot_and_a_missing_snapshot():
    from volym_amd import _lib, scene
    dims = (4, 4, 4)
    vol = labels = np.zeros(64, np.uint8)
    snap = np.zeros((2, 4, 4), np.uint32)
    r = scene.Relabel(dims=dims, flags=_lib.RELABEL_IDS, to={0: 1})
    with pytest.raises(ValueError):
        scene.relabel_volume(vol, dims, r, labels)
    with pytest.raises(ValueError):
        scene.relabel_volume(vol, dims, r, labels, ids=snap, ids_box=((0, 0, 1), (4, 4, 3)))
    new, res = scene.relabel_volume(vol, dims, r.replace(box=((0, 0, 1), (4, 4, 3))), labels, ids=snap, ids_box=((0, 0, 1), (4, 4, 3)))
    assert int(res["changed"]) == 32 and res["box"].tolist() == [0, 0, 1, 4, 4, 3] and int(new.sum()) == 32


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 2, 3, 5])
def test_growing_a_segment_by_r_counts_what_the_distance_histogram_says(r):
    """every texel is present (density >= 1) and every label may turn into S: count(S) afterwards is the texels with D <= r^2"""
    from volym_amd import scene
    host = RS.scene_a()
    S = 2
    d = scene.Distance(dims=host.dims, select=scene.surface_select([S]))
    summary, dmap = scene.distance_volume(host.vol, host.dims, d, labels=host.labels)
    grow = scene.Relabel(dims=host.dims, flags=8, to=np.full(256, S), d2=(0, r * r))
    new, res = scene.relabel_volume(host.vol, host.dims, grow, host.labels, dmap=dmap, dmap_box=d.box)
    assert int((new == S).sum()) == int(summary["hist"][:r + 1].sum())
    assert int(res["arrived"][S]) == int(summary["hist"][1:r + 1].sum()) == int(res["changed"])


def test_splitting_a_piece_off_leaves_one_piece_fewer_and_one_piece_of_the_new_label():
    from volym_amd import scene
    host = RS.scene_a()
    old, fresh = 3, 9
    c = scene.Components(dims=host.dims, min_byte=120, select=scene.surface_select([old]))
    summary, table, ids = scene.components_volume(host.vol, host.dims, c, labels=host.labels)
    n = int(summary["n_components"])
    assert n > 3
    for k in (0, n // 2, int(np.argmax(table["count"])), n - 1):
        split = scene.Relabel(dims=host.dims, flags=2, to={old: fresh}, ids=(k, k))
        new, res = scene.relabel_volume(host.vol, host.dims, split, host.labels, ids=ids, ids_box=c.box)
        assert int(res["changed"]) == int(table["count"][k]) == int(res["left"][old]) == int(res["arrived"][fresh])
        assert res["box"].tolist() == [int(v) for v in table["box"][k][:3]] + [int(v) + 1 for v in table["box"][k][3:]]
        after_old = scene.components_volume(host.vol, host.dims, c, labels=new.ravel())[0]
        after_new = scene.components_volume(host.vol, host.dims, c.replace(select=scene.surface_select([fresh])), labels=new.ravel())[0]
        assert int(after_old["n_components"]) == n - 1 and int(after_new["n_components"]) == 1


# ---- what the device tests rely on ----------------------------------------------------------------------------------------------
SCENES = {"a": (RS.scene_a, RS.cases_a), "b": (RS.scene_b, RS.cases_b), "ragged": (RS.scene_ragged, RS.cases_ragged)}


@pytest.mark.parametrize("which", list(SCENES))
def test_the_requests_change_what_the_device_tests_need_them_to(which):
    from volym_amd import _lib
    make, cases = SCENES[which]
    host = make()
    names = set()
    for case in cases():
        new, res, r = RS.expect(host, case)
        names.add(case.name)
        changed = int(res["changed"])
        assert int(res["left"].sum()) == int(res["arrived"].sum()) == changed, case.name
        dry = bool(r.flags & _lib.RELABEL_DRY_RUN)
        assert int((new != host.labels).sum()) == (0 if dry else changed), case.name
        if case.trivial:
            assert changed <= 1, case.name
        else:
            assert changed >= 50, (case.name, changed)
        if changed:
            (x0, y0, z0), (x1, y1, z1) = r.box
            b = res["box"].tolist()
            assert x0 <= b[0] < b[3] <= x1 and y0 <= b[1] < b[4] <= y1 and z0 <= b[2] < b[5] <= z1, case.name
        if case.wraps:
            assert RS.wrapping_chunks(host.dims, host.labels, new) > 0, case.name
    assert len(names) == len(cases())
    if which == "ragged":
        assert sum(1 for c in cases() if c.wraps) >= 4 and {bool(c.components) for c in cases() if c.wraps} == {False, True}
    if which == "a":
        flags = {c.relabel.flags & ~_lib.RELABEL_DRY_RUN for c in cases()}
        assert flags >= {0, 1, 2, 6, 8, 10, 14}
