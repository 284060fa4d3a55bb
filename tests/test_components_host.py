"""The components pass without a GPU: the C structs and constants, volym_components_check against scene.check_components, the host
twin scene.components_volume against a plain breadth-first flood fill (and against scipy.ndimage.label where scipy is installed), the
closed forms of the constructed scenes, the canonical numbering, the identities with the measure twin, truncated tables and
scene.components_summary.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import components_scenes as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

REQUEST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("select", 32, 256), ("max_components", 288, 4)]
SUMMARY_LAYOUT = [("n_components", 0, 8), ("n_solid", 8, 8), ("recorded", 16, 8), ("per_label", 24, 2048)]
RECORD_LAYOUT = [("x", 0, 2), ("y", 2, 2), ("z", 4, 2), ("label", 6, 1), ("flags", 7, 1), ("count", 8, 4), ("box", 12, 12)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Components) == 292 and C.sizeof(_lib.ComponentsSummary) == 2072 and C.sizeof(_lib.Component) == 24
    assert _lib.COMPONENTS_SUMMARY_DTYPE.itemsize == 2072 and _lib.COMPONENT_DTYPE.itemsize == 24
    for struct, dtype, layout in ((_lib.Components, None, REQUEST_LAYOUT), (_lib.ComponentsSummary, _lib.COMPONENTS_SUMMARY_DTYPE, SUMMARY_LAYOUT),
                                  (_lib.Component, _lib.COMPONENT_DTYPE, RECORD_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    consts = [_lib.COMPONENTS_UNCUT, _lib.COMPONENTS_SPLIT_LABELS, _lib.COMPONENTS_DEFAULT_MAX, _lib.COMPONENTS_TABLE_MAX, _lib.COMPONENTS_BOX_MAX,
              _lib.COMPONENT_NONE]
    assert consts == [1, 2, 65536, 1 << 24, 2 ** 31 - 2, 0xFFFFFFFF]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(volym_components), sizeof(struct volym_components_summary), sizeof(struct volym_component));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_components, %s));\n' % f for f, _, _ in REQUEST_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_components_summary, %s));\n' % f for f, _, _ in SUMMARY_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_component, %s));\n' % f for f, _, _ in RECORD_LAYOUT) +
                   '  printf(" %d %d %u %u %u %u %d", VOLYM_COMPONENTS_UNCUT, VOLYM_COMPONENTS_SPLIT_LABELS, VOLYM_COMPONENTS_DEFAULT_MAX,\n'
                   '         VOLYM_COMPONENTS_TABLE_MAX, VOLYM_COMPONENTS_BOX_MAX, VOLYM_COMPONENT_NONE, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [292, 2072, 24] + [o for _, o, _ in REQUEST_LAYOUT] + [o for _, o, _ in SUMMARY_LAYOUT] + [o for _, o, _ in RECORD_LAYOUT] + consts + [2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_components_pass", "volym_components_check", "volym_read_components", "volym_read_component_table", "volym_read_component_ids",
                 "volym_component_of", "volym_components_device_ptr", "volym_component_ids_device_ptr", "volym_component_table_device_ptr"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("components_pass", "read_components", "read_component_table", "read_component_ids", "component_of"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("components", "component_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Components", "check_components", "components_volume", "components_summary"):
        assert callable(getattr(scene, name))
    assert "import scipy" not in open(scene.__file__).read() and "from scipy" not in open(scene.__file__).read()


def _check_rows():
    """(name, request, dims, valid)"""
    from volym_amd import _lib, scene
    d = (9, 7, 5)
    F = scene.Components
    whole = ((0, 0, 0), d)
    big = (4096, 4096, 4096)
    rows = [("whole", F(whole), d, True), ("empty on x", F(((3, 0, 0), (3, 7, 5))), d, True), ("empty at the far corner", F((d, d)), d, True),
            ("one texel", F(((8, 6, 4), d)), d, True), ("uncut", F(whole, 1), d, True), ("split", F(whole, 2), d, True), ("both flags", F(whole, 3), d, True),
            ("flag 4", F(whole, 4), d, False), ("flag 2^31", F(whole, 1 << 31), d, False),
            ("min_byte 0", F(whole, 0, 0), d, False), ("min_byte 1", F(whole, 0, 1), d, True), ("min_byte 255", F(whole, 0, 255), d, True),
            ("min_byte 256", F(whole, 0, 256), d, False), ("min_byte 2^31", F(whole, 1, 1 << 31), d, False),
            ("nothing selected", F(whole, 0, 1, np.zeros(256)), d, True), ("select bytes of any value", F(whole, 0, 1, np.arange(256)), d, True),
            ("capacity 1", F(whole, max_components=1), d, True), ("capacity 2^24", F(whole, max_components=_lib.COMPONENTS_TABLE_MAX), d, True),
            ("capacity 2^24 + 1", F(whole, max_components=_lib.COMPONENTS_TABLE_MAX + 1), d, False),
            ("capacity 2^32 - 1", F(whole, max_components=2 ** 32 - 1), d, False),
            # the 2^31 - 2 texel limit: 1024^3 fits, 2^31 - 2 exactly (2 x 1073741823, and 2 x 3 x 357913941 = 2^31 - 2), one more does not
            ("1024 cubed", F(((0, 0, 0), (1024, 1024, 1024))), big, True),
            ("2^31 - 2 texels", F(((0, 0, 0), (2, 3, 357913941))), (2, 3, 357913941), True),
            ("2^31 texels", F(((0, 0, 0), (2048, 1024, 1024))), big, False),
            ("2^31 - 1 texels", F(((0, 0, 0), (1, 1, 2 ** 31 - 1))), (1, 1, 2 ** 31 - 1), False),
            ("2^31 + 2^20 texels in an offset box", F(((1, 1, 1), (2049, 1025, 1026))), big, False),
            ("4096 cubed", F(((0, 0, 0), big)), big, False),
            ("2^64 texels: wraps 64 bits to 0", F(((0, 0, 0), (2 ** 22, 2 ** 21, 2 ** 21))), (2 ** 22, 2 ** 21, 2 ** 21), False),
            ("an empty box whose width x height alone is beyond the limit", F(((0, 0, 0), (2 ** 31, 2, 0))), (2 ** 31, 2, 1), True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond axis %d" % a, F(((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 3; hi = list(d); hi[a] = 2
        rows.append(("lo above hi on axis %d" % a, F((tuple(lo), tuple(hi))), d, False))
    return rows


def test_check_agrees_with_python_on_every_row(volym_lib):
    from volym_amd import scene
    rows = _check_rows()
    assert sum(ok for *_, ok in rows) >= 12 and sum(not ok for *_, ok in rows) >= 16
    for name, c, dims, ok in rows:
        rc = volym_lib.volym_components_check(C.byref(c.to_c()), (C.c_uint32 * 3)(*dims))
        assert rc == (0 if ok else E_INVALID), name
        if ok:
            assert scene.check_components(c, dims) is c, name
        else:
            with pytest.raises(ValueError):
                scene.check_components(c, dims)
    ok = scene.Components(((0, 0, 0), (1, 1, 1))).to_c()
    assert volym_lib.volym_components_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_components_check(C.byref(ok), None) == E_INVALID
    with pytest.raises(ValueError):
        scene.Components(((0, 0, 0), (1, 1, 1)), 0, 1, np.full(256, 256)).to_c()
    with pytest.raises(ValueError):
        scene.Components(((0, 0, 0), (1, 1, 1)), max_components=2 ** 32).to_c()
    with pytest.raises(ValueError):
        scene.Components()                                        # neither a box nor dims


# ---- the twin against the rule ------------------------------------------------------------------------------------------------
def _solid(host_vol, host_labels, dims, c):
    """(solid, labels) over the request's box, [z, y, x]"""
    nx, ny, nz = dims
    lo, hi = c.box
    sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    b = np.asarray(host_vol).reshape(nz, ny, nx)[sub]
    l = np.asarray(host_labels).reshape(nz, ny, nx)[sub]
    return (b >= c.min_byte) & (np.asarray(c.select)[l] != 0), l


def _against_the_flood_fill(name, vol, labels, dims, c, result):
    """the twin's result against the breadth-first fill: ids, roots, counts, boxes, border flags, labels, the summary"""
    from volym_amd import _lib
    summary, table, ids = result
    solid, l = _solid(vol, labels, dims, c)
    if solid.size == 0:
        assert int(summary["n_components"]) == 0 and len(table) == 0 and ids.size == 0, name
        return 0
    fill, roots, counts = CS.flood_fill(solid, l if c.flags & CS.SPLIT else None)
    assert np.array_equal(ids, np.where(fill < 0, _lib.COMPONENT_NONE, fill).astype(np.uint32)), name
    n = len(roots)
    cap = c.max_components or _lib.COMPONENTS_DEFAULT_MAX
    assert (int(summary["n_components"]), int(summary["n_solid"]), int(summary["recorded"])) == (n, int(solid.sum()), min(n, cap)) and len(table) == min(n, cap), name
    lo = c.box[0]
    d, h, w = solid.shape
    # box and border flag of every component from its texels, one by one
    at = np.argwhere(fill >= 0)                                   # [z, y, x]
    of = fill[fill >= 0]
    mins, maxs = np.full((n, 3), 1 << 20, np.int64), np.full((n, 3), -1, np.int64)
    np.minimum.at(mins, of, at)
    np.maximum.at(maxs, of, at)
    on_face = np.zeros(n, np.int64)
    np.maximum.at(on_face, of, ((at == 0) | (at == np.array([d - 1, h - 1, w - 1]))).any(axis=1).astype(np.int64))
    per_label = np.zeros(256, np.int64)
    for k, (x, y, z) in enumerate(roots):
        per_label[l[z, y, x]] += 1
        if k >= len(table):
            continue
        r = table[k]
        assert (int(r["x"]), int(r["y"]), int(r["z"]), int(r["label"]), int(r["count"])) == (x + lo[0], y + lo[1], z + lo[2], int(l[z, y, x]), counts[k]), (name, k)
        want_box = [int(mins[k, 2]) + lo[0], int(mins[k, 1]) + lo[1], int(mins[k, 0]) + lo[2], int(maxs[k, 2]) + lo[0], int(maxs[k, 1]) + lo[1], int(maxs[k, 0]) + lo[2]]
        assert r["box"].tolist() == want_box, (name, k)
        assert int(r["flags"]) == int(on_face[k]), (name, k)
    assert summary["per_label"].tolist() == per_label.tolist(), name
    return n


@pytest.mark.parametrize("which", ["a", "b"])
def test_the_twin_is_the_flood_fill_on_the_random_scenes(which):
    host = CS.scene_a() if which == "a" else CS.scene_b()
    found = 0
    for flags in (0, CS.SPLIT):
        for name, c in CS.requests(flags):
            found += _against_the_flood_fill((flags, name), host.vol, host.labels, host.dims, c, CS.expect(host, c))
    assert found > 500
    # without labels every label is 0 and SPLIT_LABELS changes nothing
    for name, c in CS.requests(CS.SPLIT)[:4]:
        assert CS.as_bytes(CS.expect(host, c, labels=False)) == CS.as_bytes(CS.expect(host, c.replace(flags=0), labels=False)), name
        _against_the_flood_fill(("no labels", name), host.vol, np.zeros_like(host.labels), host.dims, c.replace(flags=0), CS.expect(host, c, labels=False))


def test_the_twin_is_the_flood_fill_on_the_long_rows():
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    dims, vol, labels = _ragged()
    for name in ("65", "66 from 1"):
        for min_byte, flags in ((4, 0), (1, CS.SPLIT)):
            c = scene.Components(CS.LONG_BOXES[name], flags, min_byte)
            _against_the_flood_fill((name, min_byte), vol, labels, dims, c, scene.components_volume(vol, dims, c, labels=labels))


def test_the_twins_partition_is_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    from volym_amd import _lib, scene
    host = CS.scene_a()
    for name, c in CS.requests():
        summary, table, ids = CS.expect(host, c)
        solid, _ = _solid(host.vol, host.labels, host.dims, c)
        if solid.size == 0:
            continue
        theirs, n = ndimage.label(solid, structure=ndimage.generate_binary_structure(3, 1))
        assert n == int(summary["n_components"]), name
        # the same partition: the map between the two numberings is one to one
        pairs = np.unique(np.stack([ids[solid].astype(np.int64), theirs[solid].astype(np.int64)], axis=1), axis=0)
        assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n, name
        assert ((ids == _lib.COMPONENT_NONE) == (theirs == 0)).all(), name


def test_the_closed_forms_of_the_constructed_scenes():
    from volym_amd import scene
    for name, (dims, vol, lab, c, closed) in CS.constructed().items():
        summary, table, ids = scene.components_volume(vol, dims, c, labels=lab)
        assert (int(summary["n_components"]), int(summary["n_solid"])) == (closed["n_components"], closed["n_solid"]), name
        assert table["count"].tolist() == closed["counts"], name
        if "open" in closed:
            assert table["flags"].tolist() == closed["open"], name
    dims, vol, lab, c, closed = CS.constructed()["serpentine"]
    summary, table, ids = scene.components_volume(vol, dims, c, labels=lab)
    assert closed["n_solid"] > 1300 and (int(table["x"][0]), int(table["y"][0]), int(table["z"][0])) == (0, 0, 0)
    assert table["box"][0].tolist() == [0, 0, 0, 65, 8, 6]
    _against_the_flood_fill("serpentine", vol, lab, dims, c, (summary, table, ids))
    dims, vol, lab, c, closed = CS.constructed()["checkerboard"]
    summary, table, ids = scene.components_volume(vol, dims, c, labels=lab)
    assert int(summary["n_components"]) == int(summary["n_solid"]) > 200


# ---- the numbering, the sums, the capacity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
def test_roots_ascend_and_record_k_has_id_k_and_counts_sum_to_n_solid(which):
    host = CS.scene_a() if which == "a" else CS.scene_b()
    for flags in (0, CS.SPLIT):
        for name, c in CS.requests(flags):
            summary, table, ids = CS.expect(host, c)
            assert int(summary["recorded"]) == int(summary["n_components"]) == len(table), name        # untruncated
            key = (table["z"].astype(np.int64) * 4096 + table["y"]) * 4096 + table["x"]
            assert (np.diff(key) > 0).all(), name
            lo = c.box[0]
            assert ids[table["z"] - lo[2], table["y"] - lo[1], table["x"] - lo[0]].tolist() == list(range(len(table))), name
            assert int(table["count"].astype(np.int64).sum()) == int(summary["n_solid"]), name
            assert int(summary["per_label"].sum()) == len(table) and np.array_equal(np.bincount(table["label"], minlength=256), summary["per_label"]), name


def test_one_label_alone_has_the_measure_twins_count_under_every_cut():
    from volym_amd import scene
    host = CS.scene_a()
    for step, box, plane, hidden in CS.CUTS:
        host.set_cut(_NoContext(), box, plane, hidden)
        now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
        rec, _ = scene.measure_volume(now, host.dims, scene.Measure(dims=host.dims), labels=host.labels, cut=host.cut, uncut=host.vol)
        for l in range(5):
            c = scene.Components(dims=host.dims, select=scene.surface_select([l]))
            summary, table, _ = CS.expect(host, c)
            assert int(summary["n_solid"]) == int(rec["count"][l]), (step, l)
            assert int(summary["per_label"][l]) == int(summary["n_components"]), (step, l)


class _NoContext:
    """Host.set_cut's context when there is none"""

    def set_crop_box(self, *a):
        pass

    set_clip_plane = set_segment_visibility = set_crop_box


def test_a_truncated_table_is_a_prefix_of_the_whole_one():
    from volym_amd import scene
    host = CS.scene_a()
    c = scene.Components(CS.BOXES["whole"], 0, 200)
    full = CS.expect(host, c)
    n = int(full[0]["n_components"])
    assert n > 1000
    for cap in (1, 7, n - 1, n, n + 1):
        summary, table, ids = CS.expect(host, c.replace(max_components=cap))
        assert int(summary["recorded"]) == min(cap, n) == len(table) and int(summary["n_components"]) == n
        assert table.tobytes() == full[1][:cap].tobytes() and np.array_equal(ids, full[2])
        assert summary["per_label"].tolist() == full[0]["per_label"].tolist()


def test_components_summary():
    from volym_amd import scene
    host = CS.scene_a()
    c = scene.Components(CS.BOXES["whole"], CS.SPLIT, 128)
    summary, table, ids = CS.expect(host, c)
    spacing = (0.5, 0.25, 2.0)
    got = scene.components_summary(summary, table, spacing, below=4)
    assert list(got) == sorted(got) == [0, 1, 2, 3, 4]
    for l, one in got.items():
        mine = table[table["label"] == l]
        assert one["pieces"] == one["recorded"] == len(mine) == int(summary["per_label"][l])
        k = int(np.flatnonzero(table["label"] == l)[np.argmax(mine["count"])])
        assert one["largest"] == scene.component_dict(table[k], k, spacing) and one["largest"]["count"] == int(mine["count"].max())
        assert one["largest"]["volume"] == one["largest"]["count"] * 0.25
        assert one["share"] == int(mine["count"].max()) / int(summary["n_solid"])
        small = mine["count"] < 4
        assert one["small"]["pieces"] == int(small.sum()) > 0 and one["small"]["texels"] == int(mine["count"][small].sum())
        assert [int(table["count"][i]) < 4 and int(table["label"][i]) == l for i in one["small"]["numbers"]] == [True] * int(small.sum())
    # a truncated table: the pieces are the summary's, the rest what the table holds
    cut = scene.components_summary(*CS.expect(host, c.replace(max_components=3))[:2])
    assert sum(v["recorded"] for v in cut.values()) == 3 and {l: v["pieces"] for l, v in cut.items()} == {l: v["pieces"] for l, v in got.items()}
    assert scene.components_summary(*scene.empty_components()[:2]) == {}


def test_the_clis_refuse_a_bad_threshold(volym_lib):
    from volym_amd import __main__ as cli
    assert cli._surface_arg("Canopy,3:40", "--components") == (["Canopy", 3], 40)
    with pytest.raises(SystemExit) as e:
        cli._surface_arg("Canopy:x", "--components")
    assert "--components" in str(e.value)
    r = subprocess.run([os.path.join(ROOT, "volym_amd", "volym"), "run", "simple", "--components", "Canopy:300"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--components" in r.stderr


def test_the_scan_scene_has_two_block_sums_per_thread_and_every_piece_recorded():
    """what tests/test_gpu_components.py test_the_offset_scan_with_two_block_sums_per_thread relies on"""
    from tests import surface_scenes as S
    from volym_amd import _lib
    c, (summary, table, ids) = CS.scan_components(True)
    assert S.rows(c.box) == 65792 > 256 * _lib.SURFACE_SCAN_ROWS
    assert int(summary["n_components"]) == int(summary["recorded"]) == len(table) > 10000
    assert int(ids[ids != _lib.COMPONENT_NONE].max()) == len(table) - 1
    # without the split and with every label selected pieces merge: another result, so one left over from the first pass would show
    whole, (summary2, table2, _) = CS.scan_components(False)
    assert whole.box == c.box and whole.flags == 0 and np.asarray(whole.select).all()
    assert 1 < int(summary2["n_components"]) == int(summary2["recorded"]) == len(table2) < len(table)
