"""The surface passes without a GPU: the C structs and constants, volym_surface_check against scene.check_surface, the host twin
scene.surface_volume against a plain triple loop, closed forms, the canonical order, the divergence identity against the measure
twin, the mesh and its files, and the conditions on the scenes that tests/test_gpu_surface.py relies on (asserted here on the twin,
where they cost nothing).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import measure_scenes as M
from tests import surface_scenes as S
from tests.test_measure_host import NoContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

SURFACE_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("select", 32, 256)]
SUMMARY_LAYOUT = [("faces", 0, 12288), ("total", 12288, 8), ("pos", 12296, 6144), ("neg", 18440, 6144)]
FACE_LAYOUT = [("x", 0, 2), ("y", 2, 2), ("z", 4, 2), ("dir", 6, 1), ("label", 7, 1)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Surface) == 288 and C.sizeof(_lib.SurfaceSummary) == 24584 and C.sizeof(_lib.SurfaceFace) == 8
    assert _lib.SURFACE_SUMMARY_DTYPE.itemsize == 24584 and _lib.SURFACE_FACE_DTYPE.itemsize == 8
    for struct, dtype, layout in ((_lib.Surface, None, SURFACE_LAYOUT), (_lib.SurfaceSummary, _lib.SURFACE_SUMMARY_DTYPE, SUMMARY_LAYOUT),
                                  (_lib.SurfaceFace, _lib.SURFACE_FACE_DTYPE, FACE_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    assert (_lib.SURFACE_UNCUT, _lib.SURFACE_SCAN_ROWS) == (1, 256)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(volym_surface), sizeof(struct volym_surface_summary), sizeof(struct volym_surface_face));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_surface, %s));\n' % f for f, _, _ in SURFACE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_surface_summary, %s));\n' % f for f, _, _ in SUMMARY_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_surface_face, %s));\n' % f for f, _, _ in FACE_LAYOUT) +
                   '  printf(" %d %d %d", VOLYM_SURFACE_UNCUT, VOLYM_SURFACE_SCAN_ROWS, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [288, 24584, 8] + [o for _, o, _ in SURFACE_LAYOUT] + [o for _, o, _ in SUMMARY_LAYOUT] + [o for _, o, _ in FACE_LAYOUT] + [1, 256, 2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, mesh, scene
    for name in ("volym_surface_pass", "volym_read_surface", "volym_surface_device_ptr", "volym_surface_faces_pass", "volym_read_surface_faces",
                 "volym_surface_check"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("surface_pass", "read_surface", "surface_device_ptr", "surface_faces_pass", "read_surface_faces"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("surface", "surface_at", "export_surface"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Surface", "check_surface", "surface_volume", "surface_summary", "surface_mesh", "surface_select"):
        assert callable(getattr(scene, name))
    for name in ("write_stl", "read_stl", "write_obj", "read_obj", "write"):
        assert callable(getattr(mesh, name))


def _check_rows():
    """(name, surface, dims, valid)"""
    from volym_amd import scene
    d = (9, 7, 5)
    F = scene.Surface
    whole = ((0, 0, 0), d)
    rows = [("whole", F(whole), d, True), ("empty on x", F(((3, 0, 0), (3, 7, 5))), d, True), ("empty at the far corner", F((d, d)), d, True),
            ("one texel", F(((8, 6, 4), d)), d, True), ("uncut", F(whole, 1), d, True), ("flag 2", F(whole, 2), d, False),
            ("flag 3", F(whole, 3), d, False), ("flag 2^31", F(whole, 1 << 31), d, False),
            ("min_byte 0", F(whole, 0, 0), d, False), ("min_byte 1", F(whole, 0, 1), d, True), ("min_byte 255", F(whole, 0, 255), d, True),
            ("min_byte 256", F(whole, 0, 256), d, False), ("min_byte 2^31", F(whole, 1, 1 << 31), d, False),
            ("nothing selected", F(whole, 0, 1, np.zeros(256)), d, True), ("select bytes of any value", F(whole, 0, 1, np.arange(256)), d, True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond axis %d" % a, F(((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 3; hi = list(d); hi[a] = 2
        rows.append(("lo above hi on axis %d" % a, F((tuple(lo), tuple(hi))), d, False))
    rows.append(("4096 cubed", F(((0, 0, 0), (4096, 4096, 4096))), (4096, 4096, 4096), True))
    return rows


def test_check_agrees_with_python_on_every_row(volym_lib):
    from volym_amd import scene
    rows = _check_rows()
    assert sum(ok for *_, ok in rows) >= 9 and sum(not ok for *_, ok in rows) >= 12
    for name, s, dims, ok in rows:
        rc = volym_lib.volym_surface_check(C.byref(s.to_c()), (C.c_uint32 * 3)(*dims))
        assert rc == (0 if ok else E_INVALID), name
        if ok:
            assert scene.check_surface(s, dims) is s, name
        else:
            with pytest.raises(ValueError):
                scene.check_surface(s, dims)
    ok = scene.Surface(((0, 0, 0), (1, 1, 1))).to_c()
    assert volym_lib.volym_surface_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_surface_check(C.byref(ok), None) == E_INVALID
    with pytest.raises(ValueError):
        scene.Surface(((0, 0, 0), (1, 1, 1)), 0, 1, np.full(256, 256)).to_c()
    with pytest.raises(ValueError):
        scene.Surface(((0, 0, 0), (1, 1, 1)), 0, 1, np.zeros(255)).to_c()
    with pytest.raises(ValueError):
        scene.Surface()                                           # neither a box nor dims


# ---- the twin against the rule ------------------------------------------------------------------------------------------------
def _loop(vol, dims, s, labels, uncut):
    """the rule of include/volym_hip.h as a plain triple loop over Python integers: (faces, total, pos, neg, records)"""
    nx, ny, nz = dims
    src = uncut if (s.flags & 1 and uncut is not None) else vol
    (x0, y0, z0), (x1, y1, z1) = s.box

    def solid(x, y, z):
        if not (x0 <= x < x1 and y0 <= y < y1 and z0 <= z < z1):
            return False
        at = (z * ny + y) * nx + x
        return int(src[at]) >= s.min_byte and int(s.select[int(labels[at]) if labels is not None else 0]) != 0

    faces = [[0] * 6 for _ in range(256)]
    pos, neg = [[0] * 3 for _ in range(256)], [[0] * 3 for _ in range(256)]
    records = []
    step = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                if not solid(x, y, z):
                    continue
                l = int(labels[(z * ny + y) * nx + x]) if labels is not None else 0
                for d, (dx, dy, dz) in enumerate(step):
                    if solid(x + dx, y + dy, z + dz):
                        continue
                    faces[l][d] += 1
                    records.append((x, y, z, d, l))
                    if d & 1:
                        pos[l][d >> 1] += (x, y, z)[d >> 1] + 1
                    else:
                        neg[l][d >> 1] += (x, y, z)[d >> 1]
    return faces, len(records), pos, neg, records


def _equal_to_loop(got, want):
    summary, records = got
    faces, total, pos, neg, recs = want
    assert summary["faces"].tolist() == faces and int(summary["total"]) == total
    assert summary["pos"].tolist() == pos and summary["neg"].tolist() == neg
    assert [tuple(int(v) for v in r) for r in records.tolist()] == recs


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
    select = np.zeros(256, np.int64)
    select[[0, 1, 2, 4, 5, 7, 9, 11]] = [1, 1, 9, 255, 1, 1, 1, 1]
    seen = set()
    for box in (((0, 0, 0), dims), ((2, 1, 0), (7, 7, 4)), ((4, 3, 2), (5, 4, 3)), ((3, 3, 3), (3, 7, 5))):
        for min_byte in (1, 100):
            s = scene.Surface(box, flags, min_byte, select)
            got = scene.surface_volume(now, dims, s, labels=labels, cut=cut, uncut=uncut)
            _equal_to_loop(got, _loop(now, dims, s, labels, uncut))
            seen.add(S.as_bytes(got))
            # without an uncut copy UNCUT reads the bytes as they stand
            _equal_to_loop(scene.surface_volume(now, dims, s, labels=labels, cut=cut), _loop(now, dims, s, labels, None))
    assert len(seen) >= 5                                         # (the empty box, and perhaps the one texel, give one result for both thresholds)


def test_twin_equals_the_rule_on_scene_a():
    from volym_amd import scene
    a = S.scene_a()
    a.set_cut(NoContext(), S.BOX, S.PLANE, S.HIDDEN)
    now = scene.cut_volume(a.vol, a.dims, a.cut, a.labels)
    for s in (scene.Surface(S.BOXES["whole"], 0, 128, S.selects()["mix"]), scene.Surface(S.BOXES["x 5..30"], 1, 200, S.selects()["all"])):
        _equal_to_loop(scene.surface_volume(now, a.dims, s, labels=a.labels, uncut=a.vol), _loop(now, a.dims, s, a.labels, a.vol))


# ---- closed forms -------------------------------------------------------------------------------------------------------------
def _block(dims, lo, hi, byte=200):
    v = np.zeros(dims[::-1], np.uint8)
    v[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = byte
    return v.ravel()


def test_one_texel_two_texels_and_a_block():
    from volym_amd import scene
    dims = (8, 7, 6)
    whole = scene.Surface(dims=dims)
    summary, faces = scene.surface_volume(_block(dims, (4, 2, 3), (5, 3, 4)), dims, whole)
    assert int(summary["total"]) == 6 and summary["faces"][0].tolist() == [1] * 6
    assert [tuple(r) for r in faces.tolist()] == [(4, 2, 3, d, 0) for d in range(6)]
    assert summary["pos"][0].tolist() == [5, 3, 4] and summary["neg"][0].tolist() == [4, 2, 3]
    for a in range(3):                                            # two adjacent texels, along every axis
        hi = [5, 3, 4]; hi[a] += 1
        summary, faces = scene.surface_volume(_block(dims, (4, 2, 3), hi), dims, whole)
        assert int(summary["total"]) == 10 and len(faces) == 10
        assert summary["faces"][0].tolist() == [1 if d >> 1 == a else 2 for d in range(6)]
    for lo, hi in (((1, 1, 1), (7, 4, 3)), ((0, 0, 0), dims), ((2, 3, 1), (3, 7, 6))):       # inside, filling the volume, a column
        a, b, c = (h - l for l, h in zip(lo, hi))
        summary, faces = scene.surface_volume(_block(dims, lo, hi), dims, whole)
        assert int(summary["total"]) == 2 * (a * b + b * c + c * a) == len(faces)
        assert summary["faces"][0].tolist() == [b * c, b * c, a * c, a * c, a * b, a * b]
        assert (summary["pos"][0].astype(np.int64) - summary["neg"][0].astype(np.int64)).tolist() == [a * b * c] * 3
        assert int(summary["faces"][1:].sum()) == 0


def test_a_checkerboard_has_six_faces_per_solid_texel():
    from volym_amd import scene
    dims = (7, 6, 5)
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    board = np.where((x + y + z) % 2 == 0, 77, 0).astype(np.uint8).ravel()
    summary, faces = scene.surface_volume(board, dims, scene.Surface(dims=dims, min_byte=77))
    solid = int((board > 0).sum())
    assert int(summary["total"]) == 6 * solid == len(faces) and summary["faces"][0].tolist() == [solid] * 6
    assert int(scene.surface_volume(board, dims, scene.Surface(dims=dims, min_byte=78))[0]["total"]) == 0


def test_a_block_cut_by_the_requests_box_closes_along_the_box():
    from volym_amd import scene
    dims = (10, 9, 8)
    vol = _block(dims, (1, 1, 1), (9, 8, 7))                      # 8 x 7 x 6
    summary, faces = scene.surface_volume(vol, dims, scene.Surface(((4, 0, 0), (10, 9, 5))))       # keeps 5 x 7 x 4 of it
    a, b, c = 5, 7, 4
    assert int(summary["total"]) == 2 * (a * b + b * c + c * a)
    assert summary["faces"][0].tolist() == [b * c, b * c, a * c, a * c, a * b, a * b]
    assert (summary["pos"][0].astype(np.int64) - summary["neg"][0].astype(np.int64)).tolist() == [a * b * c] * 3
    assert faces["x"].min() == 4 and faces["z"].max() == 4        # the closing faces sit on texels inside the box
    # the same by bytes: a texel of a selected label whose own byte is below min_byte is not solid
    labels = np.full(vol.size, 3, np.uint8)
    dim = vol.copy().reshape(dims[::-1])
    dim[:, :, :4] //= 2
    s = scene.Surface(dims=dims, min_byte=150, select=scene.surface_select([3]))
    got = scene.surface_volume(dim.ravel(), dims, s, labels=labels)
    assert got[0]["faces"][3].tolist() == [7 * 6, 7 * 6, 5 * 6, 5 * 6, 5 * 7, 5 * 7]


# ---- the order, the identity --------------------------------------------------------------------------------------------------
def test_the_records_come_in_strictly_ascending_z_y_x_dir():
    for host in (S.scene_a(), S.scene_b()):
        host.set_cut(NoContext(), S.BOX, S.PLANE, S.HIDDEN)
        seen = 0
        for name, s in S.surfaces():
            summary, faces = S.expect(host, s)
            keys = S.face_keys(faces)
            assert (np.diff(keys) > 0).all(), name
            assert len(faces) == int(summary["total"]) == int(summary["faces"].sum()), name
            seen += len(faces)
        assert seen > 20000


def test_the_divergence_sums_give_the_measured_count_under_every_cut():
    """pos - neg on every axis == the number of solid texels: per label with that label selected alone (its own surface is closed;
    selected together, two solid texels of different labels have no face between them and only the sum over the labels closes).
    With min_byte 1 on Scene A (bytes 1..255) that number is the measure twin's count, under every cut state."""
    from volym_amd import scene
    enclosed = lambda summary: summary["pos"].astype(np.int64) - summary["neg"].astype(np.int64)
    for host, alone in ((S.scene_a(), range(5)), (S.scene_b(), (0, 77, 255))):
        for step, box, plane, hidden in S.CUTS:
            host.set_cut(NoContext(), box, plane, hidden)
            for b, rbox in S.BOXES.items():
                rec, _ = M.expect(host, scene.Measure(rbox))
                together = enclosed(S.expect(host, scene.Surface(rbox, 0, 1))[0])
                assert together.sum(axis=0).tolist() == [int(rec["count"].sum())] * 3, (step, b)
                for l in alone:
                    e = enclosed(S.expect(host, scene.Surface(rbox, 0, 1, scene.surface_select([l])))[0])
                    assert e[l].tolist() == [int(rec["count"][l])] * 3, (step, b, l)
                    assert not np.delete(e, l, axis=0).any(), (step, b, l)
        # at a threshold: the solid texels themselves
        lab = host.labels.astype(np.int64)
        now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
        mix = S.selects()["mix"]
        assert enclosed(S.expect(host, scene.Surface(dims=S.DIMS, min_byte=128, select=mix))[0]).sum(axis=0).tolist() == \
            [int(((now >= 128) & (mix[lab] != 0)).sum())] * 3
        e = enclosed(S.expect(host, scene.Surface(dims=S.DIMS, min_byte=128, select=S.selects()["one"]))[0])
        assert e[3].tolist() == [int(((now >= 128) & (lab == 3)).sum())] * 3 and e[3][0] > 0
    # Scene A's blocks of labels touch: selected together, the sums of one label alone do not close
    a = S.scene_a()
    e = enclosed(S.expect(a, scene.Surface(dims=S.DIMS))[0])
    assert any(len(set(e[l].tolist())) > 1 or e[l][0] != int((a.labels == l).sum()) for l in range(5))


def test_surface_summary_in_physical_units():
    from volym_amd import scene
    dims = (10, 9, 8)
    summary, _ = scene.surface_volume(_block(dims, (1, 1, 1), (9, 8, 7)), dims, scene.Surface(dims=dims))
    s = scene.surface_summary(summary, 0, (0.5, 0.25, 2.0))
    assert s["faces"] == [42, 42, 48, 48, 56, 56] and s["pairs"] == [84, 96, 112] and s["enclosed"] == 8 * 7 * 6
    assert s["area"] == 84 * 0.25 * 2.0 + 96 * 0.5 * 2.0 + 112 * 0.5 * 0.25 and s["volume"] == 336 * 0.25
    assert abs(s["sphericity"] - np.pi ** (1 / 3) * (6 * s["volume"]) ** (2 / 3) / s["area"]) < 1e-12
    cube, _ = scene.surface_volume(_block(dims, (1, 1, 1), (7, 7, 7)), dims, scene.Surface(dims=dims))
    assert abs(scene.surface_summary(cube, 0)["sphericity"] - (np.pi / 6) ** (1 / 3)) < 1e-12
    assert scene.surface_summary(summary, 5) is None
    with_count = scene.surface_summary(summary, 0, (1, 1, 1), {"count": 400})
    assert with_count["measured"] == 400 and with_count["sphericity"] > scene.surface_summary(summary, 0)["sphericity"]
    # all labels together; and one label of several that touch: its own sums need not close
    a = S.scene_a()
    both, _ = S.expect(a, scene.Surface(dims=S.DIMS))
    union = scene.surface_summary(both)
    assert union["label"] is None and union["enclosed"] == S.NX * S.NY * S.NZ and union["pairs"] == [2 * S.NY * S.NZ, 2 * S.NX * S.NZ, 2 * S.NX * S.NY]
    parts = [scene.surface_summary(both, l) for l in range(5)]
    assert sum(p["area"] for p in parts) == union["area"] and any(p["enclosed"] is None and p["sphericity"] is None for p in parts)


# ---- the mesh and its files ---------------------------------------------------------------------------------------------------
def _edges(quads):
    """(directed edges as pairs, one row per edge use)"""
    return np.stack([quads, np.roll(quads, -1, axis=1)], axis=2).reshape(-1, 2)


def test_the_mesh_is_watertight_and_wound_outwards():
    from volym_amd import scene
    dims = (10, 9, 8)
    _, faces = scene.surface_volume(_block(dims, (1, 1, 1), (9, 8, 7)), dims, scene.Surface(dims=dims))
    vertices, quads = scene.surface_mesh(faces, (0.5, 0.25, 2.0), (1.0, 2.0, 3.0))
    assert quads.shape == (len(faces), 4) and len(vertices) == 2 + len(faces)      # a quad sphere: V - E + F = 2 with E = 2 F
    e = _edges(quads)
    directed = e[:, 0] * len(vertices) + e[:, 1]
    assert len(np.unique(directed)) == len(directed)              # no edge is used twice in the same direction ...
    undirected = np.sort(e, axis=1)
    _, uses = np.unique(undirected[:, 0] * len(vertices) + undirected[:, 1], return_counts=True)
    assert (uses == 2).all()                                      # ... and every edge by exactly two faces of this 6-connected solid
    # outward: the quad's normal is the face's direction, and the signed volume is the block's
    p = vertices[quads]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    unit = scene.SURFACE_FACE_NORMALS[faces["dir"]]
    assert (np.sign(normal) == unit).all()
    volume = (np.cross(p[:, 0], p[:, 1]) * p[:, 2]).sum() / 6 + (np.cross(p[:, 0], p[:, 2]) * p[:, 3]).sum() / 6
    assert abs(volume - 8 * 7 * 6 * 0.25) < 1e-9
    # any solid, touching at edges and corners too: every edge is used an even number of times
    host = S.scene_a()
    _, faces = S.expect(host, scene.Surface(S.BOXES["whole"], 0, 128, S.selects()["mix"]))
    vertices, quads = scene.surface_mesh(faces)
    undirected = np.sort(_edges(quads), axis=1)
    _, uses = np.unique(undirected[:, 0] * len(vertices) + undirected[:, 1], return_counts=True)
    assert len(faces) > 5000 and (uses % 2 == 0).all() and (uses == 4).any()
    assert np.array_equal(vertices, np.unique(vertices, axis=0)[np.lexsort(np.unique(vertices, axis=0).T)])      # deduplicated, sorted z, y, x


def test_stl_and_obj_read_back(tmp_path):
    from volym_amd import mesh, scene
    host = S.scene_a()
    _, faces = S.expect(host, scene.Surface(S.BOXES["x 5..30"], 0, 200, S.selects()["all"]))
    spacing, origin = (0.5, 0.25, 2.0), (-3.0, 0.125, 7.0)
    vertices, quads = scene.surface_mesh(faces, spacing, origin)
    stl = str(tmp_path / "a.stl")
    assert mesh.write(stl, faces, spacing, origin) == 2 * len(faces)
    assert os.path.getsize(stl) == 84 + 100 * len(faces)
    normals, tri = mesh.read_stl(stl)
    assert np.array_equal(normals, np.repeat(scene.SURFACE_FACE_NORMALS[faces["dir"]], 2, axis=0))
    assert np.array_equal(tri[0::2], vertices[quads[:, [0, 1, 2]]].astype(np.float32))
    assert np.array_equal(tri[1::2], vertices[quads[:, [0, 2, 3]]].astype(np.float32))
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.sign(n) == normals).all()
    obj = str(tmp_path / "a.obj")
    mesh.write(obj, faces, spacing, origin)
    v, q = mesh.read_obj(obj)
    assert np.array_equal(v, vertices) and np.array_equal(q, quads)
    none = faces[:0]
    assert mesh.write_stl(str(tmp_path / "none.stl"), none) == 0 and os.path.getsize(str(tmp_path / "none.stl")) == 84
    with pytest.raises(ValueError):
        mesh.write(str(tmp_path / "a.ply"), faces)


# ---- the conditions the device tests rely on ----------------------------------------------------------------------------------
def test_the_scenes_of_the_device_tests_are_what_those_tests_need():
    from volym_amd import _lib, scene
    a, b = S.scene_a(), S.scene_b()
    assert a.dims == S.DIMS == (37, 22, 19) and S.NX % 16 and a.vol.min() >= 1
    # faces in every one of the six directions at min_byte 128, for several labels
    summary, faces = S.expect(a, scene.Surface(dims=S.DIMS, min_byte=128))
    assert (summary["faces"][:5] > 0).all() and int(summary["faces"][5:].sum()) == 0
    assert (np.bincount(faces["dir"], minlength=6) > 100).all()
    summary, _ = S.expect(b, scene.Surface(dims=S.DIMS, min_byte=128))
    assert (summary["faces"].sum(axis=1) > 0).sum() >= 250
    # the "x 5..30" box has rows that share a 16-byte chunk of the linear layout, and rows that start and end inside one
    assert M.shared_chunks(S.BOXES["x 5..30"]) >= 1
    # more rows than one workgroup of the scan covers, in a box whose row count is no multiple of it; and boxes of one row and none
    assert S.rows(S.BOXES["whole"]) == 418 > _lib.SURFACE_SCAN_ROWS and S.rows(S.BOXES["whole"]) % _lib.SURFACE_SCAN_ROWS
    assert S.rows(S.BOXES["x 5..30"]) == 272 > _lib.SURFACE_SCAN_ROWS
    assert S.rows(S.BOXES["texel"]) == 1 and S.rows(S.BOXES["empty"]) == 0 and S.rows(S.BOXES["256 rows"]) == _lib.SURFACE_SCAN_ROWS
    # select tables: none selects nothing, one a label both scenes have, the mix several with bytes other than 1
    sel = S.selects()
    assert not sel["none"].any() and sel["all"].all() and sel["one"].sum() == 1 and set(sel["mix"]) >= {0, 1, 7, 255}
    assert int(S.expect(a, scene.Surface(dims=S.DIMS, select=sel["none"]))[0]["total"]) == 0
    # every cut changes the surface, and lifting it brings the first one back
    results = []
    for name, box, plane, hidden in S.CUTS:
        a.set_cut(NoContext(), box, plane, hidden)
        results.append(S.as_bytes(S.expect(a, scene.Surface(dims=S.DIMS, min_byte=128))))
    assert len(set(results)) == 5 and all(r == results[0] for r in results[2::2])
    # no two requests of the short list give the same result, so a result that carried over from another pass would show
    a.set_cut(NoContext(), S.BOX, S.PLANE, S.HIDDEN)
    results = [S.as_bytes(r) for r in (S.expect(a, s) for _, s in S.surfaces()) if int(r[0]["total"])]
    assert len(set(results)) == len(results) >= 8
    assert len(S.every_surface()) == 7 * 4 * 3
    # rows longer than a wave: solid runs that cross the chunk borders at x0 + 64, in every box of the list
    from tests.test_gpu_crop_box import _ragged
    dims, vol, labels = _ragged()
    assert dims == S.LONG_DIMS and sorted(hi[0] - lo[0] for lo, hi in S.LONG_BOXES.values()) == [64, 65, 66, 94, 97]
    for name, (lo, hi) in S.LONG_BOXES.items():
        solid = (vol >= 4).reshape(dims[::-1])[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
        if hi[0] - lo[0] > 64:
            assert int((solid[:, :, 63] & solid[:, :, 64]).sum()) > 100, name        # the run goes on in the next chunk: no face there
            assert int((solid[:, :, 63] != solid[:, :, 64]).sum()) > 100, name       # it ends at the border: a face from the carried bit
        summary, faces = scene.surface_volume(vol, dims, scene.Surface((lo, hi), 0, 4), labels=labels)
        assert (summary["faces"].sum(axis=1) > 0).sum() >= 2 and (np.diff(S.face_keys(faces)) > 0).all(), name


def test_the_scan_scene_has_two_block_sums_per_thread_and_uneven_rows():
    """what tests/test_gpu_surface.py test_the_offset_scan_with_two_block_sums_per_thread relies on"""
    from volym_amd import _lib
    s, (summary, faces) = S.scan_surface()
    assert S.rows(s.box) == 65792 > 256 * _lib.SURFACE_SCAN_ROWS                # 257 blocks: ceil(257 / 256) = 2 sums per thread
    assert int(summary["total"]) == len(faces) > 100000
    (x0, y0, z0), (x1, y1, z1) = s.box
    per_row = np.bincount((faces["z"].astype(np.int64) - z0) * (y1 - y0) + (faces["y"] - y0), minlength=S.rows(s.box))
    assert len(per_row) == S.rows(s.box) and int((per_row == 0).sum()) > S.rows(s.box) // 3      # the offsets are no arithmetic progression
    assert (np.diff(S.face_keys(faces)) > 0).all()
