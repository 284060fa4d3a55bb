"""The geodesic pass and the flood without a GPU: the C structs and constants, volym_geodesic_check and volym_flood_check against
the Python checks, the layered host twin scene.geodesic_volume against a per-label breadth-first search and against a restatement of
the device's schedule (tiles relaxed in a random order against halos of mixed age until nothing changes), the reached count against
the components twin, every summary field recounted by loops, the constructed scenes against closed forms, scene.flood_volume
against a per-texel loop, and a truncated pass against the untruncated one.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import geodesic_scenes as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

GEODESIC_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("seed", 36, 256), ("through", 292, 256), ("max_steps", 548, 4),
                   ("n_points", 552, 4), ("points", 556, 768)]
SUMMARY_LAYOUT = [("n_seed", 0, 8), ("n_medium", 8, 8), ("n_reached", 16, 8), ("max_steps", 24, 4), ("max_at", 28, 12), ("cell", 40, 2048), ("cell_medium", 2088, 2048),
                  ("hist", 4136, 2048)]
SITE_LAYOUT = [("steps", 0, 4), ("label", 4, 4)]
FLOOD_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("give", 36, 256), ("take", 292, 256), ("to", 548, 256), ("steps_lo", 804, 4),
                ("steps_hi", 808, 4)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Geodesic) == 1324 and C.sizeof(_lib.GeodesicSummary) == 6184 == _lib.GEODESIC_SUMMARY_DTYPE.itemsize
    assert C.sizeof(_lib.GeodesicSite) == 8 and C.sizeof(_lib.Flood) == 812
    for struct, dtype, layout in ((_lib.Geodesic, None, GEODESIC_LAYOUT), (_lib.GeodesicSummary, _lib.GEODESIC_SUMMARY_DTYPE, SUMMARY_LAYOUT),
                                  (_lib.GeodesicSite, None, SITE_LAYOUT), (_lib.Flood, None, FLOOD_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    consts = [_lib.GEODESIC_UNCUT, _lib.GEODESIC_POINTS_MAX, _lib.GEODESIC_STEPS_MAX, _lib.GEODESIC_BOX_MAX, _lib.GEODESIC_NONE, _lib.FLOOD_UNCUT, _lib.FLOOD_DRY_RUN]
    assert consts == [1, 64, 2 ** 24 - 3, 2 ** 31 - 2, 0xFFFFFFFF, 1, 2]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu", sizeof(volym_geodesic), sizeof(struct volym_geodesic_summary), sizeof(struct volym_geodesic_site), sizeof(volym_flood));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_geodesic, %s));\n' % f for f, _, _ in GEODESIC_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_geodesic_summary, %s));\n' % f for f, _, _ in SUMMARY_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_geodesic_site, %s));\n' % f for f, _, _ in SITE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(volym_flood, %s));\n' % f for f, _, _ in FLOOD_LAYOUT) +
                   '  printf(" %d %u %u %u %u %d %d %d", VOLYM_GEODESIC_UNCUT, VOLYM_GEODESIC_POINTS_MAX, VOLYM_GEODESIC_STEPS_MAX, VOLYM_GEODESIC_BOX_MAX, VOLYM_GEODESIC_NONE,'
                   ' VOLYM_FLOOD_UNCUT, VOLYM_FLOOD_DRY_RUN, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [1324, 6184, 8, 812] + [o for layout in (GEODESIC_LAYOUT, SUMMARY_LAYOUT, SITE_LAYOUT, FLOOD_LAYOUT) for _, o, _ in layout] + consts + [2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_geodesic_pass", "volym_geodesic_check", "volym_read_geodesic", "volym_read_geodesic_map", "volym_geodesic_at", "volym_geodesic_device_ptr",
                 "volym_geodesic_map_device_ptr", "volym_flood_labels", "volym_flood_check"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("geodesic_pass", "read_geodesic", "read_geodesic_map", "geodesic_at", "flood_labels"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("reach", "grow_through", "wand_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Geodesic", "check_geodesic", "geodesic_volume", "geodesic_summary", "Flood", "check_flood", "flood_volume"):
        assert callable(getattr(scene, name))


def _geodesic_rows():
    """(name, request, valid) in a volume of 9 x 7 x 5"""
    from volym_amd import scene
    d = (9, 7, 5)
    G = scene.Geodesic
    whole = ((0, 0, 0), d)
    inner = ((2, 1, 1), (7, 6, 4))
    rows = [("whole", G(whole), True), ("empty on x", G(((3, 0, 0), (3, 7, 5))), True), ("empty at the far corner", G((d, d)), True), ("one texel", G(((8, 6, 4), d)), True),
            ("uncut", G(whole, 1), True), ("flag 2", G(whole, 2), False), ("flag 3", G(whole, 3), False), ("flag 2^31", G(whole, 1 << 31), False),
            ("window 0..0", G(whole, window=(0, 0)), True), ("window 255..255", G(whole, window=(255, 255)), True), ("window 9..8", G(whole, window=(9, 8)), False),
            ("window 0..256", G(whole, window=(0, 256)), False), ("window 256..256", G(whole, window=(256, 256)), False),
            ("one step", G(whole, max_steps=1), True), ("the most steps", G(whole, max_steps=2 ** 24 - 3), True), ("a step too many", G(whole, max_steps=2 ** 24 - 2), False),
            ("steps 2^32 - 1", G(whole, max_steps=2 ** 32 - 1), False),
            ("no table set", G(whole, seed=np.zeros(256), through=np.zeros(256)), True),
            ("a point", G(whole, points=[(8, 6, 4)]), True), ("a duplicate point", G(whole, points=[(1, 2, 3), (1, 2, 3)]), True),
            ("64 points", G(whole, points=[(k % 9, k % 7, k % 5) for k in range(64)]), True), ("65 points", G(whole, points=[(k % 9, k % 7, k % 5) for k in range(65)]), False),
            ("a point in the inner box", G(inner, points=[(2, 1, 1), (6, 5, 3)]), True), ("a point in an empty box", G(((3, 0, 0), (3, 7, 5)), points=[(3, 0, 0)]), False)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, G(((0, 0, 0), tuple(hi))), False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, G((tuple(lo), tuple(hi))), False))
        p = [2, 1, 1]; p[a] -= 1
        rows.append(("a point below the box on axis %d" % a, G(inner, points=[(3, 3, 3), tuple(p)]), False))
        p = [6, 5, 3]; p[a] += 1
        rows.append(("a point at the box's hi on axis %d" % a, G(inner, points=[tuple(p)]), False))
    return d, rows


def test_the_geodesic_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    dims, rows = _geodesic_rows()
    for name, g, valid in rows:
        rc = volym_lib.volym_geodesic_check(C.byref(g.to_c()), (C.c_uint32 * 3)(*dims))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_geodesic(g, dims) is g, name
        else:
            with pytest.raises(ValueError):
                scene.check_geodesic(g, dims)
    big = (4096, 4096, 4096)                                       # the over-large box: one texel more than 2^31 - 2 allows
    for box, valid in ((((0, 0, 0), (4096, 4096, 127)), True), (((0, 0, 0), (4096, 4096, 128)), False), (((0, 0, 0), (2048, 1024, 1024)), False),
                       (((1, 0, 0), (2048, 1024, 1024)), True)):
        g = scene.Geodesic(box)
        assert (volym_lib.volym_geodesic_check(C.byref(g.to_c()), (C.c_uint32 * 3)(*big)) == 0) == valid, box
        if not valid:
            with pytest.raises(ValueError):
                scene.check_geodesic(g, big)
    assert volym_lib.volym_geodesic_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_geodesic_check(C.byref(scene.Geodesic(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    for bad in (dict(max_steps=2 ** 32), dict(window=(0, -1)), dict(seed=np.full(256, 256)), dict(through=np.zeros(255)), dict(points=[(1, 2)]), dict(points=[(0, 0, -1)])):
        with pytest.raises(ValueError):
            scene.Geodesic(dims=(2, 2, 2), **bad).to_c()


def _flood_rows():
    from volym_amd import scene
    d = (9, 7, 5)
    F = scene.Flood
    whole = ((0, 0, 0), d)
    rows = [("whole", F(whole), True), ("empty on x", F(((3, 0, 0), (3, 7, 5))), True), ("empty at the far corner", F((d, d)), True), ("one texel", F(((8, 6, 4), d)), True),
            ("uncut", F(whole, 1), True), ("dry run", F(whole, 2), True), ("both flags", F(whole, 3), True), ("flag 4", F(whole, 4), False),
            ("flag 16", F(whole, 16), False), ("flag 2^31", F(whole, 1 << 31), False),
            ("window 0..0", F(whole, window=(0, 0)), True), ("window 255..255", F(whole, window=(255, 255)), True), ("window 9..8", F(whole, window=(9, 8)), False),
            ("window 0..256", F(whole, window=(0, 256)), False), ("window 256..256", F(whole, window=(256, 256)), False),
            ("band 0..0", F(whole, steps=(0, 0)), True), ("band 7..7", F(whole, steps=(7, 7)), True), ("band 8..7", F(whole, steps=(8, 7)), False),
            ("band to 2^32 - 1", F(whole, steps=(0, 2 ** 32 - 1)), True), ("band 2^32 - 1 .. 0", F(whole, steps=(2 ** 32 - 1, 0)), False),
            ("no label gives or takes", F(whole, give=np.zeros(256), take=np.zeros(256)), True), ("to renames", F(whole, to={0: 9, 3: 0}), True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, F(((0, 0, 0), tuple(hi))), False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, F((tuple(lo), tuple(hi))), False))
    return d, rows


def test_the_flood_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    dims, rows = _flood_rows()
    for name, f, valid in rows:
        rc = volym_lib.volym_flood_check(C.byref(f.to_c()), (C.c_uint32 * 3)(*dims))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_flood(f, dims) is f, name
        else:
            with pytest.raises(ValueError):
                scene.check_flood(f, dims)
    assert volym_lib.volym_flood_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_flood_check(C.byref(scene.Flood(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    for bad in (dict(steps=(0, 2 ** 32)), dict(window=(0, -1)), dict(give=np.full(256, 256)), dict(take=np.zeros(255)), dict(to=np.full(256, 256))):
        with pytest.raises(ValueError):
            scene.Flood(dims=(2, 2, 2), **bad).to_c()
    assert scene.Flood(dims=(2, 2, 2), to={0: 9}).to.tolist() == [9] + list(range(1, 256))


# ---- the twin against the rule restated ------------------------------------------------------------------------------------------------
def _random_boxes(n):
    """n random scenes up to 7^3: (dims, vol, labels, scene.Geodesic) with densities of matter from empty to full, labels 0..4 and
    the step limits 1, 2, 5 and none in turn"""
    from volym_amd import scene
    rng = np.random.default_rng(11)
    out = []
    for k in range(n):
        dims = tuple(int(v) for v in rng.integers(1, 8, 3))
        size = dims[0] * dims[1] * dims[2]
        share = (0.0, 0.3, 0.55, 0.7, 0.85, 1.0)[k % 6]
        vol = np.where(rng.random(size) < share, rng.integers(100, 256, size), rng.integers(0, 100, size)).astype(np.uint8)
        lab = rng.choice([0, 0, 0, 0, 0, 0, 1, 2, 3, 4], size).astype(np.uint8)
        pts = [tuple(int(rng.integers(0, d)) for d in dims) for _ in range(k % 3)]
        g = scene.Geodesic(None, 0, (100, 255), GS.table(1, 2, 3) if k % 5 else GS.table(2, 4), GS.table(0, 4) if k % 4 else GS.table(0, 1), (1, 2, 5, 0)[k % 4], pts, dims=dims)
        out.append((dims, vol, lab, g))
    return out


def _box_bytes(dims, vol, lab):
    return vol.reshape(dims[::-1]), lab.reshape(dims[::-1])


def test_the_twin_equals_a_search_per_label_on_random_boxes():
    from volym_amd import scene
    ties = reached = 0
    boxes = _random_boxes(320)
    for k, (dims, vol, lab, g) in enumerate(boxes):
        summary, keys = scene.geodesic_volume(vol, dims, g, labels=lab)
        b, l = _box_bytes(dims, vol, lab)
        seed, medium = GS.predicates(b, l, g)
        want, t = GS.brute_force(seed, medium, l, g.max_steps)
        assert np.array_equal(np.where(keys == np.uint32(GS.NONE), -1, keys.astype(np.int64)), want), (k, dims)
        ties += t
        reached += int(summary["n_reached"])
    assert len(boxes) >= 300 and ties > 500 and reached > 5000, (ties, reached)


def test_the_twin_equals_the_schedule_of_the_device_on_random_boxes():
    """tiles of 3 x 2 x 2, 2 x 3 x 1 and 4 x 4 x 4 in turn, relaxed in a random order against halos of mixed age"""
    from volym_amd import scene
    rng = np.random.default_rng(5)
    boxes = _random_boxes(320)[3::5]
    assert len(boxes) >= 60
    for k, (dims, vol, lab, g) in enumerate(boxes):
        _, keys = scene.geodesic_volume(vol, dims, g, labels=lab)
        b, l = _box_bytes(dims, vol, lab)
        seed, medium = GS.predicates(b, l, g)
        got = GS.scheduled(seed, medium, l, g.max_steps, ((3, 2, 2), (2, 3, 1), (4, 4, 4))[k % 3], rng)
        assert np.array_equal(np.where(keys == np.uint32(GS.NONE), -1, keys.astype(np.int64)), got), (k, dims)


def test_the_reached_count_from_one_texel_is_its_piece_in_the_components_twin():
    from volym_amd import scene
    dims = (19, 14, 11)
    rng = np.random.default_rng(8)
    n = dims[0] * dims[1] * dims[2]
    vol = np.where(rng.random(n) < 0.45, 200, 0).astype(np.uint8)
    lab = rng.integers(0, 3, n).astype(np.uint8)
    select = scene.surface_select([0, 2])
    c = scene.Components(None, 0, 1, select, dims=dims)
    summary, table, ids = scene.components_volume(vol, dims, c, labels=lab)[:3]
    counts = np.bincount(ids[ids != np.uint32(0xFFFFFFFF)].astype(np.int64))
    pieces = 0
    for piece in np.argsort(-counts)[:6].tolist():
        z, y, x = (int(v[0]) for v in np.nonzero(ids == piece))
        g = scene.Geodesic(None, 0, (1, 255), GS.table(), GS.table(0, 2), 0, [(x, y, z)], dims=dims)
        s, keys = scene.geodesic_volume(vol, dims, g, labels=lab)
        assert int(s["n_reached"]) == int(counts[piece]) and np.array_equal(keys != np.uint32(GS.NONE), ids == piece), piece
        pieces += int(counts[piece]) > 1
    assert pieces >= 3


def test_every_summary_field_recounted_by_loops():
    from volym_amd import scene
    for dims, vol, lab, g in _random_boxes(60)[::3] + [(GS.DIMS, GS.scene_a().vol, GS.scene_a().labels, g) for _, g in GS.requests()[:4]]:
        summary, keys = scene.geodesic_volume(vol, dims, g, labels=lab)
        if keys.size == 0:
            continue
        lo, hi = g.box
        sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        b, l = _box_bytes(dims, vol, lab)
        seed, medium = GS.predicates(b[sub], l[sub], g)
        want = GS.summary_by_loops(keys, seed, medium, lo)
        for f in ("n_seed", "n_medium", "n_reached", "max_steps"):
            assert int(summary[f]) == want[f], (f, dims)
        for f in ("max_at", "cell", "cell_medium", "hist"):
            assert summary[f].tolist() == want[f], (f, dims)


def test_the_constructed_scenes_have_their_closed_forms():
    from volym_amd import scene
    made = GS.constructed()
    assert len(GS.serpentine_path()) == 1339
    for name, (dims, vol, lab, g, closed) in made.items():
        GS.check_closed(name, scene.geodesic_volume(vol, dims, g, labels=lab), closed)
    # the premises of the late shorter route, from the twin: either route alone reaches T in its own length, the straight one is the
    # shorter, and it crosses at least four times as many tile faces
    dims, vol, lab, g, closed = made["late shorter route"]
    (t, (steps, label)), = closed["at"].items()
    winding, straight = closed["winding"], closed["straight"]
    alone = {}
    for l in (2, 9):
        _, keys = scene.geodesic_volume(vol, dims, g.replace(seed=GS.table(l)), labels=lab)
        alone[l] = int(keys[t[2], t[1], t[0]]) >> 8
    assert alone == {2: len(winding) - 1, 9: len(straight) - 1} and alone[9] < alone[2] and steps == alone[9] and label == 9
    assert GS.faces_crossed(straight) >= 4 * GS.faces_crossed(winding) > 0
    assert len({tuple(p[i] // GS.tile()[i] for i in range(3)) for p in winding}) <= 2
    # the mirrored seeds: the tied texel lies where its name says
    ext = GS.tile()
    for axis in range(3):
        (face,), = [list(made["mirrored along %s, on a tile face" % "xyz"[axis]][4]["at"])]
        (inside,), = [list(made["mirrored along %s, inside a tile" % "xyz"[axis]][4]["at"])]
        assert face[axis] % ext[axis] == 0 and face[axis] > 0 and 0 < inside[axis] % ext[axis] < ext[axis] - 1


def test_a_truncated_pass_is_the_untruncated_one_cut_off():
    from volym_amd import scene
    host = GS.scene_a()
    for _, g in GS.requests()[:6]:
        _, full = scene.geodesic_volume(host.vol, host.dims, g.replace(max_steps=0), labels=host.labels)
        for r in (1, 2, 4, 9):
            _, cut = scene.geodesic_volume(host.vol, host.dims, g.replace(max_steps=r), labels=host.labels)
            assert np.array_equal(cut, np.where((full != np.uint32(GS.NONE)) & ((full >> 8) > r), np.uint32(GS.NONE), full)), r


# ---- the flood's twin ------------------------------------------------------------------------------------------------------------------
def test_the_flood_twin_equals_a_loop_per_texel():
    from volym_amd import scene
    host = GS.scene_a()
    nx, ny, nz = host.dims
    changed = 0
    for case in GS.flood_cases():
        _, keys = GS.expect(host, case.geodesic)
        new, result = scene.flood_volume(host.vol, host.dims, case.flood, host.labels, keys, case.geodesic.box)
        f, (plo, phi) = case.flood, case.geodesic.box
        want = host.labels.reshape(nz, ny, nx).copy()
        count, left, arrived, hull = 0, [0] * 256, [0] * 256, None
        for z in range(f.box[0][2], f.box[1][2]):
            for y in range(f.box[0][1], f.box[1][1]):
                for x in range(f.box[0][0], f.box[1][0]):
                    l = int(want[z, y, x])
                    key = int(keys[z - plo[2], y - plo[1], x - plo[0]])
                    if not f.give[l] or key == GS.NONE:
                        continue
                    g, steps = key & 0xFF, key >> 8
                    n = int(f.to[g])
                    if not f.take[g] or n == l or not f.window[0] <= int(host.vol[x + nx * (y + ny * z)]) <= f.window[1] or not f.steps[0] <= steps <= f.steps[1]:
                        continue
                    count += 1
                    left[l] += 1
                    arrived[n] += 1
                    hull = [x, y, z, x + 1, y + 1, z + 1] if hull is None else [min(hull[0], x), min(hull[1], y), min(hull[2], z), max(hull[3], x + 1), max(hull[4], y + 1),
                                                                                  max(hull[5], z + 1)]
                    if not f.flags & GS.FLOOD_DRY_RUN:
                        want[z, y, x] = n
        assert (count == 0) == case.trivial, case.name
        assert int(result["changed"]) == count and result["left"].tolist() == left and result["arrived"].tolist() == arrived, case.name
        assert result["box"].tolist() == (hull or [0] * 6) and np.array_equal(new, want), case.name
        changed += count
    assert changed > 10000
