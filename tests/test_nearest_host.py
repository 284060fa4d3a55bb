"""The nearest pass and the fill without a GPU: the C structs and constants, volym_nearest_check and volym_fill_check against the
Python checks, the host twin scene.nearest_volume against an all-pairs minimum with lexicographic ties, against the distance twin
and (where scipy is installed) against the distance of scipy's indices, every summary field recounted by loops, the tie scenes
against closed forms, scene.fill_volume against a per-texel loop and against the relabel twin with DISTANCE (Simple.grow's recipe),
and the separation of two touching balls composed from the twins.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import distance_scenes as DS
from tests import nearest_scenes as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

SUMMARY_LAYOUT = [("n_solid", 0, 8), ("n_present", 8, 8), ("n_finite", 16, 8), ("cell", 24, 2048), ("cell_present", 2072, 2048)]
SITE_LAYOUT = [("at", 0, 12), ("d2", 12, 4), ("label", 16, 4)]
FILL_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("give", 36, 256), ("take", 292, 256), ("d2_lo", 548, 4), ("d2_hi", 552, 4)]
# the issue's struct, field for field, is 556 bytes: 24 + 4 + 8 + 256 + 256 + 8 (its comment says 552)
FILL_BYTES = 556


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.NearestSummary) == 4120 == _lib.NEAREST_SUMMARY_DTYPE.itemsize and C.sizeof(_lib.NearestSite) == 20 and C.sizeof(_lib.Fill) == FILL_BYTES
    for struct, dtype, layout in ((_lib.NearestSummary, _lib.NEAREST_SUMMARY_DTYPE, SUMMARY_LAYOUT), (_lib.NearestSite, None, SITE_LAYOUT), (_lib.Fill, None, FILL_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    consts = [_lib.NEAREST_NONE, _lib.FILL_UNCUT, _lib.FILL_DRY_RUN]
    assert consts == [0xFFFFFFFF, 1, 2]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(struct volym_nearest_summary), sizeof(struct volym_nearest_site), sizeof(volym_fill));\n' +
                   "".join('  printf(" %%zu", offsetof(struct volym_nearest_summary, %s));\n' % f for f, _, _ in SUMMARY_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_nearest_site, %s));\n' % f for f, _, _ in SITE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(volym_fill, %s));\n' % f for f, _, _ in FILL_LAYOUT) +
                   '  printf(" %u %d %d %d", VOLYM_NEAREST_NONE, VOLYM_FILL_UNCUT, VOLYM_FILL_DRY_RUN, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [4120, 20, FILL_BYTES] + [o for layout in (SUMMARY_LAYOUT, SITE_LAYOUT, FILL_LAYOUT) for _, o, _ in layout] + consts + [2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_nearest_pass", "volym_nearest_check", "volym_read_nearest", "volym_read_nearest_sites", "volym_read_nearest_labels", "volym_nearest_at",
                 "volym_nearest_device_ptr", "volym_nearest_sites_device_ptr", "volym_nearest_labels_device_ptr", "volym_fill_labels", "volym_fill_check"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("nearest_pass", "read_nearest", "read_nearest_sites", "read_nearest_labels", "nearest_at", "fill_labels"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("nearest", "fill", "separate"):
        assert callable(getattr(demo.Simple, name))
    for name in ("check_nearest", "nearest_volume", "Fill", "check_fill", "fill_volume"):
        assert callable(getattr(scene, name))
    assert "import scipy" not in open(scene.__file__).read() and "from scipy" not in open(scene.__file__).read()


def test_the_nearest_check_and_its_twin_give_the_same_verdict(volym_lib):
    """every row of the distance check's table, with INSIDE turned into a refusal"""
    from tests.test_distance_host import _check_rows
    from volym_amd import scene
    insides = 0
    for name, d, dims, valid in _check_rows():
        inside = bool(d.flags & DS.INSIDE)
        insides += inside and valid
        valid = valid and not inside
        rc = volym_lib.volym_nearest_check(C.byref(d.to_c()), (C.c_uint32 * 3)(*dims))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_nearest(d, dims) is d, name
        else:
            with pytest.raises(ValueError):
                scene.check_nearest(d, dims)
    assert insides >= 2
    assert volym_lib.volym_nearest_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_nearest_check(C.byref(scene.Distance(dims=(1, 1, 1)).to_c()), None) == E_INVALID


def _fill_rows():
    """(name, request, valid) in a volume of 9 x 7 x 5"""
    from volym_amd import scene
    d = (9, 7, 5)
    F = scene.Fill
    whole = ((0, 0, 0), d)
    rows = [("whole", F(whole), True), ("empty on x", F(((3, 0, 0), (3, 7, 5))), True), ("empty at the far corner", F((d, d)), True), ("one texel", F(((8, 6, 4), d)), True),
            ("uncut", F(whole, 1), True), ("dry run", F(whole, 2), True), ("both flags", F(whole, 3), True), ("flag 4", F(whole, 4), False),
            ("flag 16", F(whole, 16), False), ("flag 2^31", F(whole, 1 << 31), False),
            ("window 0..0", F(whole, window=(0, 0)), True), ("window 255..255", F(whole, window=(255, 255)), True), ("window 9..8", F(whole, window=(9, 8)), False),
            ("window 0..256", F(whole, window=(0, 256)), False), ("window 256..256", F(whole, window=(256, 256)), False),
            ("band 0..0", F(whole, d2=(0, 0)), True), ("band 7..7", F(whole, d2=(7, 7)), True), ("band 8..7", F(whole, d2=(8, 7)), False),
            ("band to 2^32 - 1", F(whole, d2=(0, 2 ** 32 - 1)), True), ("band 2^32 - 1 .. 0", F(whole, d2=(2 ** 32 - 1, 0)), False),
            ("no label gives or takes", F(whole, give=np.zeros(256), take=np.zeros(256)), True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, F(((0, 0, 0), tuple(hi))), False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, F((tuple(lo), tuple(hi))), False))
    return d, rows


def test_the_fill_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    dims, rows = _fill_rows()
    for name, f, valid in rows:
        rc = volym_lib.volym_fill_check(C.byref(f.to_c()), (C.c_uint32 * 3)(*dims))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_fill(f, dims) is f, name
        else:
            with pytest.raises(ValueError):
                scene.check_fill(f, dims)
    assert volym_lib.volym_fill_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_fill_check(C.byref(scene.Fill(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    for bad in (dict(d2=(0, 2 ** 32)), dict(window=(0, -1)), dict(give=np.full(256, 256)), dict(take=np.zeros(255))):
        with pytest.raises(ValueError):
            scene.Fill(dims=(2, 2, 2), **bad).to_c()


# ---- the twin against the rule --------------------------------------------------------------------------------------------------
def _random_cases(seed, n):
    """(dims, vol, labels, request): boxes up to 7^3 inside volumes up to 8^3, weights from {1, 4, 9, 25, 64}, densities from empty to
    full"""
    from volym_amd import scene
    rng = np.random.default_rng(seed)
    for k in range(n):
        dims = tuple(int(v) for v in rng.integers(1, 9, 3))
        nx, ny, nz = dims
        fill = (0.0, 0.05, 0.3, 0.7, 0.95, 1.0)[k % 6]
        vol = np.where(rng.random(nx * ny * nz) < fill, rng.integers(1, 256, nx * ny * nz), 0).astype(np.uint8)
        lab = rng.integers(0, 4, nx * ny * nz).astype(np.uint8)
        lo = tuple(int(rng.integers(0, max(n_ - 6, 1))) for n_ in dims)
        hi = tuple(int(rng.integers(l + 1, min(l + 7, n_) + 1)) for l, n_ in zip(lo, dims))
        select = np.ones(256, np.int64) if k % 3 == 0 else (rng.random(256) < 0.6).astype(np.int64)
        weight = tuple(int(v) for v in rng.choice([1, 4, 9, 25, 64], 3))
        yield dims, vol, lab, scene.Distance((lo, hi), 0, int(rng.choice([1, 1, 100])), select, weight)


def _box_bytes(dims, vol, lab, d):
    nx, ny, nz = dims
    (x0, y0, z0), (x1, y1, z1) = d.box
    b = vol.reshape(nz, ny, nx)[z0:z1, y0:y1, x0:x1]
    l = lab.reshape(nz, ny, nx)[z0:z1, y0:y1, x0:x1]
    return b, l, (b >= d.min_byte) & (np.asarray(d.select)[l] != 0)


def test_the_twin_is_the_all_pairs_minimum_with_lexicographic_ties():
    from volym_amd import scene
    n = tied = 0
    for dims, vol, lab, d in _random_cases(5, 300):
        summary, sites, near = scene.nearest_volume(vol, dims, d, labels=lab)
        b, l, solid = _box_bytes(dims, vol, lab, d)
        want_sites, want_near = NS.brute_force(solid, l, d.weight)
        assert sites.dtype == np.uint32 and near.dtype == np.uint8
        assert np.array_equal(sites, want_sites) and np.array_equal(near, want_near), (dims, d.box, d.weight)
        # how many texels have more than one nearest solid texel: the ties are exercised
        if solid.any():
            d2 = scene.nearest_d2(sites, d.box, d.weight)
            zz, yy, xx = np.indices(solid.shape)
            for z, y, x in np.argwhere(solid)[:40].tolist():
                other = d.weight[0] * (xx - x) ** 2 + d.weight[1] * (yy - y) ** 2 + d.weight[2] * (zz - z) ** 2
                tied += int(((other == d2) & (sites != x + solid.shape[2] * (y + solid.shape[1] * z))).sum())
        n += 1
    assert n == 300 and tied > 500


def test_the_distance_to_the_site_is_the_distance_map():
    """on every request of the distance tests without INSIDE, under every cut, and on their constructed scenes"""
    from tests.test_distance_host import _NoContext
    from volym_amd import scene
    checked = 0
    for which in (NS.scene_a, NS.scene_b):
        host = which()
        for turn, (step, box, plane, hidden) in enumerate(NS.CUTS):
            host.set_cut(_NoContext(), box, plane, hidden)
            for flags in (0, NS.UNCUT):
                for name, d in NS.requests(flags, turn)[turn % 2::2]:
                    summary, sites, near = NS.expect(host, d)
                    want, dmap = DS.expect(host, d)
                    assert np.array_equal(scene.nearest_d2(sites, d.box, d.weight).astype(np.uint32), dmap), (step, name)
                    assert [int(summary[k]) for k in ("n_solid", "n_present", "n_finite")] == [int(want[k]) for k in ("n_solid", "n_present", "n_finite")], (step, name)
                    checked += 1
    assert checked > 80


def test_the_twin_against_the_distance_of_scipys_indices():
    ndimage = pytest.importorskip("scipy.ndimage")
    from volym_amd import scene
    for dims, vol, lab, d in _random_cases(9, 60):
        _, sites, _ = scene.nearest_volume(vol, dims, d, labels=lab)
        _, _, solid = _box_bytes(dims, vol, lab, d)
        if not solid.any():
            assert (sites == NS.NONE).all()
            continue
        sampling = [math.sqrt(d.weight[2]), math.sqrt(d.weight[1]), math.sqrt(d.weight[0])]
        iz, iy, ix = ndimage.distance_transform_edt(~solid, sampling=sampling, return_distances=False, return_indices=True)
        zz, yy, xx = np.indices(solid.shape)
        theirs = d.weight[0] * (xx - ix) ** 2 + d.weight[1] * (yy - iy) ** 2 + d.weight[2] * (zz - iz) ** 2        # (its ties are its own: only the distance)
        assert np.array_equal(theirs, scene.nearest_d2(sites, d.box, d.weight)), (dims, d.box, d.weight)


def test_the_summary_is_the_maps_and_the_bytes_recounted():
    from volym_amd import scene
    waiting = 0
    for dims, vol, lab, d in _random_cases(13, 60):
        summary, sites, near = scene.nearest_volume(vol, dims, d, labels=lab)
        b, l, solid = _box_bytes(dims, vol, lab, d)
        want = NS.summary_by_loops(sites, near, b, l, d)
        for k in ("n_solid", "n_present", "n_finite"):
            assert int(summary[k]) == want[k], (k, dims, d.box)
        assert summary["cell"].tolist() == want["cell"] and summary["cell_present"].tolist() == want["cell_present"]
        assert int(summary["cell"].sum()) == int(summary["n_finite"]) == (sites.size if solid.any() else 0)
        if solid.any():
            assert int(summary["cell_present"].sum()) == int(summary["n_present"]) - int(summary["n_solid"])
        waiting += int(summary["cell_present"].sum())
    assert waiting > 100


def test_the_tie_scenes_and_the_closed_forms():
    from volym_amd import scene
    for name, (dims, vol, lab, d, closed) in NS.constructed().items():
        result = scene.nearest_volume(vol, dims, d, labels=lab)
        NS.check_closed(name, result, closed, d)
        b, l, solid = _box_bytes(dims, vol, lab, d)
        if b.size <= 4000:
            want_sites, want_near = NS.brute_force(solid, l, d.weight)
            assert np.array_equal(result[1], want_sites) and np.array_equal(result[2], want_near), name
    assert len(NS.ties()) == 18


def test_without_labels_the_empty_box_and_the_helpers():
    from volym_amd import scene
    dims, vol, lab, d, _ = NS.ties()["mirrored along y"]
    summary, sites, near = scene.nearest_volume(vol, dims, d)
    assert not near.any() and int(summary["cell"][0]) == sites.size and int(summary["cell"].sum()) == sites.size
    assert np.array_equal(sites, scene.nearest_volume(vol, dims, d, labels=lab)[1])
    summary, sites, near = scene.nearest_volume(np.zeros(8, np.uint8), (2, 2, 2), scene.Distance(((1, 1, 1), (1, 2, 2))))
    assert sites.shape == near.shape == (0, 0, 0) and summary.tobytes() == scene.empty_nearest()[0].tobytes() == bytes(4120)
    with pytest.raises(ValueError):
        scene.nearest_volume(vol, dims, d.replace(flags=DS.INSIDE))
    s = scene.nearest_summary(scene.nearest_volume(vol, dims, d, labels=lab)[0], {1: "low", 2: "high"})
    assert set(s["cells"]) == {"low", "high"} and s["cells"]["low"]["texels"] + s["cells"]["high"]["texels"] == 9 * 7 * 5 and s["n_solid"] == 2
    assert s["cells"]["low"]["fill"] == 0                                  # (nothing is present but the seeds)


# ---- the fill -------------------------------------------------------------------------------------------------------------------
def _fill_by_loops(vol, uncut, dims, f, labels, sites, near, pass_box, weight):
    """the rule, a texel at a time"""
    nx, ny, nz = dims
    (x0, y0, z0), (x1, y1, z1) = f.box
    (px, py, pz), (qx, qy, qz) = pass_box
    w, h = qx - px, qy - py
    src = (uncut if f.flags & NS.FILL_UNCUT else vol).reshape(nz, ny, nx)
    new = labels.reshape(nz, ny, nx).copy()
    old = labels.reshape(nz, ny, nx)
    changed, left, arrived, hull = 0, [0] * 256, [0] * 256, None
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                l, s, n = int(old[z, y, x]), int(sites[z - pz, y - py, x - px]), int(near[z - pz, y - py, x - px])
                if not f.give[l] or s == NS.NONE or not f.take[n] or n == l or not f.window[0] <= int(src[z, y, x]) <= f.window[1]:
                    continue
                sx, sy, sz = px + s % w, py + (s // w) % h, pz + s // (w * h)
                d2 = weight[0] * (x - sx) ** 2 + weight[1] * (y - sy) ** 2 + weight[2] * (z - sz) ** 2
                if not f.d2[0] <= d2 <= f.d2[1]:
                    continue
                changed += 1
                left[l] += 1
                arrived[n] += 1
                hull = (x, y, z, x + 1, y + 1, z + 1) if hull is None else tuple(min(a, b) for a, b in zip(hull[:3], (x, y, z))) + tuple(max(a, b) for a, b in zip(hull[3:], (x + 1, y + 1, z + 1)))
                if not f.flags & NS.FILL_DRY_RUN:
                    new[z, y, x] = n
    return new, changed, left, arrived, list(hull or (0,) * 6)


def test_the_fill_twin_against_a_per_texel_loop():
    from tests.test_distance_host import _NoContext
    from volym_amd import scene
    host = NS.scene_a()
    changed = 0
    for cut in (None, (NS.BOX, NS.PLANE, NS.HIDDEN)):
        if cut:
            host.set_cut(_NoContext(), *cut)
        now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
        for case in NS.fill_cases():
            _, sites, near = NS.expect(host, case.distance)
            new, result = NS.fill_expect(host, case)
            want = _fill_by_loops(now, host.vol, host.dims, case.fill, host.labels, sites, near, case.distance.box, case.distance.weight)
            assert np.array_equal(new, want[0].ravel()), case.name
            assert [int(result["changed"]), result["left"].tolist(), result["arrived"].tolist(), result["box"].tolist()] == list(want[1:]), case.name
            assert int(result["changed"]) == 0 if case.trivial else (int(result["changed"]) > 0 or cut is not None), (case.name, cut is not None)
            assert (case.fill.flags & NS.FILL_DRY_RUN != 0 or int(result["changed"]) == 0) == np.array_equal(new, host.labels), case.name
            changed += int(result["changed"])
    assert changed > 10000
    by_name = {c.name: c for c in NS.fill_cases()}
    host = NS.scene_a()
    # the texel whose nearest label does not take stays: it does not go to the second nearest
    case = by_name["take excludes the nearest: the texel stays"]
    _, sites, near = NS.expect(host, case.distance)
    new, result = NS.fill_expect(host, case)
    old = host.labels
    gives = np.isin(old, [0, 4])
    assert int((gives & (near.ravel() != 2)).sum()) > 100 and np.array_equal(new[gives & (near.ravel() != 2)], old[gives & (near.ravel() != 2)])
    assert np.array_equal(new != old, gives & (near.ravel() == 2))


def test_a_fill_from_one_segment_is_the_relabel_by_distance():
    """Simple.grow's recipe: a distance pass from one segment and the edit with DISTANCE, against a nearest pass from the same segment
    and the fill with give = into and the band (0, R): the same labels and the same result"""
    from volym_amd import _lib, scene
    for host, seed, into in ((NS.scene_a(), 2, (0, 1, 3)), (NS.scene_a(), 4, (0,)), (NS.scene_b(), 77, tuple(range(0, 256, 3)))):
        into = tuple(v for v in into if v != seed)
        for weight, band in (((1, 1, 1), 4), ((1, 4, 25), 30), ((64, 1, 9), 64)):
            d = scene.Distance(dims=host.dims, select=NS.table(seed), weight=weight)
            _, dmap = scene.distance_volume(host.vol, host.dims, d, labels=host.labels)
            old_way = scene.relabel_volume(host.vol, host.dims, scene.Relabel(None, _lib.RELABEL_DISTANCE, to={v: seed for v in into}, d2=(0, band), dims=host.dims),
                                           host.labels, dmap=dmap, dmap_box=d.box)
            _, sites, near = scene.nearest_volume(host.vol, host.dims, d, labels=host.labels)
            new_way = scene.fill_volume(host.vol, host.dims, scene.Fill(None, 0, (0, 255), NS.table(*into), NS.table(seed), (0, band), dims=host.dims), host.labels,
                                        sites, near, d.box, weight)
            assert np.array_equal(old_way[0], new_way[0]) and old_way[1].tobytes() == new_way[1].tobytes(), (seed, weight, band)
            assert int(new_way[1]["changed"]) > 20, (seed, weight, band)


def separate_by_twins(dims, vol, labels, name, r, most=8):
    """Simple.separate composed from the twins (labels: uint8 flat; new labels are the smallest unused): (labels after, the pieces'
    labels largest first)"""
    from volym_amd import _lib, scene
    band = int(math.floor(float(r) ** 2 + 1e-9))
    free = [v for v in range(1, 256) if not (labels == v).any()]
    first = free.pop(0)
    inside = scene.Distance(dims=dims, flags=DS.INSIDE, select=NS.table(name))
    _, dmap = scene.distance_volume(vol, dims, inside, labels=labels)
    lab, _ = scene.relabel_volume(vol, dims, scene.Relabel(None, _lib.RELABEL_DISTANCE, to={name: first}, d2=(band + 1, DS.NONE - 1), dims=dims), labels,
                                  dmap=dmap, dmap_box=inside.box)
    comp = scene.Components(dims=dims, select=NS.table(first))
    summary, table, ids = scene.components_volume(vol, dims, comp, labels=lab.ravel())
    if not len(table):
        return lab.ravel(), []
    order = np.argsort(-table["count"].astype(np.int64), kind="stable")[:most].tolist()
    pieces = [first]
    for k in order[1:]:
        value = free.pop(0)
        lab, _ = scene.relabel_volume(vol, dims, scene.Relabel(None, _lib.RELABEL_IDS, to={first: value}, ids=(k, k), dims=dims), lab.ravel(), ids=ids, ids_box=comp.box)
        pieces.append(value)
    lab, _ = scene.relabel_volume(vol, dims, scene.Relabel(None, _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT, to={first: name}, ids=(order[0], order[0]), dims=dims),
                                  lab.ravel(), ids=ids, ids_box=comp.box)
    near = scene.Distance(dims=dims, select=NS.table(*pieces))
    _, sites, near_labels = scene.nearest_volume(vol, dims, near, labels=lab.ravel())
    lab, _ = scene.fill_volume(vol, dims, scene.Fill(None, 0, (0, 255), NS.table(name), NS.table(*pieces), dims=dims), lab.ravel(), sites, near_labels, near.box)
    return lab.ravel(), pieces


@pytest.mark.parametrize("apart", [9, 10])
def test_two_touching_balls_separate_at_the_mid_plane(apart):
    dims, vol, labels = NS.two_balls(apart)
    nx, ny, nz = dims
    after, pieces = separate_by_twins(dims, vol, labels, 1, 5)            # (at depth 4 the neck, 4.5 texels wide at x = 14, still holds)
    assert len(pieces) == 2 and not (after == 1).any()
    got = after.reshape(nz, ny, nx)
    was = labels.reshape(nz, ny, nx) == 1
    xx = np.indices((nz, ny, nx))[2]
    # the texels left of the mid-plane go to the first piece, those right of it to the second; 10 apart the plane x = 15 holds texels,
    # whose two nearest core texels mirror each other: the one with the lower x is the lower site
    mid = 10 + apart / 2.0
    assert np.array_equal(got[was & (xx <= mid)], np.full(int((was & (xx <= mid)).sum()), pieces[0]))
    assert np.array_equal(got[was & (xx > mid)], np.full(int((was & (xx > mid)).sum()), pieces[1]))
    assert (apart == 10) == bool((was & (xx == mid)).any())
    assert np.array_equal(got[~was], labels.reshape(nz, ny, nx)[~was])
    assert int((after == pieces[0]).sum()) + int((after == pieces[1]).sum()) == int(was.sum())
