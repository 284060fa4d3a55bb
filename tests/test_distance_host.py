"""The distance pass without a GPU: the C structs and constants, volym_distance_check against scene.check_distance, the host twin
scene.distance_volume against a brute-force all-pairs minimum (and against scipy.ndimage.distance_transform_edt where scipy is
installed), the closed forms of the constructed scenes, the identities of the summary and the helpers of scene.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import distance_scenes as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

REQUEST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("select", 32, 256), ("weight", 288, 12)]
SUMMARY_LAYOUT = [("n_solid", 0, 8), ("n_present", 8, 8), ("n_finite", 16, 8), ("max_d2", 24, 4), ("max_at", 28, 12), ("near_d2", 40, 1024),
                  ("near_at", 1064, 3072), ("hist", 4136, 2048)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Distance) == 300 and C.sizeof(_lib.DistanceSummary) == 6184 and _lib.DISTANCE_SUMMARY_DTYPE.itemsize == 6184
    for struct, dtype, layout in ((_lib.Distance, None, REQUEST_LAYOUT), (_lib.DistanceSummary, _lib.DISTANCE_SUMMARY_DTYPE, SUMMARY_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    consts = [_lib.DISTANCE_UNCUT, _lib.DISTANCE_INSIDE, _lib.DISTANCE_WEIGHT_MAX, _lib.DISTANCE_BOX_MAX, _lib.DISTANCE_NONE, _lib.DISTANCE_BINS]
    assert consts == [1, 2, 64, 2 ** 31 - 2, 0xFFFFFFFF, 256]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(volym_distance), sizeof(struct volym_distance_summary));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_distance, %s));\n' % f for f, _, _ in REQUEST_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_distance_summary, %s));\n' % f for f, _, _ in SUMMARY_LAYOUT) +
                   '  printf(" %d %d %u %u %u %d %d", VOLYM_DISTANCE_UNCUT, VOLYM_DISTANCE_INSIDE, VOLYM_DISTANCE_WEIGHT_MAX, VOLYM_DISTANCE_BOX_MAX,\n'
                   '         VOLYM_DISTANCE_NONE, VOLYM_DISTANCE_BINS, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [300, 6184] + [o for _, o, _ in REQUEST_LAYOUT] + [o for _, o, _ in SUMMARY_LAYOUT] + consts + [2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_distance_pass", "volym_distance_check", "volym_read_distance", "volym_read_distance_map", "volym_distance_at",
                 "volym_distance_device_ptr", "volym_distance_map_device_ptr"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("distance_pass", "read_distance", "read_distance_map", "distance_at"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("distance", "thickness", "clearance", "distance_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Distance", "check_distance", "distance_volume", "distance_summary", "distance_weights"):
        assert callable(getattr(scene, name))
    assert "import scipy" not in open(scene.__file__).read() and "from scipy" not in open(scene.__file__).read()


def _check_rows():
    """(name, request, dims, valid)"""
    from volym_amd import scene
    d = (9, 7, 5)
    F = scene.Distance
    whole = ((0, 0, 0), d)
    big = (4096, 4096, 4096)
    rows = [("whole", F(whole), d, True), ("empty on x", F(((3, 0, 0), (3, 7, 5))), d, True), ("empty at the far corner", F((d, d)), d, True),
            ("one texel", F(((8, 6, 4), d)), d, True), ("uncut", F(whole, 1), d, True), ("inside", F(whole, 2), d, True), ("both flags", F(whole, 3), d, True),
            ("flag 4", F(whole, 4), d, False), ("flag 2^31", F(whole, 1 << 31), d, False),
            ("min_byte 0", F(whole, 0, 0), d, False), ("min_byte 255", F(whole, 0, 255), d, True), ("min_byte 256", F(whole, 0, 256), d, False),
            ("weights 64", F(whole, weight=(64, 64, 64)), d, True), ("weights 1, 25, 64", F(whole, weight=(1, 25, 64)), d, True),
            # the box limit from both sides: 2 x 3 x 357913941 = 2^31 - 2 texels pass, 2^31 - 1 do not
            ("box of 2^31 - 2048 texels", F(((0, 0, 0), (4096, 4096, 127))), big, True),
            ("box of 2^31 texels", F(((0, 0, 0), (4096, 4096, 128))), big, False),
            ("box of 2^31 - 2 texels", F(((0, 0, 0), (2, 3, 357913941))), (2, 3, 357913941), True),
            ("box of 2^31 - 1 texels", F(((0, 0, 0), (1, 1, 2 ** 31 - 1))), (1, 1, 2 ** 31 - 1), False),
            ("the largest volume", F(((0, 0, 0), big)), big, False), ("a slab of it", F(((0, 0, 4000), big)), big, True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, F(((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, F((tuple(lo), tuple(hi))), d, False))
        for v, ok in ((0, False), (65, False), (2 ** 32 - 1, False), (63, True)):
            w = [1, 1, 1]; w[a] = v
            rows.append(("weight %d on axis %d" % (v, a), F(whole, weight=tuple(w)), d, ok))
    return rows


def test_the_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import _lib, scene
    assert 2 * 3 * 357913941 == _lib.DISTANCE_BOX_MAX
    for name, d, dims, valid in _check_rows():
        c_dims = (C.c_uint32 * 3)(*dims)
        rc = volym_lib.volym_distance_check(C.byref(d.to_c()), c_dims)
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_distance(d, dims) is d, name
        else:
            with pytest.raises(ValueError):
                scene.check_distance(d, dims)
    assert volym_lib.volym_distance_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_distance_check(C.byref(scene.Distance(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    with pytest.raises(ValueError):
        scene.Distance(dims=(2, 2, 2), weight=(1, 1, -1)).to_c()


# ---- the twin against the rule --------------------------------------------------------------------------------------------------
def _random_cases(seed, n):
    """(dims, vol, labels, request): boxes up to 7^3 inside volumes up to 8^3, densities from empty to full"""
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
        weight = tuple(int(v) for v in rng.choice([1, 4, 25, 64], 3))
        for flags in (0, DS.INSIDE):
            yield dims, vol, lab, scene.Distance((lo, hi), flags, int(rng.choice([1, 1, 100])), select, weight)


def _solid(dims, vol, lab, d):
    nx, ny, nz = dims
    (x0, y0, z0), (x1, y1, z1) = d.box
    b = vol.reshape(nz, ny, nx)[z0:z1, y0:y1, x0:x1]
    l = lab.reshape(nz, ny, nx)[z0:z1, y0:y1, x0:x1]
    return b, l, (b >= d.min_byte) & (np.asarray(d.select)[l] != 0)


def test_the_twin_is_the_all_pairs_minimum():
    from volym_amd import scene
    n = 0
    for dims, vol, lab, d in _random_cases(5, 150):
        summary, dmap = scene.distance_volume(vol, dims, d, labels=lab)
        _, _, solid = _solid(dims, vol, lab, d)
        want = DS.brute_force(solid, d.weight, bool(d.flags & DS.INSIDE))
        assert dmap.dtype == np.uint32 and np.array_equal(dmap, want), (dims, d.box, d.weight, d.flags)
        n += 1
    assert n == 300


def test_the_twin_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    from volym_amd import scene
    for dims, vol, lab, d in _random_cases(9, 60):
        _, dmap = scene.distance_volume(vol, dims, d, labels=lab)
        _, _, solid = _solid(dims, vol, lab, d)
        sampling = [math.sqrt(d.weight[2]), math.sqrt(d.weight[1]), math.sqrt(d.weight[0])]
        if d.flags & DS.INSIDE:
            edt = ndimage.distance_transform_edt(np.pad(solid, 1), sampling=sampling)[1:-1, 1:-1, 1:-1]     # the mask padded by one texel of zeros
        elif solid.any():
            edt = ndimage.distance_transform_edt(~solid, sampling=sampling)
        else:
            assert (dmap == DS.NONE).all()
            continue
        assert np.array_equal(np.rint(edt ** 2).astype(np.uint32), dmap), (dims, d.box, d.weight, d.flags)


def test_the_closed_forms():
    from volym_amd import scene
    for name, (dims, vol, lab, d, closed) in DS.constructed().items():
        DS.check_closed(name, scene.distance_volume(vol, dims, d, labels=lab), closed)


def test_ceil_sqrt_is_exact():
    from volym_amd import scene
    v = np.concatenate([np.arange(0, 70000), np.array([k * k + e for k in range(250, 70000, 997) for e in (-1, 0, 1)])])
    want = [math.isqrt(int(x) - 1) + 1 if x else 0 for x in v.tolist()]
    assert scene.distance_ceil_sqrt(v).tolist() == want


# ---- the summary ----------------------------------------------------------------------------------------------------------------
def test_the_summary_is_the_map_and_the_bytes_recounted():
    """every field from the map and the bytes by plain loops over texels: counters, the first texel of the maximum, the nearest
    present texel per label, the histogram with an integer root; and the identities between the fields"""
    from volym_amd import scene
    seen = 0
    for dims, vol, lab, d in _random_cases(13, 60):
        summary, dmap = scene.distance_volume(vol, dims, d, labels=lab)
        b, l, solid = _solid(dims, vol, lab, d)
        (x0, y0, z0), _ = d.box
        n_finite, top, top_at, near, hist = 0, None, (0, 0, 0), {}, [0] * 256
        for (z, y, x), v in np.ndenumerate(dmap):
            v = int(v)
            if v == DS.NONE:
                continue
            n_finite += 1
            hist[min(math.isqrt(v - 1) + 1 if v else 0, 255)] += 1
            if top is None or v > top:
                top, top_at = v, (x + x0, y + y0, z + z0)
            if b[z, y, x] >= d.min_byte and (int(l[z, y, x]) not in near or v < near[int(l[z, y, x])][0]):
                near[int(l[z, y, x])] = (v, (x + x0, y + y0, z + z0))
        assert int(summary["n_solid"]) == int(solid.sum()) and int(summary["n_present"]) == int((b >= d.min_byte).sum())
        assert int(summary["n_finite"]) == n_finite == int(summary["hist"].sum())
        assert int(summary["max_d2"]) == (DS.NONE if top is None else top) and tuple(summary["max_at"].tolist()) == top_at
        assert summary["hist"].tolist() == hist
        for v in range(256):
            want = near.get(v, (DS.NONE, (0, 0, 0)))
            assert int(summary["near_d2"][v]) == want[0] and tuple(summary["near_at"][v].tolist()) == want[1], v
        inside = bool(d.flags & DS.INSIDE)
        if inside:
            assert n_finite == dmap.size
        else:
            for v in np.unique(l[solid]).tolist():                # every selected label with a solid texel is at distance 0
                assert int(summary["near_d2"][v]) == 0
                seen += 1
        again = scene.distance_map_summary(dmap, b, l, d)
        assert again.tobytes() == summary.tobytes()
    assert seen > 20


class _NoContext:
    """Host.set_cut's context when there is none"""

    def set_crop_box(self, *a):
        pass

    set_clip_plane = set_segment_visibility = set_crop_box


def test_n_solid_is_the_components_twins_under_every_cut():
    from tests import components_scenes as CS
    from volym_amd import scene
    cut_something = 0
    for which in (DS.scene_a, DS.scene_b):
        host = which()
        for turn, (step, box, plane, hidden) in enumerate(DS.CUTS):
            host.set_cut(_NoContext(), box, plane, hidden)
            for flags in (0, DS.INSIDE):
                for name, d in DS.requests(flags, turn):
                    summary, dmap = DS.expect(host, d)
                    c = scene.Components(d.box, 0, d.min_byte, d.select)
                    assert int(summary["n_solid"]) == int(CS.expect(host, c)[0]["n_solid"]), (step, name)
                    zeros = int((dmap == 0).sum())
                    assert zeros == (dmap.size - int(summary["n_solid"]) if flags else int(summary["n_solid"])), (step, name)
            whole = scene.Distance(dims=host.dims)
            cut_something += int(DS.expect(host, whole)[0]["n_solid"]) < int(DS.expect(host, whole.replace(flags=DS.UNCUT))[0]["n_solid"])
    assert cut_something >= 8


def test_the_empty_box_and_the_long_rows():
    from tests.test_gpu_crop_box import _ragged
    from volym_amd import scene
    summary, dmap = scene.distance_volume(np.zeros(8, np.uint8), (2, 2, 2), scene.Distance(((1, 1, 1), (1, 2, 2))))
    assert dmap.shape == (0, 0, 0) and summary.tobytes() == scene.empty_distance()[0].tobytes()
    assert int(summary["max_d2"]) == DS.NONE and (summary["near_d2"] == DS.NONE).all() and int(summary["hist"].sum()) == 0
    dims, vol, labels = _ragged()
    assert dims == DS.LONG_DIMS
    d = scene.Distance(DS.LONG_BOXES["97"], DS.INSIDE, 4, None, (1, 1, 4))
    summary, dmap = scene.distance_volume(vol, dims, d, labels=labels)             # fast enough for 97 x 80 x 71
    assert int(summary["n_solid"]) > 1000 and int(summary["max_d2"]) > 4 and int(summary["n_finite"]) == 97 * 80 * 71


# ---- the helpers ----------------------------------------------------------------------------------------------------------------
def test_distance_weights_and_summary():
    from volym_amd import scene
    assert scene.distance_weights((0.5, 0.5, 2.5)) == ((1, 1, 25), 0.5)
    assert scene.distance_weights((1, 1, 1)) == ((1, 1, 1), 1.0)
    assert scene.distance_weights((2.0, 0.25, 1.0)) == ((64, 1, 16), 0.25)
    for bad in ((1, 1, 1.5), (1, 9, 1), (0, 1, 1), (1, -1, 1), (1, 1)):
        with pytest.raises(ValueError):
            scene.distance_weights(bad)
    dims, vol, lab, d, closed = DS.constructed()["slabs weighted"]
    summary, _ = scene.distance_volume(vol, dims, d, labels=lab)
    s = scene.distance_summary(summary, 0.5)
    assert s["n_solid"] == 3 * 6 * 5 and s["clearance"][2] == {"d2": 49 * 25, "distance": 35 * 0.5, "at": (9, 0, 0)} and s["clearance"][1]["d2"] == 0
    assert s["max"] == 55 * 0.5 and s["max_at"] == (13, 0, 0)
    assert s["within"][0] == 3 * 6 * 5 and s["within"][4] == 3 * 6 * 5 and s["within"][5] == 4 * 6 * 5 and s["within"][254] == 14 * 6 * 5
    e = scene.distance_summary(scene.empty_distance()[0])
    assert e["max"] is None and e["max_d2"] is None and e["clearance"] == {} and e["within"][254] == 0
