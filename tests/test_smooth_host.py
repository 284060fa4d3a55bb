"""The smoothing without a GPU: the C struct and constants, volym_smooth_check against its twin in scene, the host twin
scene.smooth_volume against a plain triple loop over Python integers and a collections.Counter, the closed forms, and the conditions
tests/test_gpu_smooth.py relies on, asserted on the twin.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import relabel_scenes as RS
from tests import smooth_scenes as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

REQUEST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("radius", 36, 12), ("give", 48, 256), ("take", 304, 256)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_struct_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Smooth) == 560
    for f, off, size in REQUEST_LAYOUT:
        d = getattr(_lib.Smooth, f)
        assert (d.offset, d.size) == (off, size), f
    consts = [_lib.SMOOTH_UNCUT, _lib.SMOOTH_DRY_RUN, _lib.SMOOTH_MAX_RADIUS]
    assert consts == [1, 16, 3] and (_lib.SMOOTH_UNCUT, _lib.SMOOTH_DRY_RUN) == (_lib.RELABEL_UNCUT, _lib.RELABEL_DRY_RUN)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(volym_smooth), sizeof(struct volym_relabel_result));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_smooth, %s));\n' % f for f, _, _ in REQUEST_LAYOUT) +
                   '  printf(" %d %d %u", VOLYM_SMOOTH_UNCUT, VOLYM_SMOOTH_DRY_RUN, VOLYM_SMOOTH_MAX_RADIUS);\n'
                   '  printf(" %d %d", VOLYM_SMOOTH_UNCUT == VOLYM_RELABEL_UNCUT, VOLYM_SMOOTH_DRY_RUN == VOLYM_RELABEL_DRY_RUN);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [560, 4128] + [o for _, o, _ in REQUEST_LAYOUT] + consts + [1, 1], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_smooth_labels", "volym_smooth_check"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert callable(demo.GpuContext.smooth_labels)
    for name in ("smooth", "smooth_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Smooth", "check_smooth", "smooth_volume", "smooth_table"):
        assert callable(getattr(scene, name))
    assert "each an undo step" in " ".join(demo.Simple.smooth.__doc__.lower().split())
    header = " ".join(open(os.path.join(ROOT, "include", "volym_hip.h")).read().split())
    section = header[header.index("--- smooth:"):header.index("int volym_smooth_check(")]
    assert "cast no vote" in section and "has no forward for this call" in section and "writes nothing" in section


def _check_rows():
    """(name, request, dims, valid)"""
    from volym_amd import scene
    d = (9, 7, 5)
    whole = ((0, 0, 0), d)

    def F(radius=(1, 1, 1), **kw):
        kw.setdefault("box", whole)
        return scene.Smooth(radius, **kw)

    rows = [("radius 1", F(), d, True), ("empty box", F(box=((3, 0, 0), (3, 7, 5))), d, True), ("radius 3", F((3, 3, 3)), d, True), ("in slices", F((1, 1, 0)), d, True),
            ("one axis", F((0, 0, 2)), d, True), ("both flags", F(flags=17), d, True), ("flag 2", F(flags=2), d, False), ("flag 32", F(flags=32), d, False),
            ("flag 2^31", F(flags=1 << 31), d, False), ("window 0..0", F(window=(0, 0)), d, True), ("window 7..6", F(window=(7, 6)), d, False),
            ("window 0..256", F(window=(0, 256)), d, False), ("all radii 0", F((0, 0, 0)), d, False), ("nothing gives", F(give=np.zeros(256)), d, True),
            ("nothing takes", F(take=np.zeros(256)), d, True),
            ("the largest volume", F(box=((0, 0, 0), (4096, 4096, 4096))), (4096, 4096, 4096), True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, F(box=((0, 0, 0), tuple(hi))), d, False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, F(box=(tuple(lo), tuple(hi))), d, False))
        for v in (4, 2 ** 32 - 1):
            r = [1, 1, 1]; r[a] = v
            rows.append(("radius %d on axis %d" % (v, a), F(tuple(r)), d, False))
    return rows


def test_the_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    for name, s, dims, valid in _check_rows():
        cd = (C.c_uint32 * 3)(*dims)
        rc = volym_lib.volym_smooth_check(C.byref(s.to_c()), cd)
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_smooth(s, dims) is s, name
        else:
            with pytest.raises(ValueError):
                scene.check_smooth(s, dims)
    one = scene.Smooth(1, dims=(1, 1, 1))
    assert volym_lib.volym_smooth_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_smooth_check(C.byref(one.to_c()), None) == E_INVALID
    with pytest.raises(ValueError):
        scene.Smooth(1)                                                 # no box and no dims
    with pytest.raises(ValueError):
        scene.Smooth((1, 1), dims=(2, 2, 2)).to_c()
    with pytest.raises(ValueError):
        scene.Smooth(1, give=np.zeros(255), dims=(2, 2, 2)).to_c()
    with pytest.raises(ValueError):
        scene.smooth_table([256])


# ---- the twin against the plain loop --------------------------------------------------------------------------------------------
def _same(dims, r, vol, labels, uncut=None):
    from volym_amd import scene
    new, res = scene.smooth_volume(vol, dims, r, labels, uncut=uncut)
    read = uncut if (r.flags & 1 and uncut is not None) else vol
    want, changed, left, arrived, hull = SS.plain_smooth(read, dims, r, labels)
    assert np.array_equal(new.ravel(), want), (r.radius, r.flags)
    assert int(res["changed"]) == changed == int(res["left"].sum()) == int(res["arrived"].sum())
    assert {l: int(v) for l, v in enumerate(res["left"]) if v} == dict(left) and {l: int(v) for l, v in enumerate(res["arrived"]) if v} == dict(arrived)
    assert tuple(int(v) for v in res["box"]) == (hull or (0, 0, 0, 0, 0, 0))
    if r.flags & 16:
        assert np.array_equal(new.ravel(), np.asarray(labels).ravel())
    return changed


@pytest.mark.parametrize("dims", SS.SMALL_DIMS)
def test_the_twin_is_the_plain_loop_on_small_volumes_for_every_flag_and_radius(dims):
    host = SS.scene_small(dims)
    cut = np.where(np.arange(host.vol.size) % 3 == 0, 0, host.vol).astype(np.uint8)        # the scene bytes as a cut would leave them
    total = 0
    for name, r in SS.small_requests(dims):
        total += _same(dims, r, cut, host.labels, uncut=host.vol)
    assert total > 1000


def test_the_twin_is_the_plain_loop_on_scene_a_for_every_case():
    host = RS.scene_a()
    for case in SS.cases():
        changed = _same(host.dims, case.smooth, host.vol, host.labels, uncut=host.vol)
        assert (changed >= 20) or "a" in case.few, (case.name, changed)


# ---- the closed forms -----------------------------------------------------------------------------------------------------------
def _run(dims, labels, radius, **kw):
    from volym_amd import scene
    lab = np.asarray(labels, np.uint8)
    new, res = scene.smooth_volume(np.full(lab.size, 9, np.uint8), dims, scene.Smooth(radius, dims=dims, **kw), lab.ravel())
    return new, res


RADII = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 1, 0), (3, 0, 0), (0, 2, 1)]


@pytest.mark.parametrize("radius", RADII)
def test_a_uniform_volume_and_a_flat_interface_are_fixed_points(radius):
    dims = (9, 8, 7)
    new, res = _run(dims, np.full(9 * 8 * 7, 5), radius)
    assert int(res["changed"]) == 0 and (new == 5).all()
    for axis in range(3):
        lab = np.zeros((7, 8, 9), np.uint8)
        half = [slice(None)] * 3
        half[axis] = slice(3, None)
        lab[tuple(half)] = 200
        new, res = _run(dims, lab, radius)
        assert int(res["changed"]) == 0 and np.array_equal(new, lab), axis


def test_a_lone_texel_becomes_the_sea_in_the_interior_and_at_a_corner_unless_take_leaves_the_sea_out():
    dims = (6, 5, 4)
    for at in ((2, 2, 2), (0, 0, 0), (3, 4, 5)):                       # [z, y, x]: the interior (1 vote to 26) and two corners (1 to 7)
        lab = np.full((4, 5, 6), 3, np.uint8)
        lab[at] = 8
        new, res = _run(dims, lab, 1)
        assert int(res["changed"]) == 1 and (new == 3).all() and int(res["left"][8]) == 1 and int(res["arrived"][3]) == 1
        assert tuple(res["box"]) == (at[2], at[1], at[0], at[2] + 1, at[1] + 1, at[0] + 1)
        new, res = _run(dims, lab, 1, take=SS.but(3))
        assert int(res["changed"]) == 0 and np.array_equal(new, lab)


def test_a_checkerboard_at_radius_1_inverts_in_the_interior():
    dims = (7, 6, 5)
    z, y, x = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    lab = np.where((x + y + z) % 2 == 0, 4, 9).astype(np.uint8)
    new, res = _run(dims, lab, 1)
    inner = (slice(1, -1),) * 3
    assert np.array_equal(new[inner], (13 - lab)[inner])               # 13 votes to 14: every interior texel flips
    assert int(res["changed"]) >= 5 * 4 * 3


def test_the_ties():
    a, b, c = 7, 3, 5
    # a row `a b` at the volume's edge with radius (1, 0, 0): one vote each, the own label keeps the tie
    new, _ = _run((2, 1, 1), [a, b], (1, 0, 0))
    assert new.ravel().tolist() == [a, b]
    # `b b a c c` with radius (2, 0, 0): a has 1, b and c have 2 each: the smallest of them
    new, _ = _run((5, 1, 1), [b, b, a, c, c], (2, 0, 0))
    assert new.ravel().tolist()[2] == min(b, c)
    new, _ = _run((5, 1, 1), [c, c, a, b, b], (2, 0, 0))
    assert new.ravel().tolist()[2] == min(b, c)
    # `c a b` with radius (1, 0, 0): one vote each, a stays
    new, _ = _run((3, 1, 1), [c, a, b], (1, 0, 0))
    assert new.ravel().tolist()[1] == a


def test_a_radius_that_covers_the_volume_makes_every_giving_texel_the_global_mode():
    rng = np.random.default_rng(11)
    lab = rng.choice([1, 2, 6], 4 * 3 * 4, p=[0.5, 0.3, 0.2]).astype(np.uint8)
    mode = int(np.bincount(lab).argmax())
    assert np.bincount(lab)[mode] > np.sort(np.bincount(lab))[-2]       # (no tie for the mode)
    new, res = _run((4, 3, 4), lab, 3, give=SS.table(2, mode))
    want = np.where(lab == 2, mode, lab)
    assert np.array_equal(new.ravel(), want) and int(res["changed"]) == int((lab == 2).sum())
    assert int(res["left"].sum()) == int(res["arrived"].sum()) == int(res["changed"])


# ---- what the device tests rely on ----------------------------------------------------------------------------------------------
def test_the_pinned_counts():
    from volym_amd import scene
    for (which, radius), texels in SS.TEXELS.items():
        host = SS.SCENES[which]()
        new, res = scene.smooth_volume(host.vol, host.dims, scene.Smooth(radius, dims=host.dims), host.labels)
        assert int(res["changed"]) == texels, (which, radius)
        if (which, radius) in SS.LINEAR_CHUNKS:
            chunks = -(-host.labels.size // 16)
            assert (scene.label_chunks_changed(host.dims, host.labels, new, False), chunks) == SS.LINEAR_CHUNKS[which, radius]


@pytest.mark.parametrize("which", list(SS.SCENES))
def test_every_case_that_is_not_marked_changes_at_least_20_texels(which):
    host = SS.SCENES[which]()
    for case in SS.cases(host.dims):
        changed = int(SS.expect(host, case)[1]["changed"])
        assert changed >= 20 or which in case.few, (which, case.name, changed)
        assert changed < 20 or which not in case.few, (which, case.name, changed)


def test_the_ragged_cases_change_texels_of_two_rows_within_one_linear_chunk():
    host = RS.scene_ragged()
    by_name = {c.name: c for c in SS.cases(host.dims)}
    for name in ("joint, radius 2", "joint, radius 3", "joint, radius 0, 2, 1", "only 1 gives, radius 2"):
        new, _ = SS.expect(host, by_name[name])
        assert RS.wrapping_chunks(host.dims, host.labels, new) >= 2, name
    noisy = SS.scene_overflow()
    new, _ = SS.expect(noisy, by_name["joint, radius 1"])
    assert RS.wrapping_chunks(noisy.dims, noisy.labels, new) > 1000


def test_the_overflow_case_changes_most_chunks_and_the_small_case_few():
    from volym_amd import scene
    for bricked in (False, True):
        items = scene.relabel_slab_items(SS.DIMS, None, bricked)
        for which, few in (("a", True), ("b", False)):
            host = SS.SCENES[which]()
            new, _ = SS.expect(host, SS.cases()[0])
            records = scene.label_chunks_changed(host.dims, host.labels, new, bricked)
            assert (records < 0.1 * items) if few else (records > 0.9 * items), (which, bricked, records, items)
        # scene B has fewer items than the staging area's floor; the same kind of labels over the ragged volume overruns it
        host = SS.scene_overflow()
        items = scene.relabel_slab_items(host.dims, None, bricked)
        new, res = SS.expect(host, SS.cases(host.dims)[0])
        records = scene.label_chunks_changed(host.dims, host.labels, new, bricked)
        assert records > 0.9 * items and records > 2 * SS.first_capacity(items) and int(res["changed"]) > 300000, (bricked, records, items)
        ragged = SS.SCENES["ragged"]()
        new, _ = SS.expect(ragged, SS.cases(ragged.dims)[0])
        assert scene.label_chunks_changed(ragged.dims, ragged.labels, new, bricked) < SS.first_capacity(items) // 4
