"""The host side of fill between slices (no GPU): the layouts of its structs on both sides of ctypes and in C, what the checks refuse,
and the host twins scene.interpolate_volume and scene.interpolate_labels_volume pinned to an independent restatement -- a per-texel
loop over Python integers on small planes and scipy's Euclidean transform where scipy imports -- to closed forms (half-plane strips
with their ties, concentric discs, shapes disjoint in projection) and to a case built about the 64-bit comparison.
tests/test_gpu_interpolate.py compares the device with these twins.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import interpolate_scenes as IS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INTERPOLATE_LAYOUT = [("box", 0), ("flags", 24), ("min_byte", 28), ("select", 32), ("weight", 288), ("axis", 300), ("max_gap", 304), ("keys", 308)]
SUMMARY_LAYOUT = [("n_slices", 0), ("n_keys", 4), ("n_gaps", 8), ("n_gap_slices", 12), ("n_refused", 16), ("reserved", 20), ("n_shape", 24), ("n_inside", 32),
                  ("n_new", 40), ("n_stale", 48), ("slice", 56)]
SLICE_LAYOUT = [("kind", 0), ("key_lo", 4), ("key_hi", 8), ("count", 12)]
EDIT_LAYOUT = [("box", 0), ("flags", 24), ("min_byte", 28), ("max_byte", 32), ("to", 36), ("out", 292)]


def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Interpolate) == 820 and C.sizeof(_lib.InterpolateSummary) == 65592 == _lib.INTERPOLATE_SUMMARY_DTYPE.itemsize
    assert C.sizeof(_lib.InterpolateSlice) == 16 == _lib.INTERPOLATE_SLICE_DTYPE.itemsize and C.sizeof(_lib.InterpolateEdit) == 548
    for struct, layout in ((_lib.Interpolate, INTERPOLATE_LAYOUT), (_lib.InterpolateSummary, SUMMARY_LAYOUT), (_lib.InterpolateSlice, SLICE_LAYOUT),
                           (_lib.InterpolateEdit, EDIT_LAYOUT)):
        assert [(f, getattr(struct, f).offset) for f, _ in layout] == layout, struct
    assert [(f, _lib.INTERPOLATE_SUMMARY_DTYPE.fields[f][1]) for f, _ in SUMMARY_LAYOUT] == SUMMARY_LAYOUT
    consts = [_lib.INTERPOLATE_UNCUT, _lib.INTERPOLATE_KEYS, _lib.INTERPOLATE_SHAPE, _lib.INTERPOLATE_INSIDE, _lib.INTERPOLATE_GAP, _lib.INTERPOLATE_SLICE_OUTSIDE,
              _lib.INTERPOLATE_SLICE_KEY, _lib.INTERPOLATE_SLICE_GAP, _lib.INTERPOLATE_SLICE_REFUSED, _lib.INTERPOLATE_SLICES, _lib.INTERPOLATE_EDIT_UNCUT,
              _lib.INTERPOLATE_EDIT_DRY_RUN]
    assert consts == [IS.UNCUT, IS.KEYS, IS.SHAPE, IS.INSIDE, IS.GAP, IS.OUTSIDE_SLICE, IS.KEY_SLICE, IS.GAP_SLICE, IS.REFUSED_SLICE, 4096, IS.EDIT_UNCUT, IS.EDIT_DRY_RUN]
    assert _lib.INTERPOLATE_NONE == IS.NONE
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    names = ("VOLYM_INTERPOLATE_UNCUT", "VOLYM_INTERPOLATE_KEYS", "VOLYM_INTERPOLATE_SHAPE", "VOLYM_INTERPOLATE_INSIDE", "VOLYM_INTERPOLATE_GAP",
             "VOLYM_INTERPOLATE_SLICE_OUTSIDE", "VOLYM_INTERPOLATE_SLICE_KEY", "VOLYM_INTERPOLATE_SLICE_GAP", "VOLYM_INTERPOLATE_SLICE_REFUSED", "VOLYM_INTERPOLATE_SLICES",
             "VOLYM_INTERPOLATE_EDIT_UNCUT", "VOLYM_INTERPOLATE_EDIT_DRY_RUN")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu", sizeof(volym_interpolate), sizeof(struct volym_interpolate_summary), sizeof(struct volym_interpolate_slice), '
                   'sizeof(volym_interpolate_edit));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_interpolate, %s));\n' % f for f, _ in INTERPOLATE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_interpolate_summary, %s));\n' % f for f, _ in SUMMARY_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_interpolate_slice, %s));\n' % f for f, _ in SLICE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(volym_interpolate_edit, %s));\n' % f for f, _ in EDIT_LAYOUT) +
                   "".join('  printf(" %%u", (unsigned)%s);\n' % n for n in names) +
                   '  printf(" %u", (unsigned)(VOLYM_INTERPOLATE_NONE == 0xffffffffu));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [820, 65592, 16, 548] + [o for layout in (INTERPOLATE_LAYOUT, SUMMARY_LAYOUT, SLICE_LAYOUT, EDIT_LAYOUT) for _, o in layout] + consts + [1], out


def test_what_the_checks_refuse(volym_lib):
    """volym_interpolate_check and volym_interpolate_labels_check beside check_interpolate and check_interpolate_edit: pure host arithmetic"""
    from volym_amd import _lib, scene
    dims = (37, 22, 19)
    cdims = (C.c_uint32 * 3)(*dims)
    good = scene.Interpolate(dims=dims, min_byte=0, keys=(0, 4095), flags=IS.KEYS, weight=(64, 1, 64), axis=1, max_gap=7)
    assert volym_lib.volym_interpolate_check(C.byref(good.to_c()), cdims) == 0 and scene.check_interpolate(good, dims) is good
    assert volym_lib.volym_interpolate_check(C.byref(good.replace(box=((4, 4, 4), (4, 9, 9))).to_c()), cdims) == 0      # an empty box is valid
    bad = [dict(box=((0, 0, 0), (38, 22, 19))), dict(box=((5, 0, 0), (4, 22, 19))), dict(flags=4), dict(flags=7), dict(min_byte=256), dict(weight=(0, 1, 1)),
           dict(weight=(1, 65, 1)), dict(weight=(1, 1, 0)), dict(axis=3)]
    for kw in bad:
        q = good.replace(**kw)
        assert volym_lib.volym_interpolate_check(C.byref(q.to_c()), cdims) == _lib.E_INVALID, kw
        with pytest.raises(ValueError):
            scene.check_interpolate(q, dims)
    assert volym_lib.volym_interpolate_check(None, cdims) == _lib.E_INVALID and volym_lib.volym_interpolate_check(C.byref(good.to_c()), None) == _lib.E_INVALID
    with pytest.raises(ValueError):
        good.replace(keys=(4096,)).to_c()
    edit = scene.InterpolateEdit(dims=dims, to={0: 5}, out={5: 0}, window=(3, 255), flags=3)
    assert volym_lib.volym_interpolate_labels_check(C.byref(edit.to_c()), cdims) == 0 and scene.check_interpolate_edit(edit, dims) is edit
    for kw in (dict(box=((0, 0, 0), (37, 23, 19))), dict(box=((0, 9, 0), (37, 8, 19))), dict(flags=4), dict(window=(9, 8)), dict(window=(0, 256))):
        e = edit.replace(**kw)
        assert volym_lib.volym_interpolate_labels_check(C.byref(e.to_c()), cdims) == _lib.E_INVALID, kw
        with pytest.raises(ValueError):
            scene.check_interpolate_edit(e, dims)
    assert volym_lib.volym_interpolate_labels_check(None, cdims) == _lib.E_INVALID
    c = edit.to_c()
    assert list(c.to)[:6] == [5, 1, 2, 3, 4, 5] and list(c.out)[:6] == [0, 1, 2, 3, 4, 0] and (c.min_byte, c.max_byte, c.flags) == (3, 255, 3)
    c = good.to_c()
    assert c.keys[0] == 1 and c.keys[127] == 1 << 31 and sum(c.keys) == 1 + (1 << 31) and (c.axis, c.max_gap) == (1, 7)


# ---- the twin against an independent restatement ---------------------------------------------------------------------------------------
def _twin(shape, axis, weight=(1, 1, 1), **kw):
    """the twin's (summary, words [k, u, v], state [k, u, v]) of a shape [k, u, v] turned to `axis`"""
    from volym_amd import scene
    dims, vol, lab = IS.scene_of(shape, axis)
    q = scene.Interpolate(None, kw.pop("flags", 0), 0, IS.table(5), weight, axis, dims=dims, **kw)
    summary, words, state = scene.interpolate_volume(vol, dims, q, labels=lab)
    return summary, IS.slices_first(words.astype(np.int64), axis), IS.slices_first(state, axis)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_twin_is_the_rule_texel_by_texel(axis):
    """planes of at most 24 x 24: every word, every state byte and the whole summary from loops over Python integers"""
    rng = np.random.default_rng(5 + axis)
    noise = np.zeros((9, 11, 13), bool)
    for k in (1, 4, 5, 8):
        noise[k] = rng.random((11, 13)) < (0.15, 0.5, 0.8, 0.3)[k % 4]
    full = np.zeros((4, 5, 7), bool)
    full[0] = True
    full[3, 1:4, 2:5] = True
    cases = [("painted", IS.painted(17, 9, 12), (1, 4, 9), {}), ("noise", noise, (4, 1, 25), {}), ("noise, max_gap 2", noise, (1, 1, 1), dict(max_gap=2)),
             ("noise, KEYS", noise, (64, 9, 1), dict(flags=IS.KEYS, keys=(0, 2, 4, 5, 7))), ("a key that is all SHAPE", full, (1, 64, 4), {}),
             ("a 24 x 24 plane", IS.painted(17, 24, 24)[[2, 3, 4]] | np.roll(IS.painted(17, 24, 24)[[15, 3, 7]], 5, axis=2), (1, 1, 1), {})]
    for name, shape, weight, kw in cases:
        summary, words, state = _twin(shape, axis, weight, **kw)
        keys = None if "keys" not in kw else kw["keys"]
        w_want, s_want, kinds = IS.brute_force(shape, IS.plane_weights(weight, axis), keys, kw.get("max_gap", 0))
        assert np.array_equal(words, w_want), (name, np.argwhere(words != w_want)[:4].tolist())
        assert np.array_equal(state, s_want), (name, np.argwhere(state != s_want)[:4].tolist())
        n = shape.shape[0]
        rec = summary["slice"]
        assert rec["kind"][:n].tolist() == kinds and not rec["kind"][n:].any() and not rec["count"][n:].any(), name
        gap = np.array([k == IS.GAP_SLICE for k in kinds])
        at = [k for k in range(n) if kinds[k] == IS.KEY_SLICE]
        for k in range(n):
            lo = max([z for z in at if z <= k], default=None)
            hi = min([z for z in at if z >= k], default=None)
            if kinds[k] == IS.OUTSIDE_SLICE:
                want = (IS.NONE, IS.NONE, 0)
            elif kinds[k] == IS.KEY_SLICE:
                want = (k, k, int(shape[k].sum()))
            else:
                want = (lo, hi, int(((s_want[k] & IS.INSIDE) != 0).sum()) if kinds[k] == IS.GAP_SLICE else 0)
            assert (int(rec["key_lo"][k]), int(rec["key_hi"][k]), int(rec["count"][k])) == want, (name, k)
        runs = lambda kind: sum(1 for k in range(n) if kinds[k] == kind and kinds[k - 1] != kind)
        inside, was = (s_want[gap] & IS.INSIDE) != 0, (s_want[gap] & IS.SHAPE) != 0
        want = dict(n_slices=n, n_keys=len(at), n_gaps=runs(IS.GAP_SLICE), n_gap_slices=int(gap.sum()), n_refused=runs(IS.REFUSED_SLICE), reserved=0, n_shape=int(shape.sum()),
                    n_inside=int(inside.sum()), n_new=int((inside & ~was).sum()), n_stale=int((was & ~inside).sum()))
        assert {k: int(summary[k]) for k in want} == want, name


def test_the_planar_maps_are_scipys_transform():
    ndimage = pytest.importorskip("scipy.ndimage")
    shape = IS.painted()
    for axis in range(3):
        _, words, _ = _twin(shape, axis)
        for k in (2, 7, 8, 15):
            d_in = np.rint(ndimage.distance_transform_edt(np.pad(shape[k], 1)) ** 2).astype(np.int64)[1:-1, 1:-1]       # (the border counts as not SHAPE)
            d_out = np.rint(ndimage.distance_transform_edt(~shape[k]) ** 2).astype(np.int64)
            assert np.array_equal(words[k], np.where(shape[k], d_in << 1 | 1, d_out << 1)), (axis, k)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_half_plane_strips_and_their_ties(axis):
    c = IS.STRIP
    _, words, state = _twin(IS.strips(), axis)
    ties = 0
    for z in range(1, c["n"] - 1):
        a, b = c["n"] - 1 - z, z
        for v in range(c["nv"]):
            left, right = a * (c["p0"] - v), b * (v - c["p1"] + 1)
            ties += left == right
            assert bool(state[z, c["row"], v] & IS.INSIDE) == (left > right), (z, v)
            assert state[z, c["row"], v] & IS.GAP
    assert ties >= 1 and not state[4, c["row"], 16] & IS.INSIDE and state[4, c["row"], 15] & IS.INSIDE      # equality is outside


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_concentric_discs_and_disjoint_shapes(axis):
    summary, _, state = _twin(IS.discs(15, 5, 11, 41), axis)
    areas = [int(((state[z] & IS.INSIDE) != 0).sum()) for z in range(11)]
    assert all(x > y for x, y in zip(areas, areas[1:])), areas
    assert areas[0] > areas[5] > areas[10] and areas == summary["slice"]["count"][:11].tolist()
    # shapes that are disjoint in projection: nothing joins them.  Each shape only shrinks towards the other key, inside its own projection
    # (a texel that is SHAPE on neither key is never INSIDE), and where the shapes are thin against their distance nothing is INSIDE at all
    shape = IS.disjoint()
    summary, _, state = _twin(shape, axis)
    gap = (state & IS.GAP) != 0
    assert int(summary["n_gaps"]) == 1 and gap.sum() == 4 * 12 * 20
    inside = (state & IS.INSIDE) != 0
    for z in range(1, 5):
        assert not (inside[z] & ~(shape[0] | shape[5])).any() and not (inside[z] & shape[0] & (z > 2)).any() and not (inside[z] & shape[5] & (z < 3)).any(), z
    summary, _, state = _twin(IS.disjoint(True), axis)
    gap = (state & IS.GAP) != 0
    assert int(summary["n_gaps"]) == 1 and gap.sum() == 4 * 12 * 20 and int(summary["n_inside"]) == 0 and not (state[gap] & IS.INSIDE).any()


def test_a_case_about_the_64_bit_comparison():
    """a plane 200 wide, weight 64, a gap of 150 slices: a^2 D passes 2^32, and products wrapped to 32 bits decide otherwise"""
    from volym_amd import scene
    axis = 2
    dims, vol, lab = IS.scene_of(IS.wide(), axis)
    q = scene.Interpolate(None, 0, 0, IS.table(5), IS.wide_weight(axis), axis, dims=dims)
    summary, words, state = scene.interpolate_volume(vol, dims, q, labels=lab)
    w = IS.slices_first(words.astype(np.int64), axis)
    assert int(summary["n_gap_slices"]) == 150
    assert max(150 ** 2 * int(w[0].max() >> 1), 150 ** 2 * int(w[151].max() >> 1)) > 2 ** 32
    exact = IS.state_from_words(words, summary, axis, 0)
    got = IS.slices_first(state, axis) & (IS.GAP | IS.INSIDE)
    assert np.array_equal(got[1:151], exact[1:151]) and (got[1:151] & IS.GAP).all() and not exact[[0, 151]].any()
    wrapped = IS.state_from_words(words, summary, axis, 0, wrap=2 ** 32)
    assert (wrapped != exact).any()                              # the case discriminates


# ---- the edit's twin -------------------------------------------------------------------------------------------------------------------
def test_the_edits_twin_texel_by_texel():
    from volym_amd import scene
    dims, vol, lab = IS.edit_scene()
    nx, ny, nz = dims
    for case in IS.edit_cases(dims):
        snap = scene.interpolate_volume(vol, dims, case.interpolate, labels=lab)
        new, result = scene.interpolate_labels_volume(vol, dims, case.edit, lab, snap[2], case.interpolate.box)
        e = case.edit
        (x0, y0, z0), (x1, y1, z1) = e.box
        want = lab.reshape(nz, ny, nx).copy()
        changed, left, arrived, hull = 0, [0] * 256, [0] * 256, None
        for z in range(z0, z1):
            for y in range(y0, y1):
                for x in range(x0, x1):
                    st, l, b = int(snap[2][z, y, x]), int(want[z, y, x]), int(vol[x + nx * (y + ny * z)])
                    if not st & IS.GAP or not e.window[0] <= b <= e.window[1]:
                        continue
                    to = int(e.to[l]) if st & IS.INSIDE else int(e.out[l])
                    if to != l:
                        changed += 1
                        left[l] += 1
                        arrived[to] += 1
                        hull = (x, y, z, x + 1, y + 1, z + 1) if hull is None else tuple(min(p, q) for p, q in zip(hull[:3], (x, y, z))) + tuple(max(p, q) for p, q in zip(hull[3:], (x + 1, y + 1, z + 1)))
                        if not e.flags & IS.EDIT_DRY_RUN:
                            want[z, y, x] = to
        assert int(result["changed"]) == changed and result["left"].tolist() == left and result["arrived"].tolist() == arrived, case.name
        assert tuple(result["box"].tolist()) == (hull or (0,) * 6) and np.array_equal(new, want), case.name
    with pytest.raises(ValueError):
        scene.interpolate_labels_volume(vol, dims, IS.edit_cases(dims)[0].edit, lab, snap[2][1:], ((0, 0, 1), dims))
