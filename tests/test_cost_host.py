"""The cost pass and the spread without a GPU: the C structs and constants, volym_cost_check and volym_spread_check against the
Python checks, the sweeping host twin scene.cost_volume against a heap-based search per label and against a restatement of the
device's schedule (tiles relaxed in a random order against halos of mixed age until nothing is marked), every summary field recounted
by loops, the constructed scenes against closed forms and their premises, a truncated pass against the untruncated one,
scene.spread_volume against a per-texel loop and against scene.flood_volume handed the cost map.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cost_scenes as CS
from tests import geodesic_scenes as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1

COST_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("seed", 36, 256), ("through", 292, 256), ("max_cost", 548, 4),
               ("n_points", 552, 4), ("points", 556, 768), ("step_cost", 1324, 4), ("contrast_cost", 1328, 4), ("hist_shift", 1332, 4)]
SUMMARY_LAYOUT = [("n_seed", 0, 8), ("n_medium", 8, 8), ("n_reached", 16, 8), ("max_cost", 24, 4), ("max_at", 28, 12), ("cell", 40, 2048), ("cell_medium", 2088, 2048),
                  ("hist", 4136, 2048)]
SITE_LAYOUT = [("cost", 0, 4), ("label", 4, 4)]
SPREAD_LAYOUT = [("box", 0, 24), ("flags", 24, 4), ("min_byte", 28, 4), ("max_byte", 32, 4), ("give", 36, 256), ("take", 292, 256), ("to", 548, 256), ("cost_lo", 804, 4),
                 ("cost_hi", 808, 4)]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Cost) == 1336 and C.sizeof(_lib.CostSummary) == 6184 == _lib.COST_SUMMARY_DTYPE.itemsize
    assert C.sizeof(_lib.CostSite) == 8 and C.sizeof(_lib.Spread) == 812
    for struct, dtype, layout in ((_lib.Cost, None, COST_LAYOUT), (_lib.CostSummary, _lib.COST_SUMMARY_DTYPE, SUMMARY_LAYOUT), (_lib.CostSite, None, SITE_LAYOUT),
                                  (_lib.Spread, None, SPREAD_LAYOUT)):
        for f, off, size in layout:
            d = getattr(struct, f)
            assert (d.offset, d.size) == (off, size), f
            if dtype is not None:
                assert dtype.fields[f][1] == off and dtype.fields[f][0].itemsize == size, f
    consts = [_lib.COST_UNCUT, _lib.COST_POINTS_MAX, _lib.COST_MAX, _lib.COST_STEP_MAX, _lib.COST_BOX_MAX, _lib.COST_NONE, _lib.COST_HIST_SHIFT_MAX, _lib.SPREAD_UNCUT,
              _lib.SPREAD_DRY_RUN]
    assert consts == [1, 64, 2 ** 24 - 3, 65280, 2 ** 31 - 2, 0xFFFFFFFF, 16, 1, 2]
    assert (CS.NONE, CS.COST_MAX, CS.UNCUT, CS.SPREAD_UNCUT, CS.SPREAD_DRY_RUN) == (_lib.COST_NONE, _lib.COST_MAX, _lib.COST_UNCUT, _lib.SPREAD_UNCUT, _lib.SPREAD_DRY_RUN)
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu", sizeof(volym_cost), sizeof(struct volym_cost_summary), sizeof(struct volym_cost_site), sizeof(volym_spread));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_cost, %s));\n' % f for f, _, _ in COST_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_cost_summary, %s));\n' % f for f, _, _ in SUMMARY_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(struct volym_cost_site, %s));\n' % f for f, _, _ in SITE_LAYOUT) +
                   "".join('  printf(" %%zu", offsetof(volym_spread, %s));\n' % f for f, _, _ in SPREAD_LAYOUT) +
                   '  printf(" %d %u %u %u %u %u %u %d %d %d", VOLYM_COST_UNCUT, VOLYM_COST_POINTS_MAX, VOLYM_COST_MAX, VOLYM_COST_STEP_MAX, VOLYM_COST_BOX_MAX, VOLYM_COST_NONE,'
                   ' VOLYM_COST_HIST_SHIFT_MAX, VOLYM_SPREAD_UNCUT, VOLYM_SPREAD_DRY_RUN, VOLYM_ABI_VERSION);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [1336, 6184, 8, 812] + [o for layout in (COST_LAYOUT, SUMMARY_LAYOUT, SITE_LAYOUT, SPREAD_LAYOUT) for _, o, _ in layout] + consts + [2], out


def test_library_exports_the_calls_and_python_has_its_faces(volym_lib):
    from volym_amd import _lib, demo, scene
    for name in ("volym_cost_pass", "volym_cost_check", "volym_read_cost", "volym_read_cost_map", "volym_cost_at", "volym_cost_device_ptr", "volym_cost_map_device_ptr",
                 "volym_spread_labels", "volym_spread_check"):
        assert hasattr(volym_lib, name) and name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2
    for name in ("cost_pass", "read_cost", "read_cost_map", "cost_at", "spread_labels"):
        assert callable(getattr(demo.GpuContext, name))
    for name in ("grow_from_seeds", "cost_reach", "smart_wand_at"):
        assert callable(getattr(demo.Simple, name))
    for name in ("Cost", "check_cost", "empty_cost", "cost_volume", "cost_summary", "Spread", "check_spread", "spread_volume"):
        assert callable(getattr(scene, name))
    # the flood's check goes on refusing flag 4: the spread is a call of its own
    assert volym_lib.volym_flood_check(C.byref(scene.Flood(dims=(2, 2, 2), flags=4).to_c()), (C.c_uint32 * 3)(2, 2, 2)) == E_INVALID


def _cost_rows():
    """(name, request, valid) in a volume of 9 x 7 x 5: every refusal the header spells out, and the last valid value before each"""
    from volym_amd import scene
    d = (9, 7, 5)
    Q = scene.Cost
    whole = ((0, 0, 0), d)
    inner = ((2, 1, 1), (7, 6, 4))
    rows = [("whole", Q(whole), True), ("empty on x", Q(((3, 0, 0), (3, 7, 5))), True), ("empty at the far corner", Q((d, d)), True), ("one texel", Q(((8, 6, 4), d)), True),
            ("uncut", Q(whole, 1), True), ("flag 2", Q(whole, 2), False), ("flag 3", Q(whole, 3), False), ("flag 2^31", Q(whole, 1 << 31), False),
            ("window 0..0", Q(whole, window=(0, 0)), True), ("window 255..255", Q(whole, window=(255, 255)), True), ("window 9..8", Q(whole, window=(9, 8)), False),
            ("window 0..256", Q(whole, window=(0, 256)), False), ("window 256..256", Q(whole, window=(256, 256)), False),
            ("step 0", Q(whole, step=0), False), ("step 1", Q(whole, step=1), True), ("step 255", Q(whole, step=255), True), ("step 256", Q(whole, step=256), False),
            ("step 2^32 - 1", Q(whole, step=2 ** 32 - 1), False),
            ("contrast 0", Q(whole, contrast=0), True), ("contrast 255", Q(whole, contrast=255), True), ("contrast 256", Q(whole, contrast=256), False),
            ("a limit of 1", Q(whole, max_cost=1), True), ("the largest limit", Q(whole, max_cost=2 ** 24 - 3), True), ("a limit too large", Q(whole, max_cost=2 ** 24 - 2), False),
            ("limit 2^32 - 1", Q(whole, max_cost=2 ** 32 - 1), False),
            ("shift 16", Q(whole, hist_shift=16), True), ("shift 17", Q(whole, hist_shift=17), False), ("shift 2^31", Q(whole, hist_shift=2 ** 31), False),
            ("no table set", Q(whole, seed=np.zeros(256), through=np.zeros(256)), True),
            ("a point", Q(whole, points=[(8, 6, 4)]), True), ("a duplicate point", Q(whole, points=[(1, 2, 3), (1, 2, 3)]), True),
            ("64 points", Q(whole, points=[(k % 9, k % 7, k % 5) for k in range(64)]), True), ("65 points", Q(whole, points=[(k % 9, k % 7, k % 5) for k in range(65)]), False),
            ("a point in the inner box", Q(inner, points=[(2, 1, 1), (6, 5, 3)]), True), ("a point in an empty box", Q(((3, 0, 0), (3, 7, 5)), points=[(3, 0, 0)]), False)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, Q(((0, 0, 0), tuple(hi))), False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, Q((tuple(lo), tuple(hi))), False))
        p = [2, 1, 1]; p[a] -= 1
        rows.append(("a point below the box on axis %d" % a, Q(inner, points=[(3, 3, 3), tuple(p)]), False))
        p = [6, 5, 3]; p[a] += 1
        rows.append(("a point at the box's hi on axis %d" % a, Q(inner, points=[tuple(p)]), False))
    return d, rows


def test_the_cost_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    dims, rows = _cost_rows()
    for name, q, valid in rows:
        rc = volym_lib.volym_cost_check(C.byref(q.to_c()), (C.c_uint32 * 3)(*dims))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_cost(q, dims) is q, name
        else:
            with pytest.raises(ValueError):
                scene.check_cost(q, dims)
    big = (4096, 4096, 4096)                                       # the over-large box: one texel more than 2^31 - 2 allows
    for box, valid in ((((0, 0, 0), (4096, 4096, 127)), True), (((0, 0, 0), (4096, 4096, 128)), False), (((0, 0, 0), (2048, 1024, 1024)), False),
                       (((1, 0, 0), (2048, 1024, 1024)), True)):
        q = scene.Cost(box)
        assert (volym_lib.volym_cost_check(C.byref(q.to_c()), (C.c_uint32 * 3)(*big)) == 0) == valid, box
        if not valid:
            with pytest.raises(ValueError):
                scene.check_cost(q, big)
    assert volym_lib.volym_cost_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_cost_check(C.byref(scene.Cost(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    for bad in (dict(max_cost=2 ** 32), dict(step=-1), dict(contrast=2 ** 32), dict(hist_shift=-1), dict(window=(0, -1)), dict(seed=np.full(256, 256)),
                dict(through=np.zeros(255)), dict(points=[(1, 2)]), dict(points=[(0, 0, -1)])):
        with pytest.raises(ValueError):
            scene.Cost(dims=(2, 2, 2), **bad).to_c()


def test_the_spread_check_and_its_twin_give_the_same_verdict(volym_lib):
    from volym_amd import scene
    d = (9, 7, 5)
    S = scene.Spread
    whole = ((0, 0, 0), d)
    rows = [("whole", S(whole), True), ("empty on x", S(((3, 0, 0), (3, 7, 5))), True), ("empty at the far corner", S((d, d)), True), ("one texel", S(((8, 6, 4), d)), True),
            ("uncut", S(whole, 1), True), ("dry run", S(whole, 2), True), ("both flags", S(whole, 3), True), ("flag 4", S(whole, 4), False),
            ("flag 16", S(whole, 16), False), ("flag 2^31", S(whole, 1 << 31), False),
            ("window 0..0", S(whole, window=(0, 0)), True), ("window 255..255", S(whole, window=(255, 255)), True), ("window 9..8", S(whole, window=(9, 8)), False),
            ("window 0..256", S(whole, window=(0, 256)), False), ("window 256..256", S(whole, window=(256, 256)), False),
            ("band 0..0", S(whole, cost=(0, 0)), True), ("band 7..7", S(whole, cost=(7, 7)), True), ("band 8..7", S(whole, cost=(8, 7)), False),
            ("band to 2^32 - 1", S(whole, cost=(0, 2 ** 32 - 1)), True), ("band 2^32 - 1 .. 0", S(whole, cost=(2 ** 32 - 1, 0)), False),
            ("no label gives or takes", S(whole, give=np.zeros(256), take=np.zeros(256)), True), ("to renames", S(whole, to={0: 9, 3: 0}), True)]
    for a in range(3):
        hi = list(d); hi[a] += 1
        rows.append(("hi beyond the volume on axis %d" % a, S(((0, 0, 0), tuple(hi))), False))
        lo = [0, 0, 0]; lo[a] = 4; hi = list(d); hi[a] = 3
        rows.append(("lo above hi on axis %d" % a, S((tuple(lo), tuple(hi))), False))
    for name, s, valid in rows:
        rc = volym_lib.volym_spread_check(C.byref(s.to_c()), (C.c_uint32 * 3)(*d))
        assert (rc == 0) == valid and rc in (0, E_INVALID), (name, rc)
        if valid:
            assert scene.check_spread(s, d) is s, name
        else:
            with pytest.raises(ValueError):
                scene.check_spread(s, d)
    assert volym_lib.volym_spread_check(None, (C.c_uint32 * 3)(1, 1, 1)) == E_INVALID
    assert volym_lib.volym_spread_check(C.byref(scene.Spread(dims=(1, 1, 1)).to_c()), None) == E_INVALID
    for bad in (dict(cost=(0, 2 ** 32)), dict(window=(0, -1)), dict(give=np.full(256, 256)), dict(take=np.zeros(255)), dict(to=np.full(256, 256))):
        with pytest.raises(ValueError):
            scene.Spread(dims=(2, 2, 2), **bad).to_c()
    assert scene.Spread(dims=(2, 2, 2), to={0: 9}).to.tolist() == [9] + list(range(1, 256))


# ---- the twin against the rule restated ------------------------------------------------------------------------------------------------
def _random_boxes(n):
    """n random scenes up to 7^3: (dims, vol, labels, scene.Cost) with densities of matter from empty to full, labels 0..4, the
    contrasts 0, 1, 17 and 255 and limits set and unset in turn.  The bytes of the matter come from few values, so that chains of
    unequal step counts tie in cost."""
    from volym_amd import scene
    rng = np.random.default_rng(11)
    out = []
    for k in range(n):
        dims = tuple(int(v) for v in rng.integers(1, 8, 3))
        size = dims[0] * dims[1] * dims[2]
        share = (0.0, 0.3, 0.55, 0.7, 0.85, 1.0)[k % 6]
        matter = rng.choice([100, 101, 102, 104, 180, 255], size) if k % 2 else rng.integers(100, 256, size)
        vol = np.where(rng.random(size) < share, matter, rng.integers(0, 100, size)).astype(np.uint8)
        lab = rng.choice([0, 0, 0, 0, 0, 0, 1, 2, 3, 4], size).astype(np.uint8)
        pts = [tuple(int(rng.integers(0, d)) for d in dims) for _ in range(k % 3)]
        contrast = (0, 1, 17, 255)[k % 4]
        step = (1, 2, 1, 7, 255)[k % 5]
        limit = (0, step * 2 + contrast * 3, 0, step * 5 + contrast * 40)[(k // 4) % 4]
        q = scene.Cost(None, 0, (100, 255), GS.table(1, 2, 3) if k % 5 else GS.table(2, 4), GS.table(0, 4) if k % 4 else GS.table(0, 1), step, contrast, limit, pts, k % 17,
                       dims=dims)
        out.append((dims, vol, lab, q))
    return out


def _box_bytes(dims, vol, lab):
    return vol.reshape(dims[::-1]), lab.reshape(dims[::-1])


def _signed(keys):
    return np.where(keys == np.uint32(CS.NONE), -1, keys.astype(np.int64))


def test_the_twin_equals_a_heap_search_per_label_on_random_boxes():
    from volym_amd import scene
    ties = reached = limited = 0
    boxes = _random_boxes(320)
    assert {q.contrast for _, _, _, q in boxes} == {0, 1, 17, 255} and {bool(q.max_cost) for _, _, _, q in boxes} == {False, True}
    for k, (dims, vol, lab, q) in enumerate(boxes):
        summary, keys = scene.cost_volume(vol, dims, q, labels=lab)
        b, l = _box_bytes(dims, vol, lab)
        seed, medium = CS.predicates(b, l, q)
        want, t = CS.dijkstra(seed, medium, l, b, q)
        assert np.array_equal(_signed(keys), want), (k, dims)
        ties += t
        reached += int(summary["n_reached"])
        limited += int(summary["n_reached"]) < int(summary["n_seed"]) + int(summary["n_medium"]) and bool(q.max_cost)
    assert len(boxes) >= 300 and ties > 100 and reached > 5000 and limited > 20, (ties, reached, limited)


def test_the_twin_equals_the_schedule_of_the_device_on_random_boxes():
    """tiles of 3 x 2 x 2, 2 x 3 x 1 and 4 x 4 x 4 in turn, relaxed in a random order against halos of mixed age, from every tile and
    from the tiles the init kernel marks in turn"""
    from volym_amd import scene
    rng = np.random.default_rng(5)
    boxes = _random_boxes(320)[3::5]
    assert len(boxes) >= 60
    again = 0
    for k, (dims, vol, lab, q) in enumerate(boxes):
        _, keys = scene.cost_volume(vol, dims, q, labels=lab)
        b, l = _box_bytes(dims, vol, lab)
        seed, medium = CS.predicates(b, l, q)
        got, lowered_in = CS.scheduled(seed, medium, l, b, q, ((3, 2, 2), (2, 3, 1), (4, 4, 4))[k % 3], rng, from_seeds=bool(k % 2))
        assert np.array_equal(_signed(keys), got), (k, dims)
        again += sum(len(r) > 1 for r in lowered_in.values())
    assert again > 20                                               # tiles were lowered in more rounds than one


def test_every_summary_field_recounted_by_loops():
    from volym_amd import scene
    host = CS.scene_a()
    shifts = set()
    for dims, vol, lab, q in _random_boxes(60)[::3] + [(CS.DIMS, host.vol, host.labels, q) for _, q in CS.requests()[:4]]:
        summary, keys = scene.cost_volume(vol, dims, q, labels=lab)
        if keys.size == 0:
            continue
        lo, hi = q.box
        sub = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        b, l = _box_bytes(dims, vol, lab)
        seed, medium = CS.predicates(b[sub], l[sub], q)
        want = CS.summary_by_loops(keys, seed, medium, lo, q.hist_shift)
        for f in ("n_seed", "n_medium", "n_reached", "max_cost"):
            assert int(summary[f]) == want[f], (f, dims)
        for f in ("max_at", "cell", "cell_medium", "hist"):
            assert summary[f].tolist() == want[f], (f, dims)
        shifts.add(q.hist_shift)
    assert len(shifts) > 5
    names = scene.cost_summary(scene.cost_volume(host.vol, host.dims, CS.requests()[0][1], labels=host.labels)[0], {1: "one"})
    assert names["n_reached"] > 0 and all(set(v) == {"label", "texels", "grown"} for v in names["cells"].values())
    assert scene.cost_summary(scene.empty_cost()[0])["max_cost"] is None


# ---- the constructed scenes ------------------------------------------------------------------------------------------------------------
def test_unit_steps_give_the_geodesic_map_and_steps_of_c_its_multiple():
    """scene 1: contrast_cost 0 and step_cost 1 is the geodesic twin's map, byte for byte; step_cost 3 that map with the steps tripled"""
    from volym_amd import scene
    cases = CS.unit_cases()
    assert len(cases) >= 20
    for name, dims, vol, lab, g, closed in cases:
        gs, gk = scene.geodesic_volume(vol, dims, g, labels=lab)
        cs, ck = scene.cost_volume(vol, dims, CS.unit_request(g), labels=lab)
        assert ck.tobytes() == gk.tobytes() and ck.shape == gk.shape, name
        assert cs.tobytes() == gs.tobytes(), name                  # (the summaries are laid out alike, and hist_shift is 0)
        CS.check_closed(name, (cs, ck), closed)
        _, c3 = scene.cost_volume(vol, dims, CS.unit_request(g, 3), labels=lab)
        assert np.array_equal(c3, CS.times(gk, 3)), name


def test_the_constructed_scenes_have_their_closed_forms():
    from volym_amd import scene
    made = CS.constructed()
    got = {name: scene.cost_volume(vol, dims, q, labels=lab) for name, (dims, vol, lab, q, closed) in made.items()}
    for name, (dims, vol, lab, q, closed) in made.items():
        CS.check_closed(name, got[name], closed)
    ext = CS.tile()
    # scene 3, the ridge: in steps the target is four away, over the ridge; in cost it is the flat detour, which crosses four tile faces or more
    dims, vol, lab, q, closed = made["ridge and detour"]
    (t, (cost, _)), = closed["at"].items()
    b = vol.reshape(dims[::-1])
    detour = closed["detour"]
    assert all(sum(abs(u[i] - v[i]) for i in range(3)) == 1 for u, v in zip(detour, detour[1:])) and len({int(b[z, y, x]) for x, y, z in detour}) == 1
    assert cost == q.step * (len(detour) - 1) < closed["over"] and CS.faces_crossed(detour) >= 4
    _, steps = scene.geodesic_volume(vol, dims, scene.Geodesic(q.box, 0, q.window, q.seed, q.through, 0, q.points), labels=lab)
    assert int(steps[t[2], t[1], t[0]]) >> 8 == 4 and q.step * 4 < cost
    # ... and two labels meet at the ridge in cost, four texels before it in steps
    dims, vol, lab, q, closed = made["ridge between two labels"]
    _, steps = scene.geodesic_volume(vol, dims, scene.Geodesic(q.box, 0, q.window, q.seed, q.through), labels=lab)
    row_cost, row_steps = got["ridge between two labels"][1][1, 0, :] & 0xFF, steps[1, 0, :] & 0xFF
    assert row_cost[:ext[0]].tolist() == [1] * ext[0] and row_cost[ext[0]:].tolist() == [2] * (dims[0] - ext[0])
    assert row_steps[ext[0] - 3:ext[0]].tolist() == [2, 2, 2] and int(row_steps[ext[0] - 4]) == 1          # the tie at the midpoint goes to the smaller label
    # scene 4: each corridor alone reaches T at its own cost; the cheaper crosses more tile faces; and in the device's schedule, from the
    # tiles the init kernel marks, T's tile lowers words in three rounds or more, with rounds in which it rests between them
    dims, vol, lab, q, closed = made["a tile lowered again and again"]
    (t, (cost, label)), = closed["at"].items()
    alone = {}
    for l in (7, 8, 9):
        _, keys = scene.cost_volume(vol, dims, q.replace(seed=GS.table(l)), labels=lab)
        alone[l] = int(keys[t[2], t[1], t[0]]) >> 8
    assert alone == closed["costs"] and alone[7] > alone[8] > alone[9] == cost and label == 9
    assert closed["faces"][7] < closed["faces"][8] < closed["faces"][9] and closed["faces"][7] >= 2
    b, l = _box_bytes(dims, vol, lab)
    seed, medium = CS.predicates(b, l, q)
    keys, lowered_in = CS.scheduled(seed, medium, l, b, q, ext, np.random.default_rng(3), from_seeds=True)
    assert np.array_equal(keys, _signed(got["a tile lowered again and again"][1]))
    rounds = lowered_in[(t[2] // ext[2] * ext[2], t[1] // ext[1] * ext[1], t[0] // ext[0] * ext[0])]
    assert len(rounds) >= 3 and sum(b - a > 1 for a, b in zip(rounds, rounds[1:])) >= 2, rounds
    # scene 5, the ties: the tied texel lies where its name says, and the two chains have unequal step counts
    for axis in range(3):
        (face,), = [list(made["tied along %s, on a tile face" % "xyz"[axis]][4]["at"])]
        (inside,), = [list(made["tied along %s, inside a tile" % "xyz"[axis]][4]["at"])]
        assert face[axis] % ext[axis] == 0 and face[axis] > 0 and 0 < inside[axis] % ext[axis] < ext[axis] - 1
        dims, vol, lab, q, closed = made["tied along %s, on a tile face" % "xyz"[axis]]
        _, steps = scene.geodesic_volume(vol, dims, scene.Geodesic(q.box, 0, q.window, q.seed, q.through), labels=lab)
        assert int(steps[face[2], face[1], face[0]]) == (2 << 8 | 3)
        for l, n in ((5, 6), (3, 6)):
            _, keys = scene.cost_volume(vol, dims, q.replace(seed=GS.table(l)), labels=lab)
            assert int(keys[face[2], face[1], face[0]]) == (n << 8 | l)
    # scene 6, the overflow trap: 257 steps fit, and the sum a 32-bit register would hold for the 258th is a key below the limit
    dims, vol, lab, q, closed = made["the overflow trap"]
    assert dims[0] >= 320 and (q.step, q.contrast, q.max_cost) == (255, 255, 0)
    last = 257 * 65280
    assert last <= CS.COST_MAX < 258 * 65280 and ((last << 8) + (65280 << 8)) >= 2 ** 32 and ((((last << 8) + (65280 << 8)) % 2 ** 32) >> 8) <= CS.COST_MAX
    keys = _signed(got["the overflow trap"][1])
    assert (keys[0, 0, :258] >> 8).tolist() == [65280 * x for x in range(258)] and (keys[0, 0, 258:] == -1).all()
    assert int(got["the overflow trap"][0]["max_cost"]) == last and got["the overflow trap"][0]["hist"][255] > 0


def test_a_truncated_pass_is_the_untruncated_one_cut_off():
    """scene 7: limits on an attained cost and between two attained costs"""
    from volym_amd import scene
    host = CS.scene_a()
    cases = CS.limit_cases(host)
    assert len(cases) >= 4 and any(len(limits) == 3 for _, _, limits in cases)
    dropped = 0
    for name, c, limits in cases:
        _, full = scene.cost_volume(host.vol, host.dims, c, labels=host.labels)
        attained = set((full[full != np.uint32(CS.NONE)] >> 8).tolist())
        assert limits[0] in attained and limits[1] in attained and all(r not in attained and r - 1 in attained for r in limits[2:])
        for r in limits:
            _, cut = scene.cost_volume(host.vol, host.dims, c.replace(max_cost=r), labels=host.labels)
            want = CS.cut_off(full, r)
            assert np.array_equal(cut, want), (name, r)
            dropped += int((want != full).sum())
    assert dropped > 1000


# ---- the spread's twin -----------------------------------------------------------------------------------------------------------------
def test_the_spread_twin_equals_a_loop_per_texel_and_the_flood_twin_by_the_cost_map():
    from volym_amd import scene
    host = CS.scene_a()
    nx, ny, nz = host.dims
    changed = 0
    for case in CS.spread_cases():
        _, keys = CS.expect(host, case.cost)
        new, result = scene.spread_volume(host.vol, host.dims, case.spread, host.labels, keys, case.cost.box)
        f, (plo, phi) = case.spread, case.cost.box
        want = host.labels.reshape(nz, ny, nx).copy()
        count, left, arrived, hull = 0, [0] * 256, [0] * 256, None
        for z in range(f.box[0][2], f.box[1][2]):
            for y in range(f.box[0][1], f.box[1][1]):
                for x in range(f.box[0][0], f.box[1][0]):
                    l = int(want[z, y, x])
                    key = int(keys[z - plo[2], y - plo[1], x - plo[0]])
                    if not f.give[l] or key == CS.NONE:
                        continue
                    g, cost = key & 0xFF, key >> 8
                    n = int(f.to[g])
                    if not f.take[g] or n == l or not f.window[0] <= int(host.vol[x + nx * (y + ny * z)]) <= f.window[1] or not f.cost[0] <= cost <= f.cost[1]:
                        continue
                    count += 1
                    left[l] += 1
                    arrived[n] += 1
                    hull = [x, y, z, x + 1, y + 1, z + 1] if hull is None else [min(hull[0], x), min(hull[1], y), min(hull[2], z), max(hull[3], x + 1), max(hull[4], y + 1),
                                                                                  max(hull[5], z + 1)]
                    if not f.flags & CS.SPREAD_DRY_RUN:
                        want[z, y, x] = n
        assert (count == 0) == case.trivial, case.name
        assert int(result["changed"]) == count and result["left"].tolist() == left and result["arrived"].tolist() == arrived, case.name
        assert result["box"].tolist() == (hull or [0] * 6) and np.array_equal(new, want), case.name
        changed += count
        # flood_volume, handed the cost map and the band of cost as its band of steps, gives the same labels and the same result
        as_flood, flood_result = scene.flood_volume(host.vol, host.dims, case.spread.as_flood(), host.labels, keys, case.cost.box)
        assert np.array_equal(as_flood, new) and flood_result.tobytes() == result.tobytes(), case.name
    assert changed > 10000
