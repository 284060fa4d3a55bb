"""The label edit on the device (volym_edit_labels / volym_read_labels).

The expected labels and result are scene.relabel_volume's, the host twin of the rule (pinned to a plain triple loop by
tests/test_relabel_host.py).  The rule is integer: there is no tolerance anywhere and nothing is left out.  After every edit the
result's 4128 bytes, the labels (whole and on a sub-box) and the label counts are compared with the twin, and the state of the context
with that of a reference context that is handed the same volume, the twin's labels, the same table and the same cuts: a whole-volume
measure pass cut and UNCUT, slice passes in density and importance mode on every z plane, and one frame with importance rendering and
look-ahead on, bit-equal in rgba8.  The scenes and requests are those of tests/relabel_scenes.py, whose properties
tests/test_relabel_host.py asserts on the twin.
"""
import ctypes as C

import numpy as np
import pytest

from tests import measure_scenes as MS
from tests import relabel_scenes as RS
from tests.test_gpu_crop_box import H, PARAMS, W, _ctx, _uniforms

pytestmark = pytest.mark.gpu

SUB = ((3, 1, 2), (30, 20, 17))
POSE = (35.0, 20.0, 0.0)


def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def _cut_to(ctx, host):
    """put a context that was just handed the scene into the cut state of `host`"""
    if host.cut is None:
        return
    if host.cut["box"] != ((0, 0, 0), host.dims):
        ctx.set_crop_box(*host.cut["box"])
    if host.cut["plane"] != ((0, 0, 0), 0):
        ctx.set_clip_plane(*host.cut["plane"])
    if not np.asarray(host.cut["visible"]).all():
        ctx.set_segment_visibility(host.cut["visible"])


class Reference:
    """the context that is handed the edited labels: a new one per look (reuse False), or one that is handed the whole scene again"""

    def __init__(self, layout, reuse=True):
        self.layout, self.reuse, self.ctx = layout, reuse, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.ctx is not None:
            self.ctx.__exit__(None, None, None)
            self.ctx = None

    def at(self, host):
        if not self.reuse:
            self.close()
        if self.ctx is None:
            self.ctx = _ctx(self.layout).__enter__()
        host.upload(self.ctx)                       # (volym_set_volume: whole volume, no plane, no mask, no copies)
        _cut_to(self.ctx, host)
        return self.ctx


def _views(ctx, host, uniforms):
    """what a context shows of its scene: measure passes, slices of every z plane, one frame"""
    from volym_amd import _lib, scene
    out = {}
    for flags in (0, _lib.MEASURE_UNCUT):
        ctx.measure_pass(scene.Measure(flags=flags, group=np.arange(256) % 8, dims=host.dims))
        out["measure", flags] = MS.as_bytes(ctx.read_measure())
    for z in range(host.dims[2]):
        for mode in (_lib.SLICE_DENSITY, _lib.SLICE_IMPORTANCE):
            ctx.slice_pass(scene.slice_axis("z", z, host.dims).replace(mode=mode))
            out["slice", z, mode] = ctx.read_slice().tobytes()
    if uniforms is not None:
        ctx.update(*uniforms)
        ctx.compute_pass()
        ctx.sync()
        out["frame"] = ctx.read_rgba8().tobytes()
    return out


def _look(ctx, host, ref, what, uniforms):
    """labels, counts and state of `ctx` against the twin's labels (host.labels) and the reference context"""
    from volym_amd import _lib, scene
    nx, ny, nz = host.dims
    want = host.labels.reshape(nz, ny, nx)
    got = ctx.read_labels()
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (what, "labels", int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    (x0, y0, z0), (x1, y1, z1) = sub = tuple(tuple(min(v, n) for v, n in zip(p, host.dims)) for p in SUB)
    assert np.array_equal(ctx.read_labels(sub), want[z0:z1, y0:y1, x0:x1]), (what, "labels of a sub-box")
    assert ctx.label_counts().tolist() == np.bincount(host.labels, minlength=256).tolist(), (what, "label counts")
    mine, theirs = _views(ctx, host, uniforms), _views(ref.at(host), host, uniforms)
    for k in mine:
        assert mine[k] == theirs[k], (what, "differs from the context that was handed the edited labels", k)
    for flags in (0, _lib.MEASURE_UNCUT):
        m = scene.Measure(flags=flags, group=np.arange(256) % 8, dims=host.dims)
        assert mine["measure", flags] == MS.as_bytes(MS.expect(host, m)), (what, "measure pass against the twin", flags)


def _edit(ctx, host, case, snaps=None, passes=True):
    """run the passes `case` reads and the edit, compare the result with the twin's and take the twin's labels; returns the result"""
    from volym_amd import _lib
    if passes and case.components is not None:
        ctx.components_pass(case.components)
    if passes and case.distance is not None:
        ctx.distance_pass(case.distance)
    new, want, r = RS.expect(host, case, snaps)
    got = ctx.edit_labels(r)
    for k in ("changed", "left", "arrived", "box"):
        assert np.array_equal(got[k], want[k]), (case.name, k, np.asarray(got[k]).ravel()[:8].tolist(), np.asarray(want[k]).ravel()[:8].tolist())
    assert got.tobytes() == want.tobytes() and len(got.tobytes()) == 4128, case.name
    if not r.flags & _lib.RELABEL_DRY_RUN:
        host.labels = new
    return got


def _hand_labels(ctx, host, labels):
    """the context gets `labels` as a caller would send them: a new label volume, the table and the mask again"""
    host.labels = labels.copy()
    ctx.set_labels(host.labels, host.dims)
    ctx.set_segment_importances(host.table)
    if host.cut is not None and not np.asarray(host.cut["visible"]).all():
        ctx.set_segment_visibility(host.cut["visible"])


def _frame_uniforms(oracle):
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE, **PARAMS["straight"])
    return cu, pu


SCENES = {"a": (RS.scene_a, RS.cases_a), "b": (RS.scene_b, RS.cases_b), "ragged": (RS.scene_ragged, RS.cases_ragged)}


# ---- 1. every request, both layouts, before any cut and under cuts ----------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", list(SCENES))
def test_every_request_before_any_cut(oracle, volym_lib, layout, which):
    make, cases = SCENES[which]
    host = make()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    changed = 0
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for k, case in enumerate(cases()):
            if k:
                _hand_labels(ctx, host, original)
            changed += int(_edit(ctx, host, case)["changed"])
            _look(ctx, host, ref, case.name, uniforms)
    assert changed > 1000


@pytest.mark.parametrize("layout", [0, 1])
def test_a_rotating_subset_after_each_cut(oracle, volym_lib, layout):
    host = RS.scene_a()
    original = host.labels.copy()
    uniforms = _frame_uniforms(oracle)
    cases = RS.cases_a()
    seen = set()
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        for step, (name, box, plane, hidden) in enumerate(MS.CUTS):
            host.set_cut(ctx, box, plane, hidden)
            for case in cases[step % 4::4]:
                _hand_labels(ctx, host, original)
                _edit(ctx, host, case)
                _look(ctx, host, ref, (name, case.name), uniforms)
                seen.add(case.name)
    assert len(seen) == len(cases)


# ---- 2. edits followed by other edits of the scene ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_hiding_showing_and_cropping_after_edits(oracle, volym_lib, layout):
    """the recomputed label boxes are exact: a later mask or crop edit rewrites from them"""
    host = RS.scene_a()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in RS.cases_a()}
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        _edit(ctx, host, cases["table, x 3..8"])                       # 0, 1 -> 9 and 4 -> 2 in a narrow box: label 9 is new
        _edit(ctx, host, cases["merge 1, 2 -> 4, whole"])              # labels 1 and 2 are gone
        assert int((host.labels == 1).sum()) == 0 and int((host.labels == 9).sum()) > 50
        for hidden in ([9], [4], [1, 2], [4, 9, 0], None):              # the new label, a target, sources without voxels, several
            host.set_cut(ctx, None, None, hidden)
            _look(ctx, host, ref, ("hidden", hidden), uniforms)
        host.set_cut(ctx, MS.BOX, None, [9])
        _look(ctx, host, ref, "box and hidden", uniforms)
        _edit(ctx, host, cases["swap 0 <-> 3, rows"])                  # an edit under both, then the cuts move again
        _look(ctx, host, ref, "swap under box and hidden", uniforms)
        host.set_cut(ctx, ((5, 0, 3), (36, 22, 12)), MS.PLANE, [3])
        _look(ctx, host, ref, "another box, a plane, another label hidden", uniforms)
        host.set_cut(ctx, None, None, None)
        _look(ctx, host, ref, "all lifted", uniforms)


@pytest.mark.parametrize("layout", [0, 1])
def test_relabel_into_a_hidden_label_without_voxels_in_a_context_that_never_cut(oracle, volym_lib, layout):
    from volym_amd import _lib, scene
    host = RS.scene_a()
    uniforms = _frame_uniforms(oracle)
    case = RS.Case("0, 1 -> 9", scene.Relabel(MS.BOXES["x 5..30"], to={0: 9, 1: 9}))
    with _ctx(layout) as ctx, Reference(layout, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [9])                             # no voxel carries 9: no byte changes, no copy is made
        moved = int(_edit(ctx, host, case)["changed"])
        assert moved > 500
        _look(ctx, host, ref, "moved into the hidden label", uniforms)
        whole = scene.Measure(dims=host.dims)
        ctx.measure_pass(whole)
        assert int(ctx.read_measure()[0]["count"][9]) == 0              # the moved texels' density reads 0 ...
        ctx.measure_pass(whole.replace(flags=_lib.MEASURE_UNCUT))
        rec = ctx.read_measure()[0]
        assert int(rec["count"][9]) == moved and int(rec["min"][9]) >= 1    # ... and is kept in the uncut copy
        host.set_cut(ctx, None, None, None)
        ctx.measure_pass(whole)
        assert int(ctx.read_measure()[0]["count"][9]) == moved          # shown: it comes back
        _look(ctx, host, ref, "the label shown again", uniforms)


# ---- 3. dry runs, no-ops and the surface pass -----------------------------------------------------------------------------------
def test_a_dry_run_changes_nothing_and_only_a_real_edit_makes_a_surface_stale(oracle, volym_lib):
    from volym_amd import _lib, scene
    host = RS.scene_a()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in RS.cases_a()}
    merge = cases["merge 1, 2 -> 4, whole"]
    with _ctx(1) as ctx, Reference(1, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, MS.BOX, None, [4])
        s = scene.Surface(dims=host.dims, min_byte=100)
        ctx.surface_pass(s)
        ctx.surface_faces_pass()
        total = int(ctx.read_surface()["total"])
        faces = ctx.read_surface_faces(total).tobytes()
        assert total > 100
        before = host.labels.copy()
        dry = RS.Case("dry", merge.relabel.replace(flags=_lib.RELABEL_DRY_RUN))
        got = _edit(ctx, host, dry)
        assert int(got["changed"]) == int(((before == 1) | (before == 2)).sum()) and np.array_equal(host.labels, before)
        for name in ("identity", "identity under a window and ids", "empty box"):
            assert int(_edit(ctx, host, cases[name])["changed"]) == 0
        _look(ctx, host, ref, "after a dry run and no-ops", uniforms)
        ctx.surface_faces_pass()                                        # still the surface of the scene as it stands
        assert ctx.read_surface_faces(total).tobytes() == faces
        assert int(_edit(ctx, host, merge)["changed"]) > 0
        _refused(_lib.E_STATE, ctx.surface_faces_pass)
        _look(ctx, host, ref, "after the real edit", uniforms)
        ctx.surface_pass(s)
        ctx.surface_faces_pass()


# ---- 4. the snapshots -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_device_snapshots_are_the_twins_and_one_snapshot_serves_two_edits(oracle, volym_lib, layout):
    host = RS.scene_a()
    uniforms = _frame_uniforms(oracle)
    cases = {c.name: c for c in RS.cases_a()}
    first, second = cases["the largest piece of 3 and 4 -> 8"], cases["pieces 2..40 of 3 -> 6, rows"]
    grow, rim = cases["grow 2 by 2"], cases["shrink 2 by 1"]
    with _ctx(layout) as ctx, Reference(layout) as ref:
        host.upload(ctx)
        snaps = RS.snapshots(host, first)
        ctx.components_pass(first.components)
        assert np.array_equal(ctx.read_component_ids(), snaps["components"][2])
        assert int(_edit(ctx, host, first, snaps, passes=False)["changed"]) > 50
        # the same ids again, though the labels they were found in have changed: no new pass
        assert second.components is first.components or second.components.box == first.components.box
        assert int(_edit(ctx, host, second, snaps, passes=False)["changed"]) > 50
        _look(ctx, host, ref, "two edits from one id volume", uniforms)
        snaps = RS.snapshots(host, grow)
        ctx.distance_pass(grow.distance)
        assert np.array_equal(ctx.read_distance_map(), snaps["distance"][1])
        assert int(_edit(ctx, host, grow, snaps, passes=False)["changed"]) > 50
        # the map of the segment before it grew, applied once more: a different band of the same snapshot
        again = RS.Case("ring 5..8", grow.relabel.replace(to={2: 13}, d2=(5, 8)), distance=grow.distance)
        assert int(_edit(ctx, host, again, snaps, passes=False)["changed"]) == 0     # (those texels were no 2 and did not become one)
        again = RS.Case("ring 1..4 back to 0", grow.relabel.replace(to={2: 0}, d2=(1, 4)), distance=grow.distance)
        assert int(_edit(ctx, host, again, snaps, passes=False)["changed"]) > 50
        _look(ctx, host, ref, "three edits from one map", uniforms)
        # ids and a map of different passes in one request, the map taken under the labels as they are now
        _edit(ctx, host, cases["the rim of the blocks of 2 but the largest"])
        _edit(ctx, host, rim)
        _look(ctx, host, ref, "both snapshots", uniforms)


# ---- 5. frames in flight --------------------------------------------------------------------------------------------------------
def test_an_edit_between_frames_with_two_frames_in_flight(oracle, volym_lib):
    from volym_amd import _lib
    host = RS.scene_a()
    cu, pu = _frame_uniforms(oracle)
    cases = {c.name: c for c in RS.cases_a()}
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)]) as ctx, Reference(0, reuse=False) as ref:
        host.upload(ctx)
        host.set_cut(ctx, None, None, [4])
        ctx.update(cu, pu)
        for _ in range(3):
            ctx.compute_pass()
        before = ctx.read_rgba8()
        for name in ("merge 1, 2 -> 4, whole", "window 100..180, whole"):
            ctx.compute_pass()                                          # a frame in flight while the edit arrives
            _edit(ctx, host, cases[name])
            frames = []
            for _ in range(3):                                          # both slots, with no update in between
                ctx.compute_pass()
                frames.append(ctx.read_rgba8())
            r = ref.at(host)
            r.update(cu, pu)
            r.compute_pass()
            want = r.read_rgba8()
            assert not np.array_equal(want, before), "the edit must show"
            for k, f in enumerate(frames):
                assert np.array_equal(f, want), (name, "frame", k)
            before = want


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = RS.scene_a()
    whole = scene.Relabel(dims=host.dims, to={1: 2})
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.edit_labels, whole)                  # no volume
        _refused(_lib.E_STATE, ctx.read_labels)                         # no labels
        host.upload(ctx, labels=False)
        _refused(_lib.E_STATE, ctx.edit_labels, whole)                  # no labels
        other = (host.dims[0] + 1, host.dims[1], host.dims[2])
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)
        _refused(_lib.E_STATE, ctx.edit_labels, whole)                  # labels of other dimensions
        assert ctx.read_labels().shape == other[::-1] and int(ctx.read_labels(((0, 0, 0), (38, 1, 1))).sum()) == 3 * 38
        ctx.set_labels(host.labels, host.dims)
        assert int(ctx.edit_labels(whole.replace(flags=_lib.RELABEL_DRY_RUN))["changed"]) == int((host.labels == 1).sum())
        for flags in (_lib.RELABEL_IDS, _lib.RELABEL_DISTANCE, _lib.RELABEL_IDS | _lib.RELABEL_DISTANCE):
            _refused(_lib.E_STATE, ctx.edit_labels, whole.replace(flags=flags))        # no such pass yet
        ctx.components_pass(scene.Components(MS.BOXES["x 5..30"]))
        ctx.distance_pass(scene.Distance(MS.BOXES["rows"]))
        for flags, inside in ((_lib.RELABEL_IDS, MS.BOXES["x 5..30"]), (_lib.RELABEL_DISTANCE, MS.BOXES["rows"])):
            _refused(_lib.E_INVALID, ctx.edit_labels, whole.replace(flags=flags))      # the whole volume reaches outside that pass's box
            (x0, y0, z0), (x1, y1, z1) = inside
            _refused(_lib.E_INVALID, ctx.edit_labels, whole.replace(flags=flags, box=((x0, y0, z0), (x1, y1, z1 + 1))))
            _refused(_lib.E_INVALID, ctx.edit_labels, whole.replace(flags=flags, box=((x0, y0 - 1, z0), (x1, y1, z1))))
            assert int(ctx.edit_labels(whole.replace(flags=flags | _lib.RELABEL_DRY_RUN, box=inside, ids=(0, 2 ** 32 - 2), d2=(0, 2 ** 32 - 2)))["changed"]) > 0
        for a in range(3):
            hi = list(host.dims); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.edit_labels, whole.replace(box=((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(host.dims); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.edit_labels, whole.replace(box=(tuple(lo), tuple(hi))))
        for bad in (dict(flags=32), dict(flags=_lib.RELABEL_IDS_EXCEPT), dict(window=(9, 8)), dict(window=(0, 256)),
                    dict(flags=_lib.RELABEL_IDS, ids=(3, 2), box=MS.BOXES["x 5..30"]), dict(flags=_lib.RELABEL_DISTANCE, d2=(3, 2), box=MS.BOXES["rows"])):
            _refused(_lib.E_INVALID, ctx.edit_labels, whole.replace(**bad))
        assert volym_lib.volym_edit_labels(None, C.byref(whole.to_c()), None) == _lib.E_INVALID
        assert volym_lib.volym_edit_labels(ctx.handle, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_labels(None, None, None) == _lib.E_INVALID
        assert volym_lib.volym_read_labels(ctx.handle, None, None) == _lib.E_INVALID
        _refused(_lib.E_INVALID, ctx.read_labels, ((0, 0, 0), (host.dims[0] + 1, 1, 1)))
        _refused(_lib.E_INVALID, ctx.read_labels, ((2, 0, 0), (1, 1, 1)))
        assert ctx.read_labels(((4, 4, 4), (4, 9, 9))).size == 0
        # nothing above changed a label, and a NULL result is accepted
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)
        assert volym_lib.volym_edit_labels(ctx.handle, C.byref(whole.to_c()), None) == _lib.OK
        assert int((ctx.read_labels() == 1).sum()) == 0
        # a new volume: ids and map described the old one
        ctx.set_volume(host.vol, host.dims, 0)
        for flags in (_lib.RELABEL_IDS, _lib.RELABEL_DISTANCE):
            _refused(_lib.E_STATE, ctx.edit_labels, whole.replace(flags=flags, box=((6, 6, 6), (7, 7, 7))))


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = RS.scene_a()
    whole = scene.Relabel(dims=host.dims, to={1: 2})
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.edit_labels, whole)
        assert np.array_equal(ctx.read_labels().ravel(), host.labels)   # (reading needs no volume and minds no layout)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_labels(host.labels, host.dims)
        ctx.set_segment_importances(host.table)
        assert int(ctx.edit_labels(whole)["changed"]) == int((host.labels == 1).sum())


# ---- 7. the Python callers ------------------------------------------------------------------------------------------------------
def test_simple_edits_the_bonsai(oracle, volym_lib, tmp_path):
    from tests import common
    from volym_amd import _lib, demo, scene
    n = 64
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
                {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    whole = ((0, 0, 0), dims)
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        # grow the canopy by 2 into the air
        dist = scene.distance_volume(vol, dims, scene.Distance(dims=dims, select=scene.surface_select([2])), labels=lab)
        want, res = scene.relabel_volume(vol, dims, scene.Relabel(dims=dims, flags=_lib.RELABEL_DISTANCE, to={0: 2}, d2=(0, 4)), lab, dmap=dist[1], dmap_box=whole)
        got = d.grow(ctx, "Canopy", 2)
        assert got["changed"] == int(res["changed"]) > 50 and got["arrived"] == {2: got["changed"]} and got["left"] == {0: got["changed"]}
        assert np.array_equal(ctx.read_labels(), want)
        lab = want.ravel()
        # shrink it again by 1
        dist = scene.distance_volume(vol, dims, scene.Distance(dims=dims, flags=_lib.DISTANCE_INSIDE, select=scene.surface_select([2])), labels=lab)
        want, res = scene.relabel_volume(vol, dims, scene.Relabel(dims=dims, flags=_lib.RELABEL_DISTANCE, to={2: 0}, d2=(0, 1)), lab, dmap=dist[1], dmap_box=whole)
        assert d.shrink(ctx, "Canopy", 1)["changed"] == int(res["changed"]) > 50
        assert np.array_equal(ctx.read_labels(), want)
        lab = want.ravel()
        # keep the largest piece of the trunk at a threshold that breaks it, the rest to a new segment
        comp = scene.components_volume(vol, dims, scene.Components(dims=dims, min_byte=200, select=scene.surface_select([3])), labels=lab)
        assert int(comp[0]["n_components"]) > 1
        k = int(np.argmax(comp[1]["count"]))
        kept = d.keep_largest(ctx, "Trunk", rest="Chips", min_byte=200)
        chips = next(s for s in d._segments if s["name"] == "Chips")
        assert chips["label_value"] not in (0, 2, 3, 4) and chips["importance"] == 0 and kept["kept"] == k and kept["pieces"] == int(comp[0]["n_components"])
        want, res = scene.relabel_volume(vol, dims, scene.Relabel(dims=dims, flags=_lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT, to={3: chips["label_value"]}, ids=(k, k)),
                                         lab, ids=comp[2], ids_box=whole)
        assert kept["changed"] == int(res["changed"]) > 0 and np.array_equal(ctx.read_labels(), want)
        lab = want.ravel()
        # merge by the table, paint by a window, a dry run
        assert d.relabel(ctx, {"Chips": "Trunk"})["changed"] == int(res["changed"])
        lab = np.where(lab == chips["label_value"], 3, lab).astype(np.uint8)
        dry = d.relabel(ctx, {"Pot": 0}, dry_run=True)
        assert dry["changed"] == int((lab == 4).sum()) and np.array_equal(ctx.read_labels().ravel(), lab)
        painted = d.paint(ctx, "Pot", (30, 255), box01=((0.0, 0.0, 0.0), (1.0, 0.3, 1.0)))
        lo, hi = scene.crop_box_texels((0.0, 0.0, 0.0), (1.0, 0.3, 1.0), dims)
        want, res = scene.relabel_volume(vol, dims, scene.Relabel((lo, hi), window=(30, 255), to={0: 4}), lab)
        assert painted["changed"] == int(res["changed"]) and np.array_equal(ctx.read_labels(), want)
        lab = want.ravel()
        # click to split: the piece under the pixel gets a segment of its own with the source's importance
        d.compute_pass(ctx)
        hit = None
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (100, 40)):
            p = d.split_at(ctx, x, y, "Picked")
            if p["relabel"] is not None:
                hit = p
                break
        assert hit is not None and hit["relabel"]["changed"] > 0
        picked = next(s for s in d._segments if s["name"] == "Picked")
        source = next(s for s in segments if s["label_value"] == hit["label"])
        assert picked["importance"] == source["importance"] and hit["relabel"]["label"] == picked["label_value"]
        now = ctx.read_labels()
        assert now[hit["texel"][2], hit["texel"][1], hit["texel"][0]] == picked["label_value"]
        assert int((now == picked["label_value"]).sum()) == hit["relabel"]["changed"] and int((now.ravel() != lab).sum()) == hit["relabel"]["changed"]
        # the file holds the labels in the orientation they were read in
        path = str(tmp_path / "labels.raw")
        assert d.save_labels(ctx, path) == n ** 3
        saved = np.fromfile(path, np.uint8)
        assert np.array_equal(scene.prepare_volume(saved, dims, True), now.ravel())


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_clis_relabel_and_write_the_labels(volym_lib, tmp_path, cli):
    """--relabel and --labels-out on `run simple` with the built-in teapot: the file holds the relabelled labels in the orientation
    they were read in; the Python CLI also keeps the largest piece, grows and shrinks"""
    import json
    import os
    import subprocess
    import sys
    from volym_amd import scene, synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    out = str(tmp_path / "labels.raw")
    cmd = [sys.executable, "-m", "volym_amd", "run", "simple", "--width", "160", "--height", "90", "--screenshot", str(tmp_path / "a.png")] if cli == "python" else \
          [os.path.join(root, "volym_amd", "volym"), "run", "simple", "--width", "160", "--height", "90", "--output", str(tmp_path / "a.ppm")]
    r = subprocess.run(cmd + ["--relabel", "Cup,4:Lobster", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (cmd[0], r.stderr[-2000:])
    dims = (256, 256, 256)
    _, labels_raw = synth.synth_teapot()
    before = scene.prepare_volume(labels_raw, dims, True)
    want = np.where((before == 3) | (before == 4), 2, before).astype(np.uint8)
    moved = int((want != before).sum())
    assert moved > 1000
    saved = np.fromfile(out, np.uint8)
    assert saved.size == 256 ** 3 and np.array_equal(scene.prepare_volume(saved, dims, True), want)
    assert "labels: %d bytes -> %s" % (256 ** 3, out) in r.stdout
    if cli == "native":
        line = [l for l in r.stdout.splitlines() if l.startswith("relabel:")]
        assert len(line) == 1 and line[0].startswith("relabel: %d texels changed, box [" % moved) and "label 2: -0 +%d" % moved in line[0], r.stdout
        return
    first = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"relabel"')]
    assert len(first) == 1 and first[0]["relabel"]["changed"] == moved and first[0]["relabel"]["arrived"] == {"2": moved}
    r = subprocess.run(cmd + ["--keep-largest", "Lobster", "--grow", "Cup:2", "--shrink", "Ground:1"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [list(l)[0] for l in lines] == ["keep_largest", "grow", "shrink"], r.stdout
    assert lines[0]["keep_largest"]["pieces"] >= 1 and lines[0]["keep_largest"]["changed"] == sum(lines[0]["keep_largest"]["left"].values())
    assert lines[1]["grow"]["changed"] > 1000 and list(lines[1]["grow"]["arrived"]) == ["3"] and list(lines[1]["grow"]["left"]) == ["0"]
    assert lines[2]["shrink"]["changed"] > 1000 and list(lines[2]["shrink"]["left"]) == ["4"] and list(lines[2]["shrink"]["arrived"]) == ["0"]
    # click to split: the pixel at the centre shows a segment, whose piece becomes "Picked" with a label value of its own
    r = subprocess.run(cmd + ["--split-at", "80,45:Picked", "--labels-out", out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    split = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"split_at"')]
    assert len(split) == 1 and split[0]["split_at"] is not None and split[0]["split_at"]["label"] == 1 and split[0]["split_at"]["arrived"] == {"1": split[0]["split_at"]["changed"]}
    assert int((np.fromfile(out, np.uint8) == 1).sum()) == split[0]["split_at"]["changed"] > 0
    for bad in (["--relabel", "3"], ["--grow", "Cup"], ["--relabel", "Nobody:3"]):
        r = subprocess.run(cmd + bad, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
        assert r.returncode != 0 and bad[0][2:] in (r.stderr + r.stdout) or "label edit" in r.stderr, (bad, r.stderr[-500:])
