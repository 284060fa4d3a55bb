"""The measure pass on the device (volym_measure_pass / volym_read_measure / volym_measure_device_ptr).

The expected result is scene.measure_volume, the host twin of the rule (pinned to a plain triple loop by tests/test_measure_host.py),
of the prepared arrays the context was given and the cut state it was put in.  Every comparison is over all 36864 bytes of the
result: the rule is integer, so there is no tolerance and nothing is left out.  The scenes, boxes, cuts and group tables are those of
tests/measure_scenes.py, whose properties tests/test_measure_host.py asserts on the twin.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import measure_scenes as S
from tests.test_gpu_crop_box import CANOPY, _bonsai, _uniforms, _ctx

pytestmark = pytest.mark.gpu

FIELDS = ("count", "sum", "sum_sq", "sum_x", "sum_y", "sum_z", "box", "min", "max")


def _same(what, got, want):
    if S.as_bytes(got) == S.as_bytes(want):
        return
    for k in FIELDS:
        bad = np.flatnonzero((got[0][k] != want[0][k]).reshape(256, -1).any(axis=1))
        assert bad.size == 0, (what, k, bad[:6].tolist(), got[0][k][bad[:3]].tolist(), want[0][k][bad[:3]].tolist())
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (what, "hist", bad[:6].tolist(), got[1][got[1] != want[1]][:6].tolist(), want[1][got[1] != want[1]][:6].tolist())
    raise AssertionError((what, "the bytes differ though no field does"))


def _check(ctx, host, what, m, labels=True):
    ctx.measure_pass(m)
    want = S.expect(host, m, labels)
    _same(what, ctx.read_measure(), want)
    return want


# ---- 1. boxes, groups and cuts, both scenes, both layouts -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_box_and_group_under_every_cut(volym_lib, layout, which):
    """measured after each edit without a volym_update, in a context that never had a view; UNCUT before any cut and after cuts"""
    from volym_amd import _lib
    host = S.scene_a() if which == "a" else S.scene_b()
    counted = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.measure_device_ptr() is None
        for name, m in S.measures(_lib.MEASURE_UNCUT):
            _check(ctx, host, ("uncut, never cut", name), m)
        assert ctx.measure_device_ptr()
        for step, box, plane, hidden in S.CUTS:
            host.set_cut(ctx, box, plane, hidden)
            for name, m in S.measures():
                counted += int(_check(ctx, host, (step, name), m)[0]["count"].sum())
            for name, m in S.measures(_lib.MEASURE_UNCUT)[:4]:
                _check(ctx, host, (step, "uncut", name), m)
    assert counted > 100000


# ---- 2. label states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_without_labels_and_with_labels_of_other_dimensions(volym_lib, layout):
    from volym_amd import scene
    host = S.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels=False)
        for name, m in S.measures():
            want = _check(ctx, host, ("no labels", name), m, labels=False)
            assert int(want[0]["count"][1:].sum()) == 0
        host.set_cut(ctx, S.BOX, S.PLANE, None)
        for name, m in S.measures():
            _check(ctx, host, ("no labels, cut", name), m, labels=False)
        other = (S.NX + 1, S.NY, S.NZ)
        ctx.set_labels(np.full(other[0] * other[1] * other[2], 3, np.uint8), other)        # treated as none
        for name, m in S.measures():
            _check(ctx, host, ("labels of other dimensions", name), m, labels=False)


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_are_refused(volym_lib, layout):
    from volym_amd import _lib, scene
    host = S.scene_a()
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        _refused(_lib.E_STATE, ctx.measure_pass)
        _refused(_lib.E_STATE, ctx.measure_pass, scene.Measure(S.BOXES["texel"]))
        _refused(_lib.E_STATE, ctx.read_measure)
        ctx.set_labels(host.labels, host.dims)                   # (the option still says the other layout) ...
        _refused(_lib.E_STATE, ctx.measure_pass)
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)           # ... and now the volume's
        ctx.set_labels(host.labels, host.dims)
        _check(ctx, host, "labels uploaded again in the volume's layout", scene.Measure(dims=S.DIMS))


# ---- 3. repeats, frames, shards ------------------------------------------------------------------------------------------------------
def test_a_second_pass_carries_nothing_of_the_first(volym_lib):
    from volym_amd import scene
    host = S.scene_b()
    g = S.groups()
    with _ctx(0) as ctx:
        host.upload(ctx)
        ctx.measure_pass(scene.Measure(S.BOXES["whole"], 0, g["eight"]))
        ctx.measure_pass(scene.Measure(S.BOXES["texel"], 0, g["none"]))          # no read in between
        got = ctx.read_measure()
        _same("texel after whole", got, S.expect(host, scene.Measure(S.BOXES["texel"], 0, g["none"])))
        assert int(got[0]["count"].sum()) == 1 and int(got[1].sum()) == 0
        ctx.measure_pass(None)
        ctx.measure_pass(scene.Measure(S.BOXES["empty"]))
        _same("empty after whole", ctx.read_measure(), scene.empty_measurement())
        ctx.measure_pass(None)                                   # NULL: the whole volume, every label in group 0
        _same("NULL", ctx.read_measure(), S.expect(host, scene.Measure(dims=S.DIMS)))


def _bonsai_scene(ctx):
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut())
    ctx.set_labels(labels, dims)
    ctx.set_segment_importances(CANOPY)
    return dims, vol, labels


@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_frame_is_the_same_with_and_without_measure_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx)
        m = scene.Measure(((5, 3, 8), (60, 50, 64)), 0, np.arange(256) % 8)
        want = scene.measure_volume(vol, dims, m, labels=labels)
        assert (want[0]["count"] > 0).sum() >= 3
        ctx.measure_pass(m)                                      # before any volym_update or compute pass
        _same("before any update", ctx.read_measure(), want)
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.measure_pass(m)
        assert np.array_equal(ctx.read_rgba8(), frame), "frame read after a measure pass"
        for k in range(3):                                       # passes between frames that alternate between the slots
            ctx.compute_pass()
            ctx.measure_pass(m)
            ctx.compute_pass()
            assert np.array_equal(ctx.read_rgba8(), frame), ("frame", k)
            _same(("measure", k), ctx.read_measure(), want)


def test_a_sharded_context_measures_the_whole_volume(volym_lib):
    from volym_amd import scene
    with _ctx(0, w=160, h=96) as ctx:
        ctx.set_shard(1, 2)
        dims, vol, labels = _bonsai_scene(ctx)
        for m in (scene.Measure(dims=dims), scene.Measure(((0, 10, 20), (64, 40, 50)), 0, np.arange(256) % 8)):
            ctx.measure_pass(m)
            _same("sharded", ctx.read_measure(), scene.measure_volume(vol, dims, m, labels=labels))


def test_the_device_buffer_is_the_result_and_nothing_around_it(volym_lib):
    """the context's own buffer copied on the device into the middle of a guarded tensor: 36864 bytes, equal to the read"""
    from volym_amd import scene
    host = S.scene_a()
    with _ctx(1) as ctx:
        host.upload(ctx)
        m = scene.Measure(S.BOXES["x 5..30"], 0, S.groups()["mix"])
        ctx.measure_pass(m)
        ctx.sync()
        ptr = ctx.measure_device_ptr()
        assert ptr
        n, guard = 36864, 256
        holder = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        own = torch.as_tensor(_DeviceBytes(ptr, n), device="cuda")         # (a view of the context's buffer, no copy)
        holder[guard:guard + n].copy_(own)
        torch.cuda.synchronize()
        got = holder.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[guard + n:] == 0xA5).all()
        assert got[guard:guard + n].tobytes() == S.as_bytes(S.expect(host, m)) == S.as_bytes(ctx.read_measure())
        # the buffer stays where it is from pass to pass
        ctx.measure_pass(None)
        assert ctx.measure_device_ptr() == ptr


class _DeviceBytes:
    """n bytes of device memory at ptr, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = S.scene_a()
    whole = scene.Measure(dims=S.DIMS)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.measure_pass)                                # no volume
        _refused(_lib.E_STATE, ctx.measure_pass, whole)
        _refused(_lib.E_STATE, ctx.read_measure)                                # no pass
        assert ctx.measure_device_ptr() is None
        host.upload(ctx, labels=False)
        _refused(_lib.E_STATE, ctx.read_measure)                                # a volume, but still no pass
        ctx.measure_pass(whole)                                                 # needs the volume alone: no labels, no update
        for a in range(3):
            hi = list(S.DIMS); hi[a] += 1
            _refused(_lib.E_INVALID, ctx.measure_pass, scene.Measure(((0, 0, 0), tuple(hi))))
            lo = [0, 0, 0]; lo[a] = 5; hi = list(S.DIMS); hi[a] = 4
            _refused(_lib.E_INVALID, ctx.measure_pass, scene.Measure((tuple(lo), tuple(hi))))
        _refused(_lib.E_INVALID, ctx.measure_pass, whole.replace(flags=2))
        _refused(_lib.E_INVALID, ctx.measure_pass, whole.replace(flags=_lib.MEASURE_UNCUT | 4))
        for v in (8, 100, 254):
            g = np.zeros(256, np.int64); g[17] = v
            _refused(_lib.E_INVALID, ctx.measure_pass, whole.replace(group=g))
        assert volym_lib.volym_measure_pass(None, None) == _lib.E_INVALID
        assert volym_lib.volym_measure_pass(None, C.byref(whole.to_c())) == _lib.E_INVALID
        assert volym_lib.volym_read_measure(ctx.handle, None) == _lib.E_INVALID
        assert volym_lib.volym_read_measure(None, None) == _lib.E_INVALID
        assert volym_lib.volym_measure_device_ptr(None) is None
        # a refused pass leaves the latest result readable
        _same("after the refusals", ctx.read_measure(), S.expect(host, whole, labels=False))
        # a new volume: the result described the old one
        ctx.set_volume(host.vol, host.dims, 0)
        _refused(_lib.E_STATE, ctx.read_measure)
        assert ctx.measure_device_ptr() is None
        ctx.measure_pass(None)
        _same("after the new volume", ctx.read_measure(), S.expect(host, whole, labels=False))


# ---- 5. the Python callers ----------------------------------------------------------------------------------------------------------
def test_simple_measures_the_bonsai(oracle, volym_lib):
    from tests import common
    from volym_amd import demo, scene
    n = 32
    raw, labels_raw = common.bonsai(n)
    dims = (n, n, n)
    vol, lab = scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels_raw, dims, True)
    segments = [{"id": "Segment_1", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "Segment_2", "name": "Trunk", "label_value": 3, "importance": 0},
                {"id": "Segment_3", "name": "Pot", "label_value": 4, "importance": 0}]
    state = scene.State.with_parameters(160 / 96, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01))
    state.update()
    with demo.GpuContext(160, 96, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=segments, dims=dims)
        rec, hist = scene.measure_volume(vol, dims, scene.Measure(dims=dims), labels=lab)
        everything = d.measure(ctx)
        assert set(everything) >= {"Canopy", "Trunk", "Pot"} and len(everything) == int((rec["count"] > 0).sum())
        for name, l in (("Canopy", 2), ("Trunk", 3), ("Pot", 4)):
            want = scene.segment_summary(rec[l])
            got = everything[name]
            assert got["label"] == l and got["in_view"] == 1.0
            assert {k: got[k] for k in want} == want, name
        assert list(d.measure(ctx, ["Canopy", 4])) == ["Canopy", "Pot"]
        assert d.histogram(ctx).tolist() == np.bincount(vol, minlength=256).tolist()
        assert d.histogram(ctx, ["Canopy", "Trunk"]).tolist() == np.bincount(vol[(lab == 2) | (lab == 3)], minlength=256).tolist()
        # under cuts: the histogram of what is visible, the share of each segment that is in view
        lo, hi = d.set_crop(ctx, (0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        d.set_hidden(ctx, ["Segment_3"])
        cut = {"box": (lo, hi), "visible": scene.visibility_mask([4])}
        now = scene.cut_volume(vol, dims, cut, lab)
        rec_cut, hist_cut = scene.measure_volume(now, dims, scene.Measure(dims=dims), labels=lab, cut=cut, uncut=vol)
        assert d.histogram(ctx).tolist() == hist_cut[0].tolist()
        cut_view = d.measure(ctx, ["Canopy", "Pot"])
        assert cut_view["Pot"] is None
        assert cut_view["Canopy"]["count"] == int(rec_cut["count"][2]) and 0.0 < cut_view["Canopy"]["in_view"] < 1.0
        assert cut_view["Canopy"]["in_view"] == int(rec_cut["count"][2]) / int(rec["count"][2])
        assert d.measure(ctx, ["Canopy"], uncut=True)["Canopy"]["count"] == int(rec["count"][2])
        half = d.measure(ctx, ["Canopy"], box01=((0.0, 0.0, 0.0), (1.0, 1.0, 0.5)), uncut=True)["Canopy"]
        assert half["count"] == int(scene.measure_volume(vol, dims, scene.Measure(((0, 0, 0), (n, n, n // 2))), labels=lab)[0]["count"][2])
        d.set_hidden(ctx, [])
        ctx.set_crop_box((0, 0, 0), dims)
        # click to measure: the summary of the segment the pixel shows
        d.compute_pass(ctx)
        hits = 0
        for x, y in ((80, 48), (80, 30), (80, 70), (60, 40), (2, 2)):
            p = d.measure_at(ctx, x, y)
            if p["status"] == "hit" and p["label"] is not None:
                hits += 1
                want = scene.segment_summary(rec[p["label"]])
                assert {k: p["measure"][k] for k in want} == want and p["measure"]["label"] == p["label"]
            else:
                assert p["measure"] is None
        assert hits >= 1


# ---- 6. the accumulator widths: a constant volume of byte 255 with one label ---------------------------------------------------------
@pytest.mark.parametrize("n, layout", [(64, 0), (64, 1), (256, 0), (256, 1), (640, 1)])
def test_sums_of_squares_beyond_32_bits(volym_lib, layout, n):
    """sum_sq is 1.7e10 at 64^3 and 1.09e12 at 256^3: a 32-bit total fails at either.  The share of one of at most 2048 workgroups
    is 5.3e8 at 256^3 and stays below 2^32 up to 512^3 (134217728 * 65025 / 2048 = 4.26e9 < 4.29e9), so a 32-bit sum in LDS fails
    only beyond that: the 640^3 case, in the layout a volume of that size gets.  The closed form needs no NumPy pass."""
    from volym_amd import scene
    dims = (n, n, n)
    total = n ** 3
    with _ctx(layout) as ctx:
        ctx.set_volume(np.full(total, 255, np.uint8), dims, 0)
        ctx.set_labels(np.full(total, 7, np.uint8), dims)
        ctx.measure_pass(scene.Measure(dims=dims, group=scene.measure_groups([], [], [7])))
        rec, hist = ctx.read_measure()
    want_rec, want_hist = scene.empty_measurement()
    r = want_rec[7:8]
    r["count"], r["sum"], r["sum_sq"] = total, 255 * total, 65025 * total
    r["sum_x"] = r["sum_y"] = r["sum_z"] = total * (n - 1) // 2
    r["min"] = r["max"] = 255
    r["box"] = [0, 0, 0, n - 1, n - 1, n - 1]
    want_hist[2][255] = total
    assert 65025 * total > 2 ** 32 and (n < 640 or 65025 * total // 2048 > 2 ** 32)
    _same(("constant", n, layout), (rec, hist), (want_rec, want_hist))
