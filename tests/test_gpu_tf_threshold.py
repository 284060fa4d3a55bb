"""The transfer-function and threshold axes of the HIP ray-march against the CPU oracle.

Every other rendering test draws with the default table (256 texels, an alpha ramp that never reaches 255) and with thresholds
that are never the float of b/255.  Here: tables of 1 to 256 texels, opaque, transparent, comb, step and baked ones -- through
the host's baked tables (nearest filter) and the device's own lookup (trilinear, smoothed) --, thresholds one float below, at and
one float above a plateau's byte, at or below 0 and above 1, table and step changes between frames that are enqueued without a
wait in between, the multi-GPU loop's table, and the refusals.  The bar is test_gpu_parity.py's, on every pixel: the five
counters identical, every channel within 1e-4, rgba8 within 1 LSB.  tests/test_oracle_tf_threshold.py pins the oracle itself
on these inputs."""
import ctypes

import numpy as np
import pytest

from tests import common
from tests.test_gpu_parity import _STEPS, _check, _ctx, _render_gpu

pytestmark = pytest.mark.gpu

TF_NAMES = ["default", "random 1", "random 2", "random 3", "random 7", "random 100", "random 255", "random 256",
            "opaque", "transparent", "comb", "step", "baked"]
TF_SEED = 5

FLAG_SETS = [
    ("plain", dict()),
    ("no opacity", dict(use_opacity=0)),
    ("smoothed", dict(use_gaussian_smoothing=1)),
    ("importance rendering, straight", dict(use_importance_rendering=1)),
    ("importance rendering, cone", dict(use_importance_rendering=1, use_cone_importance_check=1)),
    ("importance colouring", dict(use_importance_coloring=1)),
    ("smoothed + importance rendering", dict(use_gaussian_smoothing=1, use_importance_rendering=1)),
]


def _family():
    fam = common.tf_family(np.random.default_rng(TF_SEED))
    assert [name for name, _ in fam] == TF_NAMES
    return dict(fam)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def bonsai64(oracle):
    from volym_amd import scene
    raw, labels = common.bonsai(64)
    dims = (64, 64, 64)
    vol, imp = common.oracle_scene(oracle, raw, labels, common.BONSAI_SEGMENTS, dims)
    dev_vol = scene.prepare_volume(raw, dims, True)
    dev_imp = scene.prepare_volume(scene.map_segments_to_importance(labels, common.BONSAI_SEGMENTS), dims, True)
    return dims, vol, imp, dev_vol, dev_imp


# ---- 1. the family of tables ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "linear"])
@pytest.mark.parametrize("name,layout", [(n, 0) for n in TF_NAMES] + [("random 7", 1), ("opaque", 1)],
                         ids=[n.replace(" ", "-") for n in TF_NAMES] + ["random-7-bricked", "opaque-bricked"])
def test_tf_family(oracle, volym_lib, bonsai64, name, layout, filt):
    """One table of the family on bonsai 64^3 at 96x64 under seven flag sets: the default kernel twice with every marched tile
    split into depth-parallel items on the second frame, then kernels 0, 1 and 3.  `opaque` and `step` end every ray in its first
    quarter; `transparent` never ends one (and leaves alpha exactly 0 on every ray that meets the cube)."""
    from volym_amd import _lib
    dims, vol, imp, dev_vol, dev_imp = bonsai64
    lut = _family()[name]
    W, H = 96, 64
    cam = oracle.benchmark_camera_uniforms(W / H)
    cases = 0
    with _ctx(W, H) as ctx:
        ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
        ctx.set_option(_lib.OPT_DEPTH_PARALLEL, 1)
        ctx.set_volume(dev_vol, dims, filt)
        ctx.set_importances(dev_imp, dims)
        ctx.set_transfer_function(lut)
        for mode, kw in FLAG_SETS:
            par = oracle.make_parameters(density_threshold=0.15, importance_check_ahead_steps=6, raymarching_step_size=0.01, **kw)
            ref = oracle.render(vol, imp, dims, lut, cam, par, W, H, filter=filt)
            for frame, variant in enumerate((2, 2, 0, 1, 3)):
                got = _render_gpu(ctx, cam, par, variant)
                _check(got, ref, "tf %s (%d texels) layout %d filter %d %s: kernel %d, frame %d" % (name, lut.size // 4, layout, filt, mode, variant, frame))
                if name == "transparent" and kw.get("use_opacity", 1) == 1 and not kw.get("use_importance_coloring"):
                    hit = ref[0][..., 3] != 1.0
                    assert hit.any() and not got[0][hit].any(), "transparent table, %s, kernel %d: a ray gathered something" % (mode, variant)
                    assert got[2]["n_dense"] > 0
                cases += 1
    assert cases == 7 * 5


# ---- 2. threshold edges --------------------------------------------------------------------------------------------------

TERRACE_DIMS = (24, 20, 28)
TERRACE_BYTES = (40, 51, 128, 255)
THRESHOLD_MODES = [("plain", dict()), ("smoothed", dict(use_gaussian_smoothing=1)),
                   ("importance rendering", dict(use_importance_rendering=1, importance_check_ahead_steps=6))]


@pytest.mark.parametrize("pose", [(25.0, 15.0, 0.0), (140.0, 40.0, 6.0)], ids=["near-partly-off-screen", "far"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["plain", "smoothed", "importance-rendering"])
@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "linear"])
def test_threshold_edges(oracle, volym_lib, filt, mode, pose):
    """The terraced volume (plateaus of bytes 40, 51, 128, 255; 24x20x28) under prev(b/255), b/255, next(b/255), 0, -1, 1, next(1)
    and 1.5: the threshold byte of the table modes, the widened culling byte of the continuous ones, the distance field, the
    AABB table with its `nothing dense` entry, tile mask and tile depth (built on the second frame of a standing view).  All four
    kernels against the oracle; the default kernel's three frames of the standing view and a fourth without culling are bit-equal."""
    from volym_amd import _lib
    vol = common.terraced_volume(TERRACE_DIMS, TERRACE_BYTES)
    rng = np.random.default_rng(8)
    imp = np.where(rng.random(vol.size) < 0.1, 255, rng.integers(0, 200, vol.size)).astype(np.uint8)
    lut = oracle.tf_default_lut()
    W, H = 88, 56
    cam = oracle.benchmark_camera_uniforms(W / H, *pose)
    mode_name, kw = THRESHOLD_MODES[mode]
    thrs = common.byte_thresholds(TERRACE_BYTES)
    assert len(thrs) == 15
    dense = []
    with _ctx(W, H) as ctx:
        ctx.set_volume(vol, TERRACE_DIMS, filt)
        ctx.set_importances(imp, TERRACE_DIMS)
        ctx.set_transfer_function(lut)
        for thr in thrs:
            par = oracle.make_parameters(density_threshold=thr, raymarching_step_size=0.013, **kw)
            ref = oracle.render(vol, imp, TERRACE_DIMS, lut, cam, par, W, H, filter=filt)
            label = "terraced pose %s filter %d %s thr %r" % (pose, filt, mode_name, thr)
            dense.append(ref[2]["n_dense"])
            frames = []
            for frame in range(3):                   # a standing view: tile mask and tile depth from the second frame on
                got = _render_gpu(ctx, cam, par, 2)
                _check(got, ref, "%s kernel 2 frame %d" % (label, frame))
                frames.append(got)
            ctx.set_option(_lib.OPT_CULLING, 0)
            plain = _render_gpu(ctx, cam, par, 2)
            ctx.set_option(_lib.OPT_CULLING, 1)
            _check(plain, ref, "%s kernel 2 without culling" % label)
            for frame, got in enumerate(frames):
                assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(got[1], plain[1]), "%s: frame %d with culling differs from the frame without" % (label, frame)
            for variant in (0, 1, 3):
                _check(_render_gpu(ctx, cam, par, variant), ref, "%s kernel %d" % (label, variant))
            if thr > 1.0:                            # nothing can be dense: the background, (0,0,0,0) on rays that meet the cube
                for got in frames + [plain]:
                    assert got[2]["n_dense"] == 0 and not got[0][..., :3].any() and set(np.unique(got[0][..., 3])) <= {0.0, 1.0}, label
            if thr <= 0.0 and not kw.get("use_gaussian_smoothing"):      # (a smoothed sample with every tap outside the cube is NaN: not dense)
                for got in frames + [plain]:
                    assert got[2]["n_dense"] == got[2]["n_steps"] > 0, label
    print("%s filter %d pose %s: n_dense per threshold %s" % (mode_name, filt, pose, dense))
    if filt == 1 or kw.get("use_gaussian_smoothing"):
        # the edge is in the picture: some plateau's interpolated samples are dense one float below b/255 and not at b/255
        assert any(dense[3 * i] != dense[3 * i + 1] for i in range(3)), dense


# ---- 3. table and step changes between enqueued frames --------------------------------------------------------------------

SENTINEL = 0xA5
BURST = 20


def _burst_pairs():
    """(table name, step size) per frame of the burst.  Odd frames keep the step of the frame before and change the table; frames
    6, 12 and 18 keep the table and change the step; the other even frames change both.  Every frame needs new tables, so each
    frame slot's ring of 8 staging buffers goes round twice and a half."""
    pairs = []
    for k in range(BURST):
        name = pairs[-1][0] if k in (6, 12, 18) else TF_NAMES[(3 * k + 4) % len(TF_NAMES)]
        pairs.append((name, _STEPS[(k // 2) % len(_STEPS)]))
    for a, b in zip(pairs, pairs[1:]):
        assert a != b
    return pairs


@pytest.mark.parametrize("flight", [1, 2])
def test_tf_and_step_changes_between_enqueued_frames(oracle, volym_lib, bonsai64, flight):
    """A burst of 20 frames, each with a transfer function and a step size of its own, each into a sentinel-filled buffer of its
    own, enqueued with throttle(3) and no wait in between: the new tables travel through the ring of 8 pinned staging slots in
    stream order.  Afterwards every buffer holds the oracle's frame for its own pair (rgba8 within 1 LSB, no sentinel left); a
    frame drawn with its neighbour's tables is the failure this looks for, and the oracle's frames of neighbouring pairs are
    checked to differ by more than that.  Then one more frame with the last pair unchanged: the same bytes again."""
    import torch
    from volym_amd import _lib
    dims, vol, imp, dev_vol, dev_imp = bonsai64
    fam = _family()
    pairs = _burst_pairs()
    W, H = 200, 120
    cam = oracle.benchmark_camera_uniforms(W / H)
    cu = _lib.CameraUniforms.from_buffer_copy(bytes(cam))
    refs, pus = [], []
    for name, step in pairs:
        par = oracle.make_parameters(raymarching_step_size=step)
        refs.append(oracle.render(vol, imp, dims, fam[name], cam, par, W, H, want_f32=False)[1])
        pus.append(_lib.ParameterUniforms.from_buffer_copy(bytes(par)))
    for k in range(1, BURST):
        d = np.abs(refs[k].astype(np.int32) - refs[k - 1].astype(np.int32)).max(axis=-1)
        assert (d > 1).sum() >= 50, "frames %d and %d (%s, %s) are too much alike to tell a stale table" % (k - 1, k, pairs[k - 1], pairs[k])

    def buffer():
        b = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
        b.fill_(SENTINEL)
        return b

    from volym_amd import demo
    with demo.GpuContext(W, H, 0) as ctx:
        if flight == 2:
            ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 2)
        ctx.set_volume(dev_vol, dims, _lib.FILTER_NEAREST)
        ctx.set_importances(dev_imp, dims)
        ctx.set_transfer_function(fam["default"])
        bufs = [buffer() for _ in range(BURST + 1)]
        torch.cuda.synchronize()
        for k, (name, step) in enumerate(pairs):
            ctx.bind_output(None, bufs[k].data_ptr())
            ctx.set_transfer_function(fam[name])
            ctx.update(cu, pus[k])
            ctx.compute_pass()
            ctx.throttle(3)
        ctx.sync()
        assert ctx.frame_device_ptr() == bufs[BURST - 1].data_ptr()
        frames = [b.cpu().numpy().reshape(H, W, 4) for b in bufs[:BURST]]
        # the last pair once more, nothing changed: no new tables are due, and the frame is the same
        ctx.bind_output(None, bufs[BURST].data_ptr())
        ctx.update(cu, pus[BURST - 1])
        ctx.compute_pass()
        ctx.sync()
        again = bufs[BURST].cpu().numpy().reshape(H, W, 4)
    for k, got in enumerate(frames + [again]):
        j = min(k, BURST - 1)
        label = "flight %d frame %d (%s, step %r)" % (flight, k, pairs[j][0], pairs[j][1])
        assert not (got.reshape(-1, 4) == SENTINEL).all(axis=-1).any(), "%s: pixels nobody wrote" % label
        d = np.abs(got.astype(np.int32) - refs[j].astype(np.int32)).max(axis=-1)
        stale = ""
        if (d > 1).any():
            for other in (j - 1, j + 1):
                if 0 <= other < BURST and np.abs(got.astype(np.int32) - refs[other].astype(np.int32)).max() <= 1:
                    stale = "; it is the frame of pair %d %s" % (other, pairs[other])
        assert not (d > 1).any(), "%s: %d pixels differ from the oracle by more than 1 LSB (max %d)%s" % (label, int((d > 1).sum()), int(d.max()), stale)
    assert np.array_equal(again, frames[BURST - 1])


# ---- 4. the multi-GPU loop's table ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
def test_mgpu_transfer_function(oracle, volym_lib, bonsai64, world):
    """volym_mgpu_set_transfer_function with a 7-texel and an opaque table on virtual ranks: the assembled frame equals the bytes
    one context renders alone, for the first table and after the change to the second."""
    from volym_amd import _lib, demo, mgpu
    dims, vol, imp, dev_vol, dev_imp = bonsai64
    fam = _family()
    W, H = 310, 170
    cam = oracle.benchmark_camera_uniforms(W / H)
    par = oracle.make_parameters(raymarching_step_size=0.01)
    cu = _lib.CameraUniforms.from_buffer_copy(bytes(cam))
    pu = _lib.ParameterUniforms.from_buffer_copy(bytes(par))
    solo = {}
    with demo.GpuContext(W, H, 0) as c:
        c.set_volume(dev_vol, dims, 0)
        c.set_importances(dev_imp, dims)
        for name in ("random 7", "opaque"):
            c.set_transfer_function(fam[name])
            c.update(cu, pu)
            c.compute_pass()
            c.sync()
            solo[name] = c.read_rgba8()
            ref = oracle.render(vol, imp, dims, fam[name], cam, par, W, H, want_f32=False)[1]
            assert np.abs(solo[name].astype(np.int32) - ref.astype(np.int32)).max() <= 1, name
    assert not np.array_equal(solo["random 7"], solo["opaque"])
    with mgpu.MultiGpu(W, H, devices=[0] * world, transport=mgpu.COPY) as mg:
        mg.set_volume(dev_vol, dims, 0)
        mg.set_importances(dev_imp, dims)
        for name in ("random 7", "opaque", "random 7"):
            mg.set_transfer_function(fam[name])
            mg.update(cu, pu)
            mg.prepare(0)
            for frames in (1, 5):
                t = mg.run(frames, use_graph=False)
                assert t["overflowed"] == 0 and t["frames"] == frames
                assert np.array_equal(mg.read_rgba8(), solo[name]), (world, name, frames)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_alone(oracle, volym_lib):
    """A table of 0 or 257 texels or a NULL table, and a NaN or infinite threshold, are VOLYM_E_INVALID; after each the context
    renders the table and threshold it had, bit for bit the frame before the refusal."""
    from volym_amd import _lib
    vol = common.terraced_volume(TERRACE_DIMS, TERRACE_BYTES)
    imp = np.zeros(vol.size, np.uint8)
    lut = _family()["random 7"]
    thr = float(np.float32(51) / np.float32(255))
    W, H = 88, 56
    cam = oracle.benchmark_camera_uniforms(W / H, 25.0, 15.0, 0.0)
    par = oracle.make_parameters(density_threshold=thr, raymarching_step_size=0.013)
    ref = oracle.render(vol, imp, TERRACE_DIMS, lut, cam, par, W, H, filter=1)
    L = _lib.lib()
    table = np.zeros(4 * 257, np.uint8)
    tp = table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    cu = _lib.CameraUniforms.from_buffer_copy(bytes(cam))
    with _ctx(W, H) as ctx:
        ctx.set_volume(vol, TERRACE_DIMS, 1)
        ctx.set_importances(imp, TERRACE_DIMS)
        ctx.set_transfer_function(lut)
        before = _render_gpu(ctx, cam, par, 2)
        _check(before, ref, "before the refusals")

        def same_frame(what):
            ctx.compute_pass()                       # no update: whatever the refused call left behind
            ctx.sync()
            assert np.array_equal(_bits(ctx.read_rgba32f()), _bits(before[0])) and np.array_equal(ctx.read_rgba8(), before[1]), what
            got = _render_gpu(ctx, cam, par, 2)      # and through an update with the old uniforms
            assert np.array_equal(_bits(got[0]), _bits(before[0])) and np.array_equal(got[1], before[1]) and got[2] == before[2], what

        for what, call in (("0 texels", lambda: L.volym_set_transfer_function(ctx.handle, tp, 0)),
                           ("257 texels", lambda: L.volym_set_transfer_function(ctx.handle, tp, 257)),
                           ("NULL table", lambda: L.volym_set_transfer_function(ctx.handle, None, 256))):
            assert call() == _lib.E_INVALID, what
            same_frame(what)
        for bad in (float("nan"), float("inf"), float("-inf")):
            pu = _lib.ParameterUniforms.from_buffer_copy(bytes(oracle.make_parameters(density_threshold=bad, raymarching_step_size=0.013)))
            with pytest.raises(_lib.VolymError) as e:
                ctx.update(cu, pu)
            assert e.value.code == _lib.E_INVALID, bad
            same_frame("threshold %r" % bad)
