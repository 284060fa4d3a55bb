"""The step-size and look-ahead axes of the HIP ray-march against the CPU oracle, to the ends of what volym_update accepts:
raymarching_step_size from f32(1e-4) to 1 (rays of 40 000 samples and rays of none to four) and importance_check_ahead_steps
from 0 to 4096.  Every other rendering test draws with steps of 0.003 to 0.033 and counts of 1 to 11, 15 and 64.  The bar is
test_gpu_parity.py's on every pixel: the five counters identical, every channel within 1e-4, rgba8 within 1 LSB.  The cases are
tests/step_lookahead_cases.py's; tests/test_oracle_step_lookahead.py pins the oracle on them, and every case is drawn here only
after its oracle counters have passed the work cap.  Each comparison prints one line (case, oracle counters, largest float
error, largest rgba8 difference): profiles/step_lookahead_axes.txt is that output."""
import numpy as np
import pytest

from tests import common
from tests import step_lookahead_cases as SC
from tests.test_gpu_parity import _check, _ctx, _render_gpu

pytestmark = pytest.mark.gpu

STEPS = common.step_axis()
COUNTS = common.ahead_axis()
FRAMES = (2, 2, 0, 1, 3)            # the default kernel twice (the second frame runs depth-parallel items dealt from the first one's costs), then the others


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ref(oracle, case):
    """the oracle's frame of a case, once it is known to be under the work cap"""
    ref = SC.reference(oracle, case)
    assert ref[2]["n_vol"] + ref[2]["n_imp"] <= SC.WORK_CAP, case
    return ref


def _report(label, ref, err, du8):
    k = ref[2]
    print("AXES | %s | n_vol %d n_imp %d n_steps %d n_dense %d n_hit %d | max float error %.3g | max rgba8 difference %d"
          % (label, k["n_vol"], k["n_imp"], k["n_steps"], k["n_dense"], k["n_hit"], err, du8))


def _draw(ctx, oracle, case, variants, label):
    """a case under the given kernel variants, each frame against the oracle; -> the frames"""
    ref = _ref(oracle, case)
    cam, par = case.uniforms(oracle)
    worst, worst8, out = 0.0, 0, []
    for frame, variant in enumerate(variants):
        got = _render_gpu(ctx, cam, par, variant)
        err, _ = _check(got, ref, "%s: %r, kernel %d, frame %d" % (label, case, variant, frame))
        worst = max(worst, err)
        worst8 = max(worst8, int(np.abs(got[1].astype(np.int32) - ref[1].astype(np.int32)).max()))
        out.append(got)
    _report("%s: %r" % (label, case), ref, worst, worst8)
    return out


def _open(size, scene_name, filt, layout=0, options=()):
    from volym_amd import _lib, scene
    dims, vol, imp = SC.scene(scene_name)
    ctx = _ctx(*size)
    ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.set_volume(vol, dims, filt)
    ctx.set_importances(imp, dims)
    ctx.set_transfer_function(scene.default_lut())
    return ctx


# ---- 1. the step axis ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i,scene_name", SC.step_axis_ids(), ids=["%.9g-%s" % (STEPS[i], s) for i, s in SC.step_axis_ids()])
def test_step_axis(oracle, volym_lib, i, scene_name):
    """One step of the axis on one scene -- uniform noise, the saturated cube, the bonsai up to step 0.1 and the boxed noise from
    0.1 up --: plain, smoothed, importance straight and cone with 6 probes, both filters, both volume layouts, both poses, two
    frame sizes; the default kernel twice with every marched tile split into depth-parallel items on the second frame, then
    kernels 0, 1 and 3.  At the fine end the fixed-point colour sum has 10^4 terms and, on the bonsai, the closed-form replay of
    the empty-space steps runs 20 000 steps per binade.  At the coarse end a ray has 0 to 4 samples in all, fewer than a
    depth-parallel item has quarters.  The noise and the saturated cube fill every macro cell, so no empty step is replayed on
    them; the boxed noise has empty cells in front of its content, and there, from step 0.25 up, base / ulp(t) reaches 2^22 in
    replay_saturated, distance-field leaps are shorter than one step, and the tile-depth clip meets rays that end before their
    second sample.  (A list entry's cost is clamped to 65535 on the device; nothing here reads costs back, so whether a 1e-4
    frame reaches the clamp is not observed: costs steer scheduling only, and the frames are the same either way.)"""
    from volym_amd import _lib
    frames = 0
    for layout, size, per_filter in SC.step_axis_cases(i, scene_name):
        for filt, modes in per_filter:
            with _open(size, scene_name, filt, layout, ((_lib.OPT_DEPTH_PARALLEL, 1),)) as ctx:
                for mode, case in modes:
                    frames += len(_draw(ctx, oracle, case, FRAMES, "step axis, layout %d, %s" % (layout, mode)))
    assert frames == 2 * 2 * 4 * 5


@pytest.mark.parametrize("step", SC.culling_steps(), ids=["%.9g" % s for s in SC.culling_steps()])
def test_culling_changes_nothing_at_the_ends(oracle, volym_lib, step):
    """Steps 1e-4, 0.001, 0.1 and 1: three frames of a standing view with culling, cost feedback, tile mask and tile depth (from
    the second frame on) and the fine bounds grid are bit-equal in f32 to the frame of a context with culling and feedback off
    and the macro-cell grid for bounds, and to a frame with VOLYM_OPT_SETUP_IEEE = 1.  All against the oracle as well."""
    from volym_amd import _lib
    for mode, case in SC.culling_cases(step):
        cam, par = case.uniforms(oracle)
        with _open(case.size, case.scene, case.filt, 0, ((_lib.OPT_CULLING, 0), (_lib.OPT_COST_FEEDBACK, 0), (_lib.OPT_BOUNDS_CELLS, 0))) as ctx:
            plain = _draw(ctx, oracle, case, (2,), "no culling, %s" % mode)[0]
        with _open(case.size, case.scene, case.filt) as ctx:
            frames = _draw(ctx, oracle, case, (2, 2, 2), "culling, %s" % mode)
            ctx.set_option(_lib.OPT_SETUP_IEEE, 1)
            frames += _draw(ctx, oracle, case, (2, 2), "culling, plain divisions, %s" % mode)
            ctx.set_option(_lib.OPT_SETUP_IEEE, 0)
        for n, got in enumerate(frames):
            assert np.array_equal(_bits(got[0]), _bits(plain[0])) and np.array_equal(got[1], plain[1]) and got[2] == plain[2], \
                "%r, %s: frame %d with culling differs from the frame without" % (case, mode, n)


# ---- 2. the look-ahead axis --------------------------------------------------------------------------------------------------------

def _ahead(oracle, count, cone):
    from volym_amd import _lib
    variants = FRAMES if count <= 65 else (2, 2)
    cases = SC.ahead_cases(count, cone)
    assert len(cases) == (6 if count <= 256 else 3)
    for case in cases:
        with _open(case.size, case.scene, case.filt, 0, ((_lib.OPT_DEPTH_PARALLEL, 1),)) as ctx:
            _draw(ctx, oracle, case, variants, "look-ahead axis")


@pytest.mark.parametrize("cone", [0, 1], ids=["straight", "cone"])
@pytest.mark.parametrize("count", [c for c in COUNTS if c < 1000])
def test_ahead_axis(oracle, volym_lib, count, cone):
    """One look-ahead count, straight or cone, on the noise scene (an important voxel within a few probes of anywhere) and on
    the cup with its `middle` and `one voxel` importance maps (most look-aheads walk every probe), at steps 0.05 and 0.013
    (counts above 256 at 0.05 and 24x16 only); two frames of the default kernel with depth-parallel items, and kernels 0, 1 and
    3 for counts up to 65.  Count 0 divides by zero where the probe step is formed (the step is never used: there is no probe);
    counts above 64 make one cone job last hundreds of probe batches while other waves wait for its verdict."""
    _ahead(oracle, count, cone)


@pytest.mark.parametrize("cone", [0, 1], ids=["straight", "cone"])
@pytest.mark.parametrize("count", [c for c in COUNTS if c >= 1000])
def test_ahead_axis_thousands(oracle, volym_lib, count, cone):
    """Counts 1000, 4095 and 4096 (the last one accepted): a cone job of 8 x 4096 probes; every verdict must still arrive"""
    _ahead(oracle, count, cone)


# ---- 3. both fields change between enqueued frames -----------------------------------------------------------------------------------

SENTINEL = 0xA5


@pytest.mark.parametrize("flight", [1, 2])
def test_pairs_change_between_enqueued_frames(oracle, volym_lib, flight):
    """12 frames, each with a (step, count) pair of its own from both axes (step 1e-4 with counts <= 2), each into a
    sentinel-filled buffer of its own, enqueued with throttle(3) and no wait in between, straight and cone: every buffer holds
    the oracle's frame for its own pair, rgba8 within 1 LSB; the oracle's frames of neighbouring pairs differ by more than
    that, so a frame drawn with its neighbour's uniforms is seen."""
    import torch
    from volym_amd import _lib, demo, scene
    dims, vol, imp = SC.scene("noise")
    W, H = SC.SMALL
    pairs = SC.burst_pairs()
    for cone in (0, 1):
        cases = SC.burst_cases(cone)
        refs = [_ref(oracle, c)[1] for c in cases]
        for k in range(1, len(cases)):
            assert (np.abs(refs[k].astype(np.int32) - refs[k - 1].astype(np.int32)).max(axis=-1) > 1).sum() >= 10, (pairs[k - 1], pairs[k])
        with demo.GpuContext(W, H, 0) as ctx:
            if flight == 2:
                ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 2)
            ctx.set_volume(vol, dims, 0)
            ctx.set_importances(imp, dims)
            ctx.set_transfer_function(scene.default_lut())
            bufs = [torch.full((W * H * 4,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in cases]
            torch.cuda.synchronize()
            for k, case in enumerate(cases):
                cam, par = case.uniforms(oracle)
                ctx.bind_output(None, bufs[k].data_ptr())
                ctx.update(_lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par)))
                ctx.compute_pass()
                ctx.throttle(3)
            ctx.sync()
            frames = [b.cpu().numpy().reshape(H, W, 4) for b in bufs]
        for k, got in enumerate(frames):
            label = "flight %d cone %d frame %d (step %r, count %d)" % (flight, cone, k, pairs[k][0], pairs[k][1])
            assert not (got.reshape(-1, 4) == SENTINEL).all(axis=-1).any(), "%s: pixels nobody wrote" % label
            d = np.abs(got.astype(np.int32) - refs[k].astype(np.int32)).max(axis=-1)
            stale = ""
            if (d > 1).any():
                for other in (k - 1, k + 1):
                    if 0 <= other < len(cases) and np.abs(got.astype(np.int32) - refs[other].astype(np.int32)).max() <= 1:
                        stale = "; it is the frame of pair %d %s" % (other, pairs[other])
            assert not (d > 1).any(), "%s: %d pixels differ from the oracle by more than 1 LSB (max %d)%s" % (label, int((d > 1).sum()), int(d.max()), stale)
            _report(label, _ref(oracle, cases[k]), float("nan"), int(d.max()))


# ---- 4. pick ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", SC.pick_steps(), ids=["%.9g" % s for s in SC.pick_steps()])
def test_pick_follows_the_step(oracle, volym_lib, step):
    """volym_pick_pass over the whole 37x23 frame of the boxed noise (empty macro cells in front of the content) at steps 0.001,
    0.1 and 1, alpha_min 0 and 0.5, against tests/pick_reference.py, the records byte-equal: in a fresh context before any frame
    (a direct march), and after its first frame (leaps through the distance field, which is not all zeros on this scene)."""
    from tests import pick_reference as R
    from volym_amd import _lib
    case = SC.pick_case(step)
    _ref(oracle, case)
    dims, vol, imp = SC.scene(case.scene)
    W, H = case.size
    cam, par = case.uniforms(oracle)
    for a_min in (0.0, 0.5):
        ref = R.frame(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H, a_min, filter=0)
        assert not ref["near"].any() and (ref["picks"]["status"] == 2).sum() >= 16, (step, a_min)
        with _open((W, H), case.scene, 0) as ctx:
            ctx.update(_lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par)))
            for when in ("before any frame", "after the first frame"):
                ctx.pick_pass(None, a_min)
                got = ctx.read_picks()
                assert got.shape == ref["picks"].shape
                assert np.array_equal(got.view(np.uint8), ref["picks"].view(np.uint8)), (step, a_min, when)
                if when == "before any frame":
                    ctx.compute_pass()
                    ctx.sync()


# ---- 5. the multi-GPU loop -----------------------------------------------------------------------------------------------------------

def test_mgpu_virtual_ranks_at_the_ends(oracle, volym_lib):
    """Three virtual ranks, steps 0.001 and 0.1, cone look-ahead of 25: the assembled frame equals the bytes one context renders
    alone, which are within 1 LSB of the oracle's."""
    from volym_amd import _lib, demo, mgpu, scene
    dims, vol, imp = SC.scene("noise")
    cases = SC.mgpu_cases()
    W, H = cases[0].size
    solo = []
    with demo.GpuContext(W, H, 0) as c:
        c.set_volume(vol, dims, 0)
        c.set_importances(imp, dims)
        c.set_transfer_function(scene.default_lut())
        for case in cases:
            cam, par = case.uniforms(oracle)
            c.update(_lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par)))
            c.compute_pass()
            c.sync()
            solo.append(c.read_rgba8())
            d = int(np.abs(solo[-1].astype(np.int32) - _ref(oracle, case)[1].astype(np.int32)).max())
            assert d <= 1, (case, d)
            _report("multi-GPU solo frame: %r" % case, _ref(oracle, case), float("nan"), d)
    assert not np.array_equal(solo[0], solo[1])
    with mgpu.MultiGpu(W, H, devices=[0] * 3, transport=mgpu.COPY) as mg:
        mg.set_volume(vol, dims, 0)
        mg.set_importances(imp, dims)
        mg.set_transfer_function(scene.default_lut())
        for case, want in list(zip(cases, solo)) + [(cases[0], solo[0])]:
            cam, par = case.uniforms(oracle)
            mg.update(_lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par)))
            mg.prepare(0)
            for frames in (1, 4):
                t = mg.run(frames, use_graph=False)
                assert t["overflowed"] == 0 and t["frames"] == frames
                assert np.array_equal(mg.read_rgba8(), want), (case, frames)


# ---- 6. the GUI's ends -----------------------------------------------------------------------------------------------------------------

NOISE_SEGMENTS = [{"id": "speckle", "name": "Speckle", "index": 0, "label_value": 1, "importance": 255}]


def test_gui_ends(oracle, volym_lib):
    """scene.State under its GUI object, as tests/test_flythrough.py drives it: step_size(0.0) and step_size(5.0) clamp to 0.001
    and 0.1, look_ahead_steps(0) and look_ahead_steps(99) to 2 and 25.  After each call one frame through the demo mirror, rgba8
    within 1 LSB of the oracle on the uniforms State produced."""
    from volym_amd import demo, flythrough as ft, scene
    rng = np.random.default_rng(33)
    dims = SC.NOISE_DIMS
    n = dims[0] * dims[1] * dims[2]
    raw = rng.integers(0, 256, n, dtype=np.uint8)
    labels = (rng.integers(0, 4, n) == 0).astype(np.uint8)
    vol, imp = common.oracle_scene(oracle, raw, labels, NOISE_SEGMENTS, dims)
    W, H = SC.SIZES[0]
    state = scene.State.with_parameters(W / H, scene.StateParameters.benchmark())
    gui = ft.Gui(state)
    gui.density_threshold(SC.NOISE_THRESHOLD)
    gui.importance_rendering(1)
    gui.cone_importance_check(1)
    state.process_mouse(-100.0, 40.0)
    state.update()
    seen = []
    with demo.GpuContext(W, H, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels, segments=NOISE_SEGMENTS, dims=dims)
        for call, arg in (("step_size", 0.0), ("look_ahead_steps", 0), ("step_size", 5.0), ("look_ahead_steps", 99)):
            getattr(gui, call)(arg)
            state.update()
            d.update_gpu_state(ctx, state)
            d.compute_pass(ctx)
            ctx.sync()
            got = ctx.read_rgba8()
            cam = oracle.CameraUniforms.from_buffer_copy(bytes(state.camera_uniforms()))
            par = oracle.Parameters.from_buffer_copy(bytes(state.parameter_uniforms()))
            seen.append((float(par.raymarching_step_size), int(par.importance_check_ahead_steps)))
            assert par.use_importance_rendering == 1 and par.use_cone_importance_check == 1
            ref = oracle.render(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H)
            assert ref[2]["n_vol"] + ref[2]["n_imp"] <= SC.WORK_CAP
            du8 = int(np.abs(got.astype(np.int32) - ref[1].astype(np.int32)).max())
            assert du8 <= 1, ("%s(%r)" % (call, arg), seen[-1], du8)
            _report("GUI %s(%r): step %r, count %d" % (call, arg, seen[-1][0], seen[-1][1]), ref, float("nan"), du8)
    f = lambda v: float(np.float32(v))
    assert seen[0][0] == f(0.001) and seen[1] == (f(0.001), 2) and seen[2] == (f(0.1), 2) and seen[3] == (f(0.1), 25), seen


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_alone(oracle, volym_lib):
    """A step one float below f32(1e-4) or above 1, 0, -0.01, NaN and +inf, and counts 4097 and 0xFFFFFFFF are VOLYM_E_INVALID;
    after each the next compute_pass gives the bytes of the frame before it.  f32(1e-4), 1, 0 and 4096 are accepted."""
    from volym_amd import _lib
    case, lowest, highest = SC.refusal_cases()
    cam, par = case.uniforms(oracle)
    cu = _lib.CameraUniforms.from_buffer_copy(bytes(cam))
    with _open(case.size, "noise", 0) as ctx:
        before = _draw(ctx, oracle, case, (2,), "before the refusals")[0]

        def same_frame(what):
            ctx.compute_pass()                       # no update: whatever the refused call left behind
            ctx.sync()
            assert np.array_equal(_bits(ctx.read_rgba32f()), _bits(before[0])) and np.array_equal(ctx.read_rgba8(), before[1]), what

        bad = [dict(raymarching_step_size=s) for s in common.refused_steps()] + [dict(importance_check_ahead_steps=n) for n in (4097, 0xFFFFFFFF)]
        assert len(bad) == 8
        for kw in bad:
            p = dict(case.par)
            p.update(kw)
            with pytest.raises(_lib.VolymError) as e:
                ctx.update(cu, _lib.ParameterUniforms.from_buffer_copy(bytes(oracle.make_parameters(**p))))
            assert e.value.code == _lib.E_INVALID, kw
            same_frame(kw)
        for accepted in (lowest, highest):         # f32(1e-4) with no probe at all, and 1 with 4096 probes
            _draw(ctx, oracle, accepted, (2,), "accepted")
