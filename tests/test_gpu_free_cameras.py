"""The camera axis of the HIP ray-march against the CPU oracle: eyes inside the cube and inside the matter, panned, rolled, narrow
and wide, near planes from 0.001 to 0.5, the cube off screen or behind the eye, and uniforms whose camera_position is not the
centre of projection of their matrix.  Every other rendering test looks through an orbit about the cube's centre at distance 1 to
10 with fovy 90 and znear 0.01, and every culling device -- projected hulls, the ray pool's rectangle, tile mask, tile depth
bounds, AABB clip -- is computed from the camera.  The bar is test_gpu_parity.py's on every pixel: the five counters identical,
every channel within 1e-4, rgba8 within 1 LSB.  The cases are tests/free_camera_cases.py's; tests/test_oracle_free_cameras.py pins
the oracle on them.  Each comparison prints one line (group, case, mode, largest float error, largest rgba8 difference, what the
view's culling was): profiles/free_cameras.txt is that output."""
import numpy as np
import pytest

from tests import free_camera_cases as FC
from tests.test_gpu_parity import _check, _ctx, _render_gpu

pytestmark = pytest.mark.gpu

CASES = FC.all_cases()
IDS = [c.name for c in CASES]
MODES = [m for m, _ in FC.MODES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _open(case, filt=0, layout=0, options=()):
    from volym_amd import _lib, scene
    dims, vol, imp = FC.scene(case.scene)
    ctx = _ctx(*case.size)
    ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.set_volume(vol, dims, filt)
    ctx.set_importances(imp, dims)
    ctx.set_transfer_function(scene.default_lut())
    return ctx


def _culling_of(ctx):
    """what a standing view's second frame runs with: "mask + depth" (and how many of the frame's 8x8 tiles are marched) or "none" """
    from volym_amd import _lib
    try:
        mask, near, far = ctx.read_tile_bounds()
    except _lib.VolymError as e:
        assert e.code == _lib.E_STATE
        return "no mask"
    return "mask %d of %d tiles, depth bounds %s" % (int(mask.sum()), mask.size, "yes" if np.isfinite(far[mask]).all() and mask.any() else "no")


def _draw(ctx, oracle, case, mode, variants, group, filt=0):
    """a case under a mode and the given kernel variants, each frame against the oracle; -> the frames"""
    ref = FC.reference(oracle, case, mode, filt)
    cam, par = case.uniforms(oracle), case.parameters(oracle, mode)
    worst, worst8, out = 0.0, 0, []
    for frame, variant in enumerate(variants):
        got = _render_gpu(ctx, cam, par, variant)
        err, _ = _check(got, ref, "%s: %r, %s, kernel %d, frame %d" % (group, case, mode, variant, frame))
        worst = max(worst, err)
        worst8 = max(worst8, int(np.abs(got[1].astype(np.int32) - ref[1].astype(np.int32)).max()))
        out.append(got)
    print("FREE | %s | %r | %s | kernels %s | n_hit %d n_steps %d n_dense %d | max float error %.3g | max rgba8 difference %d | %s"
          % (group, case, mode, "".join(str(v) for v in variants), ref[2]["n_hit"], ref[2]["n_steps"], ref[2]["n_dense"], worst, worst8,
             _culling_of(ctx) if len(variants) > 1 and variants[-1] == 2 else "-"))
    return out


# ---- 1. no culling, no lists ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_direct_kernel(oracle, volym_lib, case):
    """variant 0: every reference fetch issued, nothing culled.  Says that the ray set-up and the march take these cameras."""
    with _open(case) as ctx:
        for mode in MODES:
            _draw(ctx, oracle, case, mode, (0,), "direct")


# ---- 2. the first frame of every other kernel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_first_frames(oracle, volym_lib, case):
    """variants 1, 2 and 3 on a view's first frame: distance-field leaps, hulls, AABB clip and the ray pool's rectangle, no mask"""
    with _open(case) as ctx:
        for mode in MODES:
            for variant in (1, 2, 3):
                _draw(ctx, oracle, case, mode, (variant,), "first frame")


# ---- 3. standing views -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_standing_view(oracle, volym_lib, case):
    """variant 2 for three frames with settle() between them and depth-parallel items: the second and third frames run the re-dealt
    list, the tile mask and the depth bounds.  All three against the oracle, and bit-equal to each other.  A displaced eye further
    off than the slack has no mask on its standing frames; the one inside the slack, and the consistent cameras they were moved
    from, have one."""
    from volym_amd import _lib
    with _open(case, options=((_lib.OPT_DEPTH_PARALLEL, 1),)) as ctx:
        for mode in MODES:
            frames = _draw(ctx, oracle, case, mode, (2, 2, 2), "standing")
            for n, got in enumerate(frames[1:], start=2):
                assert np.array_equal(_bits(got[0]), _bits(frames[0][0])) and np.array_equal(got[1], frames[0][1]), \
                    "%r, %s: frame %d of the standing view differs from frame 1" % (case, mode, n)
            if case.shift is not None or case.name in (FC.DISPLACED_BASE.name, FC.DISPLACED_BASE_NEAR.name):
                has_mask = _culling_of(ctx) != "no mask"
                assert has_mask == case.culled, "%r, %s: culling %s" % (case, mode, "in force" if has_mask else "not in force")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_culling_and_feedback_change_nothing(oracle, volym_lib, case):
    """tests/test_gpu_parity.py::test_culling_and_feedback_leave_pixels_unchanged on these cameras: three frames each with culling
    off, culling on without feedback and culling on with feedback are one frame, bit for bit; that frame against the oracle"""
    from volym_amd import _lib
    with _open(case) as ctx:
        ctx.set_option(_lib.OPT_KERNEL, 2)
        for mode in MODES:
            cam, par = case.uniforms(oracle), case.parameters(oracle, mode)
            cu = _lib.CameraUniforms.from_buffer_copy(bytes(cam))
            pu = _lib.ParameterUniforms.from_buffer_copy(bytes(par))
            frames = []
            for cull, feedback in ((0, 0), (1, 0), (1, 1)):
                ctx.set_option(_lib.OPT_CULLING, cull)
                ctx.set_option(_lib.OPT_COST_FEEDBACK, feedback)
                ctx.update(cu, pu)
                for _ in range(3):
                    ctx.compute_pass()
                    ctx.sync()
                    ctx.settle()
                    frames.append((ctx.read_rgba8(), ctx.read_rgba32f()))
            for n, (u, f) in enumerate(frames[1:], start=1):
                assert np.array_equal(u, frames[0][0]) and np.array_equal(_bits(f), _bits(frames[0][1])), \
                    "%r, %s: frame %d (culling %d, feedback %d) differs from the frame without culling" % (case, mode, n % 3, n // 3 > 0, n // 3 > 1)
            ref = FC.reference(oracle, case, mode)
            _check((frames[-1][1], frames[-1][0], ctx.stats_pass()), ref, "culling and feedback: %r, %s" % (case, mode))


# ---- 4. layouts, filter, frames in flight ------------------------------------------------------------------------------------------------

SUBSET = [FC.by_name(n) for n in FC.SUBSET + FC.RAGGED_NAMES]


@pytest.mark.parametrize("case", SUBSET, ids=[c.name for c in SUBSET])
def test_bricked_layout(oracle, volym_lib, case):
    from volym_amd import _lib
    with _open(case, layout=1, options=((_lib.OPT_DEPTH_PARALLEL, 1),)) as ctx:
        for mode in MODES:
            _draw(ctx, oracle, case, mode, (0, 1, 3, 2, 2), "bricked")


@pytest.mark.parametrize("case", SUBSET, ids=[c.name for c in SUBSET])
def test_linear_filter(oracle, volym_lib, case):
    from volym_amd import _lib
    with _open(case, filt=1, options=((_lib.OPT_DEPTH_PARALLEL, 1),)) as ctx:
        for mode in MODES:
            _draw(ctx, oracle, case, mode, (0, 1, 3, 2, 2), "linear filter", filt=1)


@pytest.mark.parametrize("case", SUBSET, ids=[c.name for c in SUBSET])
def test_two_frames_in_flight(oracle, volym_lib, case):
    """frames alternate between two slots; each slot builds its mask and bounds on its own second frame: six frames"""
    from volym_amd import _lib
    with _open(case, options=((_lib.OPT_FRAMES_IN_FLIGHT, 2), (_lib.OPT_DEPTH_PARALLEL, 1))) as ctx:
        for mode in MODES:
            frames = _draw(ctx, oracle, case, mode, (2,) * 6, "two frames in flight")
            for n, got in enumerate(frames[1:], start=2):
                assert np.array_equal(_bits(got[0]), _bits(frames[0][0])), "%r, %s: frame %d differs from frame 1" % (case, mode, n)


# ---- 5. the devices, not their fallback -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FC.BOUNDS_NAMES)
def test_mask_and_bounds_are_in_force(oracle, volym_lib, name):
    """An eye inside the cube and outside the occupied cells' AABB, and a panned camera whose picture two frame edges cut: the
    standing frame has a tile mask that marches some tiles and not all, and depth bounds that are real ranges, nearer than the
    cube's diagonal and starting beyond the eye; its pixels are the first frame's and the oracle's."""
    case = FC.by_name(name)
    W, H = case.size
    with _open(case) as ctx:
        frames = _draw(ctx, oracle, case, "base", (2, 2), "bounds in force")
        assert np.array_equal(_bits(frames[1][0]), _bits(frames[0][0]))
        mask, near, far = ctx.read_tile_bounds()
    live = mask[:(H + 7) // 8, :(W + 7) // 8]
    assert live.any() and not live.all(), "%r: %d of %d tiles marched" % (case, int(live.sum()), live.size)
    seen = FC.non_constant(FC.reference(oracle, case)[0])
    for ty, tx in np.argwhere(~live):
        assert not seen[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].any(), "%r: tile (%d, %d) is masked out and shows matter" % (case, tx, ty)
    assert np.isfinite(near[mask]).all() and np.isfinite(far[mask]).all(), "a marched tile without depth bounds"
    assert (near[mask] <= far[mask]).all() and (far[mask] < 1.8).all() and (near[mask] > 0.05).any()
    assert (far[~mask] == 0).all()


ORBITS = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.5), (-120.0, -60.0, 2.0), (90.0, 89.0, 9.0), (40.0, 25.0, 3.0), (10.0, -70.0, 0.2), (-150.0, -40.0, 0.5)]


def test_orbit_cameras_keep_their_culling(oracle, volym_lib):
    """the consistent f32 cameras the rest of the suite draws with (distance 1 to 10) still get their mask and bounds on the second
    frame, at 200x120 and at the headline's 1920x1080"""
    from volym_amd import _lib, scene
    dims, vol, imp = FC.scene("bonsai")
    par = _lib.ParameterUniforms.from_buffer_copy(bytes(oracle.make_parameters()))
    for W, H, poses in ((200, 120, ORBITS), (1920, 1080, ORBITS[:1] + ORBITS[3:4])):
        with _ctx(W, H) as ctx:
            ctx.set_volume(vol, dims, 0)
            ctx.set_importances(imp, dims)
            ctx.set_transfer_function(scene.default_lut())
            for pose in poses:
                ctx.update(_lib.CameraUniforms.from_buffer_copy(bytes(oracle.benchmark_camera_uniforms(W / H, *pose))), par)
                for _ in range(2):
                    ctx.compute_pass()
                    ctx.sync()
                mask, near, far = ctx.read_tile_bounds()
                assert mask.any() and not mask.all() and np.isfinite(far[mask]).all(), (W, H, pose)


# ---- 6. pick and projection ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FC.PICK_NAMES)
def test_pick(oracle, volym_lib, name):
    """volym_pick_pass over the whole frame against tests/pick_reference.py by the criteria of tests/test_gpu_pick.py: before any
    frame (a direct march) and after the first (leaps through the distance field)"""
    from tests import pick_reference as R
    from tests.test_gpu_pick import _compare
    from volym_amd import _lib
    case = FC.by_name(name)
    dims, vol, imp = FC.scene(case.scene)
    W, H = case.size
    cam, par = case.uniforms(oracle), case.parameters(oracle, "base")
    for a_min in (0.0, 0.5):
        ref = R.frame(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H, a_min, filter=0)
        assert (ref["picks"]["status"] == 2).sum() >= 16, (case, a_min)
        with _open(case) as ctx:
            ctx.update(_lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par)))
            for when in ("before any frame", "after the first frame"):
                ctx.pick_pass(None, a_min)
                _compare((case.name, a_min, when), ctx.read_picks(), ref)
                if when == "before any frame":
                    ctx.compute_pass()
                    ctx.sync()


@pytest.mark.parametrize("name", FC.PICK_NAMES)
def test_projection(oracle, volym_lib, name):
    """volym_project_pass against scene.project_frame, records and image byte for byte (tests/test_gpu_project.py's criteria)"""
    from tests.test_gpu_project import _same_image, _same_records
    from volym_amd import _lib, scene
    case = FC.by_name(name)
    dims, vol, imp = FC.scene(case.scene)
    W, H = case.size
    cam, par = case.uniforms(oracle), case.parameters(oracle, "base")
    cu = _lib.CameraUniforms.from_buffer_copy(bytes(cam))
    for mode in ("MAX", "MEAN"):
        p = scene.Projection(FC.STEP, getattr(_lib, "PROJECT_" + mode))
        want, want_image = scene.project_frame(vol, dims, cu, W, H, p, lut=scene.default_lut())
        assert (want["status"] == 2).sum() >= 16, (case, mode)
        with _open(case) as ctx:
            ctx.update(cu, _lib.ParameterUniforms.from_buffer_copy(bytes(par)))
            for when in ("before any frame", "after the first frame"):
                ctx.project_pass(p, own_image=True)
                _same_records((case.name, mode, when), ctx.read_projection(), want)
                _same_image((case.name, mode, when), ctx.read_projection_image(), want_image)
                if when == "before any frame":
                    ctx.compute_pass()
                    ctx.sync()
