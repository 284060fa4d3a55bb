"""Volumes of 256 texels on every axis: volym_raymarch_cube256_kernel (VOLYM_OPT_TEXEL_BYTES = 1, the default) against the general
kernel (0) and the CPU oracle.

The twin's texel address is three saturating byte conversions side by side (raymarch_device.h, texel256_insert), the general
kernel's a floor-and-convert, an integer clamp and two multiply-adds.  The two differ only where a coordinate leaves 0..255, so
the volume is dense in the outer four texel layers of all six faces (random bytes: the classes flip from sample to sample) with a few
blobs inside, and the cameras make samples, speculative samples and gradient taps (+-2.56 texels) cross every face: one looks at
a corner from outside, one has its eye inside the cube, one sits 0.02 outside a face and looks along it.  256^3 is the smallest
volume the twin runs on, so the frames are small: 96x64, and 37x23 for the ragged one.

Every case is rendered under both option values: the frames must be byte-equal, the twin must have run under 1 and not under 0,
and the 0 frame must meet the suite's bar against the oracle (tests/test_gpu_parity.py _check: every channel within 1e-4, rgba8
within 1 LSB, the five counters identical through the stats pass)."""
import numpy as np
import pytest

from tests import free_camera_cases as FC
from tests.test_gpu_parity import _check, _ctx

DIMS = (256, 256, 256)
SHELL = 4
CAMERAS = {
    "corner from outside": dict(position=(1.15, 1.1, 1.2), target=(0.5, 0.5, 0.5)),
    "eye inside the cube": dict(position=(0.5, 0.75, 0.85), target=(0.5, 0.35, 0.4)),
    "0.02 outside a face, looking along it": dict(position=(0.35, 0.4, 1.02), target=(0.9, 0.45, 0.97)),
}
CASES = [FC.Case(name, "shell256", (96, 64), cam, {}) for name, cam in CAMERAS.items()]
RAGGED = FC.Case("corner from outside, ragged frame", "shell256", FC.RAGGED, CAMERAS["corner from outside"], {})
IDS = [c.name for c in CASES + [RAGGED]]

_made = {}


def shell_volume(dims):
    """prepared bytes (x fastest): random bytes in the outer SHELL texel layers of every face, three smooth blobs inside, 0 elsewhere"""
    if dims not in _made:
        nx, ny, nz = dims
        rng = np.random.default_rng(256)
        v = np.zeros((nz, ny, nx), np.uint8)
        z, y, x = np.ogrid[:nz, :ny, :nx]
        for cx, cy, cz, r in ((0.3, 0.35, 0.4, 0.12), (0.7, 0.6, 0.55, 0.16), (0.5, 0.2, 0.75, 0.08)):
            d = np.sqrt(((x + 0.5) / nx - cx) ** 2 + ((y + 0.5) / ny - cy) ** 2 + ((z + 0.5) / nz - cz) ** 2)
            v = np.maximum(v, np.where(d < r, 60 + 190 * (1.0 - d / r), 0).astype(np.uint8))
        shell = np.ones((nz, ny, nx), bool)
        shell[SHELL:nz - SHELL, SHELL:ny - SHELL, SHELL:nx - SHELL] = False
        v[shell] = rng.integers(0, 256, int(shell.sum()), dtype=np.uint8)
        _made[dims] = (v.ravel(), np.zeros(nx * ny * nz, np.uint8))
    return _made[dims]


_refs = {}


def reference(O, case, dims=DIMS):
    """the C oracle's (rgba32f, rgba8, counters) of a case; rendered once, shared, never written to"""
    key = (case.name, dims)
    if key not in _refs:
        vol, imp = shell_volume(dims)
        W, H = case.size
        f, u, k = O.render(vol, imp, dims, O.tf_default_lut(), case.uniforms(O), case.parameters(O, "base"), W, H)
        f.setflags(write=False)
        u.setflags(write=False)
        _refs[key] = (f, u, k)
    return _refs[key]


def faces_crossed(u, W, H):
    """[H, W] int pairs: the face (2 * axis + side) through which each pixel's ray enters the cube (-1: the eye is inside, or a miss)
    and the face through which it leaves (-1: a miss); float64 restatement of wgsl:221-241"""
    ivp = np.array([[u.inverse_view_proj[c][r] for c in range(4)] for r in range(4)], np.float64)
    eye = np.array([u.camera_position[i] for i in range(3)], np.float64)
    gy, gx = np.mgrid[:H, :W]
    ndc = np.stack([gx / W * 2.0 - 1.0, 1.0 - gy / H * 2.0, np.zeros((H, W)), np.ones((H, W))], axis=-1)
    wp = ndc @ ivp.T
    d = wp[..., :3] / wp[..., 3:] - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (0.0 - eye) / d, (1.0 - eye) / d
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    t_in, t_out = lo.max(axis=-1), hi.min(axis=-1)
    hit = t_out > np.maximum(t_in, 0.0)
    a_in, a_out = lo.argmax(axis=-1), hi.argmin(axis=-1)
    side_in = np.take_along_axis(t1, a_in[..., None], -1)[..., 0] < np.take_along_axis(t0, a_in[..., None], -1)[..., 0]
    side_out = np.take_along_axis(t1, a_out[..., None], -1)[..., 0] > np.take_along_axis(t0, a_out[..., None], -1)[..., 0]
    enter = np.where(hit & (t_in > 0.0), 2 * a_in + side_in, -1)
    leave = np.where(hit, 2 * a_out + side_out, -1)
    return enter, leave


@pytest.mark.parametrize("case", CASES + [RAGGED], ids=IDS)
def test_oracle_frames_cross_three_faces(oracle, case):
    """no GPU: the coloured pixels of the oracle's frame belong to rays that enter or leave the cube through at least three different
    faces, and there are enough of them -- a camera that clips nothing cannot pass the device tests for the wrong reason"""
    f32, _, k = reference(oracle, case)
    coloured = FC.non_constant(f32)
    W, H = case.size
    assert coloured.sum() >= W * H // 8 and k["n_dense"] >= 1000, (case, int(coloured.sum()), k)
    enter, leave = faces_crossed(case.uniforms(oracle), W, H)
    faces = (set(enter[coloured].tolist()) | set(leave[coloured].tolist())) - {-1}
    print("%r: %d coloured pixels, faces crossed %s, n_steps %d, n_dense %d" % (case, int(coloured.sum()), sorted(faces), k["n_steps"], k["n_dense"]))
    assert len(faces) >= 3, (case, faces)


def _open(case, dims=DIMS, options=()):
    from volym_amd import _lib, scene
    vol, imp = shell_volume(dims)
    ctx = _ctx(*case.size)
    ctx.set_option(_lib.OPT_VOLUME_LAYOUT, 0)
    ctx.set_option(_lib.OPT_KERNEL, 2)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.set_volume(vol, dims, 0)
    ctx.set_importances(imp, dims)
    ctx.set_transfer_function(scene.default_lut())
    return ctx


def _frames(ctx, oracle, case, n, twin_expected=True):
    """n frames of a standing view under VOLYM_OPT_TEXEL_BYTES 1, then n under 0, settle() between them -> the 0 arm's last frame and
    its counters.  All 2 n frames must be one frame, bit for bit."""
    from volym_amd import _lib
    cu = _lib.CameraUniforms.from_buffer_copy(bytes(case.uniforms(oracle)))
    pu = _lib.ParameterUniforms.from_buffer_copy(bytes(case.parameters(oracle, "base")))
    first, last = None, None
    for value in (1, 0):
        ctx.set_option(_lib.OPT_TEXEL_BYTES, value)
        ctx.update(cu, pu)
        for i in range(n):
            ctx.compute_pass()
            ctx.sync()
            ctx.settle()
            assert ctx.texel_bytes_in_use() == (twin_expected and value == 1), "%r: option %d, frame %d ran the wrong kernel" % (case, value, i)
            last = (ctx.read_rgba32f(), ctx.read_rgba8())
            if first is None:
                first = last
            assert np.array_equal(last[1], first[1]) and np.array_equal(last[0].view(np.uint32), first[0].view(np.uint32)), \
                "%r: frame %d under VOLYM_OPT_TEXEL_BYTES = %d differs from the first frame under 1" % (case, i, value)
    return last[0], last[1], ctx.stats_pass()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + [RAGGED], ids=IDS)
def test_twin_equals_general_kernel_and_oracle(oracle, volym_lib, case):
    """the first frame of a view (the centre-first list, adaptive depth-parallel items) under either option value"""
    with _open(case) as ctx:
        _check(_frames(ctx, oracle, case, 1), reference(oracle, case), "first frame: %r" % case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS[:3])
def test_standing_view_split_in_depth(oracle, volym_lib, case):
    """three standing frames with cost feedback and every marched tile split into depth-parallel items (VOLYM_OPT_DEPTH_PARALLEL = 1,
    the switch of the parity tests): the second and third run the re-dealt list, the tile mask and the depth bounds"""
    from volym_amd import _lib
    with _open(case, options=((_lib.OPT_DEPTH_PARALLEL, 1),)) as ctx:
        _check(_frames(ctx, oracle, case, 3), reference(oracle, case), "standing, depth-parallel: %r" % case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS[:3])
def test_standing_view_with_cost_feedback(oracle, volym_lib, case):
    """three standing frames with cost feedback and the default, adaptive split"""
    with _open(case) as ctx:
        _check(_frames(ctx, oracle, case, 3), reference(oracle, case), "standing: %r" % case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS[:3])
def test_two_frames_in_flight(oracle, volym_lib, case):
    """frames alternate between two slots: four frames per option value, two per slot"""
    from volym_amd import _lib
    with _open(case, options=((_lib.OPT_FRAMES_IN_FLIGHT, 2), (_lib.OPT_DEPTH_PARALLEL, 1))) as ctx:
        _check(_frames(ctx, oracle, case, 4), reference(oracle, case), "two frames in flight: %r" % case)


@pytest.mark.gpu
def test_a_volume_of_255_slices_runs_the_general_kernel(oracle, volym_lib):
    """256 x 256 x 255: the twin is not taken whatever the option says; same frame, and the oracle's"""
    dims, case = (256, 256, 255), CASES[0]
    with _open(case, dims=dims) as ctx:
        _check(_frames(ctx, oracle, case, 2, twin_expected=False), reference(oracle, case, dims), "256 x 256 x 255: %r" % case)


@pytest.mark.gpu
def test_texel_selftest(volym_lib):
    """volym_selftest_texel256: the byte conversion the library is built with gives clamp(floor(x), 0, 255) for every float of
    magnitude in [2^-10, 512), both signs, +-0, the denormal ends, +-2^40 and +-inf (NaN is reported apart: no position is NaN)"""
    with _ctx(16, 16) as ctx:
        bad, bad_nan, bare, bare_nan, n = ctx.selftest_texel256()
    print("texel256 self-test: %d values; form in use: %d differ (+ %d NaN); conversion without floor: %d differ (+ %d NaN)" % (n, bad, bad_nan, bare, bare_nan))
    assert n == 2 * (0x44000000 - 0x3a800000) + 16
    assert bad == 0
