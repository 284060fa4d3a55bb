"""The march's lane predicates as wave masks (raymarch_pq.h MASKS), on the shapes at which mask plumbing can go wrong.

The straight-line forms of kernel 2's two march loops hold `active`, `last_dense`, `leap_ok` and what an iteration derives from
them as 64-bit lane masks from an entry's set-up to its store.  A mask goes wrong where a bool did not: ~m sets the bits of
lanes that are out of the frame, a ballot in a divergent region drops lanes, a stale bit survives an iteration.  So the frames
here are ragged (lanes out of the frame from the start, tiles with one live lane, tiles with none), the rays end inside a
speculative batch in every way they can (t >= t_end, alpha >= 0.95, a class change at any of the K positions), and every frame is
drawn by the classic loop (centre-first list, then the cost-ordered one), by the depth-parallel loop (every marched tile as
quarters) and in both frame slots.

The bar is tests/test_gpu_parity.py's, with its helpers: the five counters equal to the oracle's, floats within 1e-4, rgba8
within 1 LSB, on every pixel of every frame.  Besides, every frame is bit-equal in f32 to the frame of a context with culling and
cost feedback off (tests/test_gpu_step_lookahead.py does the same at the ends of the step axis).  The scene is the boxed noise of
tests/step_lookahead_cases.py at other sizes: empty macro cells in front of the content, so the leap phase and the closed-form
replay run, and nine voxels in ten dense, so classes change at every position of a batch."""
import numpy as np
import pytest

from tests import common
from tests import step_lookahead_cases as SC
from tests.test_gpu_parity import _check, _ctx, _render_gpu

pytestmark = pytest.mark.gpu

VIEWPORTS = [(8, 8), (17, 9), (70, 45)]
VOLUMES = [(32, 32, 32), (40, 24, 56)]
POSES = SC.POSES
THRESHOLD = SC.threshold("boxed")
TF_SEED = 5

_scenes, _refs, _tfs = {}, {}, {}


def _scene(dims):
    """(volume, importances): SC.scene("boxed") at `dims` -- the noise confined to x, y in [1/8, 7/8) and z in [0, 3/4)"""
    if dims not in _scenes:
        nx, ny, nz = dims
        vol, imp = common.noise_scene(np.random.default_rng(34), dims)
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        inside = (x >= nx // 8) & (x < nx - nx // 8) & (y >= ny // 8) & (y < ny - ny // 8) & (z < nz - nz // 4)
        _scenes[dims] = (np.where(inside.ravel(), vol, 0).astype(np.uint8), imp)
    return _scenes[dims]


def _tf(name):
    """default; opaque (the first dense sample ends the ray by alpha); comb (alpha 0 and 255 in turn: a ray ends by alpha at whichever
    position of a batch first meets an odd byte)"""
    if not _tfs:
        _tfs.update(dict(common.tf_family(np.random.default_rng(TF_SEED))))
    return _tfs[name]


def _away(oracle, aspect):
    """the benchmark eye looking away from the cube: no ray hits it"""
    cam = oracle.camera_default(aspect, (0.5, 0.5, 1.5))
    for i, v in enumerate((0.5, 0.5, 3.0)):
        cam.target[i] = v
    return oracle.camera_uniforms(cam)


def _view(oracle, size, pose):
    W, H = size
    return _away(oracle, W / H) if pose == "away" else oracle.benchmark_camera_uniforms(W / H, *pose)


def _reference(oracle, dims, size, pose, tf, filt, par_kw):
    key = (dims, size, pose, tf, filt, tuple(sorted(par_kw.items())))
    if key not in _refs:
        vol, imp = _scene(dims)
        W, H = size
        f, u, k = oracle.render(vol, imp, dims, _tf(tf), _view(oracle, size, pose), oracle.make_parameters(**par_kw), W, H, filter=filt)
        f.setflags(write=False)
        u.setflags(write=False)
        _refs[key] = (f, u, k)
    return _refs[key]


def _open(size, dims, tf, filt, layout, options):
    from volym_amd import _lib
    vol, imp = _scene(dims)
    ctx = _ctx(*size)
    ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
    for key, value in options:
        ctx.set_option(key, value)
    ctx.set_volume(vol, dims, filt)
    ctx.set_importances(imp, dims)
    ctx.set_transfer_function(_tf(tf))
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Contexts:
    """The three contexts a (frame size, volume, table, filter, layout) is drawn in: culling and feedback off; the default; two
    frames in flight with every marched tile as quarters"""

    def __init__(self, size, dims, tf="default", filt=0, layout=0):
        from volym_amd import _lib
        self.key = (size, dims, tf, filt, layout)
        self.plain = _open(size, dims, tf, filt, layout, ((_lib.OPT_CULLING, 0), (_lib.OPT_COST_FEEDBACK, 0), (_lib.OPT_BOUNDS_CELLS, 0)))
        self.main = _open(size, dims, tf, filt, layout, ())
        self.flight = _open(size, dims, tf, filt, layout, ((_lib.OPT_FRAMES_IN_FLIGHT, 2), (_lib.OPT_DEPTH_PARALLEL, 1)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for c in (self.plain, self.main, self.flight):
            c.__exit__(*exc)

    def draw(self, oracle, pose, par_kw, label):
        """Nine frames of one view, each against the oracle and bit-equal to the first: no culling; centre-first list, cost-ordered
        list, then both again with every marched tile as quarters; four frames over the two slots.  Each with its instrumented
        launch (_render_gpu's stats_pass).  -> the oracle's counters"""
        from volym_amd import _lib
        size, dims, tf, filt, _ = self.key
        ref = _reference(oracle, dims, size, pose, tf, filt, par_kw)
        cam, par = _view(oracle, size, pose), oracle.make_parameters(**par_kw)
        frames = [("no culling", _render_gpu(self.plain, cam, par, 2))]
        self.main.set_option(_lib.OPT_DEPTH_PARALLEL, -1)
        frames += [("centre-first list", _render_gpu(self.main, cam, par, 2)), ("cost-ordered list", _render_gpu(self.main, cam, par, 2))]
        self.main.set_option(_lib.OPT_DEPTH_PARALLEL, 1)
        frames += [("quarters, centre-first list", _render_gpu(self.main, cam, par, 2)), ("quarters", _render_gpu(self.main, cam, par, 2))]
        frames += [("two in flight, frame %d" % n, _render_gpu(self.flight, cam, par, 2)) for n in range(4)]
        worst, worst8 = 0.0, 0
        for name, got in frames:
            err, _ = _check(got, ref, "%s, %s" % (label, name))
            worst, worst8 = max(worst, err), max(worst8, int(np.abs(got[1].astype(np.int32) - ref[1].astype(np.int32)).max()))
            first = frames[0][1]
            assert np.array_equal(_bits(got[0]), _bits(first[0])) and np.array_equal(got[1], first[1]) and got[2] == first[2], \
                "%s, %s: differs from the frame without culling" % (label, name)
        k = ref[2]
        print("MASKS | %s | n_vol %d n_imp %d n_steps %d n_dense %d n_hit %d | max float error %.3g | max rgba8 difference %d"
              % (label, k["n_vol"], k["n_imp"], k["n_steps"], k["n_dense"], k["n_hit"], worst, worst8))
        return k


# ---- 1. ragged frames ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", VOLUMES, ids=["%dx%dx%d" % d for d in VOLUMES])
@pytest.mark.parametrize("size", VIEWPORTS, ids=["%dx%d" % s for s in VIEWPORTS])
def test_ragged_frames(oracle, volym_lib, size, dims):
    """8x8 (one tile, three quarters of its 16x16 entry out of the frame), 17x9 (a column of tiles with one live lane per row, a
    row of tiles with one live row) and 70x45, on a cube and on a volume of three different extents: both poses, and a view whose
    rays all miss the cube."""
    hits = 0
    with Contexts(size, dims) as cs:
        for pose in POSES + ["away"]:
            k = cs.draw(oracle, pose, dict(density_threshold=THRESHOLD, raymarching_step_size=0.05), "ragged %dx%d, %s, pose %s" % (size + (dims, pose)))
            if pose == "away":
                assert k["n_hit"] == 0 and k["n_steps"] == 0, k
            else:
                hits += k["n_dense"]
    assert hits > 0


# ---- 2. every exit inside a speculative batch ------------------------------------------------------------------------------------------

EXIT_STEPS = [0.5, 0.25, 0.1, 0.013]        # rays of one to four samples (t >= t_end inside the first batch), and rays of many batches


@pytest.mark.parametrize("tf", ["default", "opaque", "comb"])
@pytest.mark.parametrize("step", EXIT_STEPS, ids=["%g" % s for s in EXIT_STEPS])
def test_every_exit_inside_a_batch(oracle, volym_lib, step, tf):
    """A ray leaves the march by t >= t_end (coarse steps: at the first, second, third or fourth sample of its first batch), by
    alpha >= 0.95 (the opaque table: at its first dense sample, wherever in a batch that is; the comb: at the first odd byte)
    or goes on after a class change at any position of a batch (the noise).  70x45 on the 40x24x56 volume and 17x9 on the cube."""
    for size, dims, pose in (((70, 45), VOLUMES[1], POSES[1]), ((17, 9), VOLUMES[0], POSES[0])):
        with Contexts(size, dims, tf) as cs:
            k = cs.draw(oracle, pose, dict(density_threshold=THRESHOLD, raymarching_step_size=step), "exits, step %g, %s table, %dx%d" % ((step, tf) + size))
            assert k["n_hit"] > 0 and k["n_steps"] > k["n_dense"] > 0, k      # dense and empty samples both: classes change


# ---- 3. every instantiation that shares the code ---------------------------------------------------------------------------------------

INSTANTIATIONS = [
    # name, filter, layout, parameters
    ("base", 0, 0, dict()),
    ("first hit", 0, 0, dict(use_opacity=0)),
    ("importance straight", 0, 0, dict(use_importance_rendering=1, importance_check_ahead_steps=6)),
    ("importance cone", 0, 0, dict(use_importance_rendering=1, use_cone_importance_check=1, importance_check_ahead_steps=6)),
    ("importance colouring", 0, 0, dict(use_importance_coloring=1)),
    ("smoothing", 0, 0, dict(use_gaussian_smoothing=1)),
    ("trilinear", 1, 0, dict()),
    ("bricked", 0, 1, dict()),
    ("bricked, importance straight", 0, 1, dict(use_importance_rendering=1, importance_check_ahead_steps=6)),
    ("bricked, importance cone", 0, 1, dict(use_importance_rendering=1, use_cone_importance_check=1, importance_check_ahead_steps=6)),
]


@pytest.mark.parametrize("name,filt,layout,kw", INSTANTIATIONS, ids=[i[0] for i in INSTANTIATIONS])
def test_every_instantiation(oracle, volym_lib, name, filt, layout, kw):
    """70x45 on the 40x24x56 volume through every instantiation of the kernel: the straight-line forms (base, importance
    rendering with either look-ahead, both layouts) and the general forms beside them, which share the set-up, the leap phase and
    the queue; the instrumented launch beside each frame."""
    size, dims = VIEWPORTS[2], VOLUMES[1]
    with Contexts(size, dims, "default", filt, layout) as cs:
        for pose in POSES:
            k = cs.draw(oracle, pose, dict(density_threshold=THRESHOLD, raymarching_step_size=0.02, **kw), "%s, pose %s" % (name, pose))
            assert k["n_dense"] > 0, k
