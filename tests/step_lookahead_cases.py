"""The cases of the step-size and look-ahead axes, shared by tests/test_oracle_step_lookahead.py (which pins the oracle on them
and asserts that they are worth drawing) and tests/test_gpu_step_lookahead.py (which draws them on the device).  Inputs and the
enumeration of cases only: no expected values live here.  The oracle's frame of a case is rendered once per process."""
import numpy as np

from tests import common

WORK_CAP = 2e7                      # n_vol + n_imp of the oracle, per case that the device draws
NOISE_DIMS = (24, 20, 28)
NOISE_THRESHOLD = 0.3
SAT_DIMS = (16, 16, 16)
BOXED_DIMS = (32, 28, 36)           # noise in the far three quarters, inset from the side faces: empty macro cells in front of every ray
BOX_DIMS = (40, 36, 44)             # the volume of test_gpu_parity.py::test_lookahead_reject_box
POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0)]          # the axis-aligned benchmark pose, and an orbit
SIZES = [(48, 32), (37, 23)]
SMALL = (24, 16)


def sizes(step):
    """The two frame sizes of a step: 48x32 and 37x23, but 37x23 and 24x16 below the GUI's finest step, where a ray takes 40 000
    samples and the 1056 hit rays of 48x32 at the benchmark pose put the smoothed and the cone frames over the work cap (2.0e7 to
    2.9e7 fetches measured; 37x23 stays below 1.7e7)"""
    return SIZES if step >= 0.001 - 1e-9 else [SIZES[1], SMALL]


MODES = [
    ("plain", dict()),
    ("smoothed", dict(use_gaussian_smoothing=1, density_threshold=0.12)),
    ("importance straight", dict(use_importance_rendering=1, importance_check_ahead_steps=6)),
    ("importance cone", dict(use_importance_rendering=1, use_cone_importance_check=1, importance_check_ahead_steps=6)),
]

_scenes = {}


def scene(name):
    """-> (dims, volume, importances): prepared bytes, the same for the oracle and the device"""
    if name in _scenes:
        return _scenes[name]
    if name == "noise":
        vol, imp = common.noise_scene(np.random.default_rng(31), NOISE_DIMS)
        out = (NOISE_DIMS, vol, imp)
    elif name == "saturated":
        n = SAT_DIMS[0] * SAT_DIMS[1] * SAT_DIMS[2]
        out = (SAT_DIMS, np.full(n, 255, np.uint8), common.noise_scene(np.random.default_rng(32), SAT_DIMS)[1])
    elif name == "boxed":
        # the noise confined to x, y in [1/8, 7/8) and z in [0, 3/4): orbit cameras with |horizontal angle| < 90 look at it through the
        # empty near quarter, so every ray that meets it has empty steps first -- in front of the box of the occupied macro cells,
        # where the march replays them in closed form -- and the content is thick enough to composite at step 1
        nx, ny, nz = BOXED_DIMS
        vol, imp = common.noise_scene(np.random.default_rng(34), BOXED_DIMS)
        z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        inside = (x >= nx // 8) & (x < nx - nx // 8) & (y >= ny // 8) & (y < ny - ny // 8) & (z < nz - nz // 4)
        out = (BOXED_DIMS, np.where(inside.ravel(), vol, 0).astype(np.uint8), imp)
    elif name == "bonsai":
        from oracle import oracle as O
        raw, labels = common.bonsai(64)
        dims = (64, 64, 64)
        vol, imp = common.oracle_scene(O, raw, labels, common.BONSAI_SEGMENTS, dims)
        out = (dims, vol, imp)
    elif name in ("middle", "one voxel"):
        # the cup and core of test_lookahead_reject_box with two of its importance maps
        rng = np.random.default_rng(99)
        dims = BOX_DIMS
        n = dims[0] * dims[1] * dims[2]
        zz, yy, xx = np.meshgrid(*(np.linspace(0.0, 1.0, d) for d in dims[::-1]), indexing="ij")
        shell = np.abs(np.sqrt((xx - 0.5) ** 2 + (yy - 0.5) ** 2 + (zz - 0.5) ** 2) - 0.38) < 0.06
        core = np.sqrt((xx - 0.45) ** 2 + (yy - 0.55) ** 2 + (zz - 0.5) ** 2) < 0.13
        vol = (np.where(shell, 110, 0) + np.where(core, 200, 0) + rng.integers(0, 6, shell.shape)).astype(np.uint8).ravel()
        if name == "middle":
            m = (xx >= 0.35) & (xx <= 0.6) & (yy >= 0.4) & (yy <= 0.7) & (zz >= 0.35) & (zz <= 0.65)
            imp = np.where(m, 255, 60).astype(np.uint8).ravel()
        else:
            imp = np.where(np.arange(n) == (20 * dims[1] + 18) * dims[0] + 20, 255, 0).astype(np.uint8)
        out = (dims, vol, imp)
    else:
        raise KeyError(name)
    _scenes[name] = out
    return out


def threshold(scene_name):
    return {"noise": NOISE_THRESHOLD, "boxed": 0.1}.get(scene_name, 0.15)      # (boxed: nine voxels in ten dense, so that sparse samples still meet some)


class Case:
    """One frame: scene, frame size, pose, filter and the parameter fields"""

    def __init__(self, scene_name, size, pose, filt, **par):
        self.scene, self.size, self.pose, self.filt = scene_name, tuple(size), tuple(pose), int(filt)
        par.setdefault("density_threshold", threshold(scene_name))
        self.par = par
        self.key = (scene_name, self.size, self.pose, self.filt, tuple(sorted(par.items())))

    def __repr__(self):
        return "%s %dx%d pose %s filter %d %s" % (self.scene, self.size[0], self.size[1], self.pose, self.filt,
                                                  " ".join("%s=%r" % kv for kv in sorted(self.par.items())))

    def uniforms(self, O):
        W, H = self.size
        return O.benchmark_camera_uniforms(W / H, *self.pose), O.make_parameters(**self.par)


_refs = {}


def reference(O, case):
    """The C oracle's (rgba32f, rgba8, counters) of a case; rendered once, shared, never written to"""
    if case.key not in _refs:
        dims, vol, imp = scene(case.scene)
        cam, par = case.uniforms(O)
        W, H = case.size
        f, u, k = O.render(vol, imp, dims, O.tf_default_lut(), cam, par, W, H, filter=case.filt)
        f.setflags(write=False)
        u.setflags(write=False)
        _refs[case.key] = (f, u, k)
    return _refs[case.key]


# ---- test_step_axis ------------------------------------------------------------------------------------------------------------

STEP_SCENES = ["noise", "saturated", "bonsai", "boxed"]
COARSE = 0.1 - 1e-6                 # from here up the boxed noise is drawn: it alone has empty space in front of content that these steps still meet


def step_axis_ids():
    """(index into step_axis(), scene) of every parameter of test_step_axis: the bonsai for steps <= 0.1 only (coarser steps
    hardly meet it), the boxed noise for steps >= 0.1"""
    return [(i, s) for i, step in enumerate(common.step_axis()) for s in STEP_SCENES
            if (s != "bonsai" or step <= 0.1 + 1e-6) and (s != "boxed" or step >= COARSE)]


def step_axis_cases(i, scene_name):
    """The frames of one parameter of test_step_axis, as [(layout, size, [(filter, [(mode name, Case)])])].
    Two entries, one per frame size of the step (sizes(step)); the first has layout i % 2, the second the other layout.
    Each entry holds both filters, each filter the four modes.  The pose of a case is POSES[(mode + filter + entry) % 2], so every
    (mode, filter) meets both poses over the two entries."""
    step = common.step_axis()[i]
    out = []
    for ci, size in enumerate(sizes(step)):
        layout = (ci + i) % 2
        per_filter = []
        for filt in (0, 1):
            per_filter.append((filt, [(name, Case(scene_name, size, POSES[(mi + filt + ci) % 2], filt, raymarching_step_size=step, **kw))
                                      for mi, (name, kw) in enumerate(MODES)]))
        out.append((layout, size, per_filter))
    return out


# ---- test_culling_changes_nothing_at_the_ends ------------------------------------------------------------------------------------

def culling_steps():
    s = common.step_axis()
    return [s[0], s[2], s[3], s[7]]


def culling_cases(step):
    """noise and saturated -- from step 0.1 up the boxed noise too --, three modes, both poses in turn, at the larger frame of the step"""
    out = []
    for si, scene_name in enumerate(("noise", "saturated", "boxed") if step >= COARSE else ("noise", "saturated")):
        for mi, (name, kw) in enumerate(MODES[:3]):
            out.append((name, Case(scene_name, sizes(step)[0], POSES[(si + mi) % 2], mi % 2, raymarching_step_size=step, **kw)))
    return out


# ---- test_ahead_axis -------------------------------------------------------------------------------------------------------------

AHEAD_SCENES = ["noise", "middle", "one voxel"]
AHEAD_STEPS = [0.05, 0.013]


def ahead_cases(count, cone):
    """The frames of one (count, straight / cone): three importance maps and two steps; counts above 256 at step 0.05 and 24x16
    only (the work cap).  The frame size alternates, the pose too."""
    out = []
    for si, scene_name in enumerate(AHEAD_SCENES):
        for ti, step in enumerate(AHEAD_STEPS):
            if count > 256 and step < 0.05:
                continue
            size = SMALL if count > 256 else SIZES[(si + ti) % 2]
            out.append(Case(scene_name, size, POSES[(si + ti + cone) % 2], 0, raymarching_step_size=step, use_importance_rendering=1,
                            use_cone_importance_check=cone, importance_check_ahead_steps=count))
    return out


# ---- test_pairs_change_between_enqueued_frames -------------------------------------------------------------------------------------

def burst_pairs():
    """12 (step, count) pairs, one per enqueued frame: every step of the axis and twelve of the counts; step 1e-4 and its
    neighbour go with counts <= 2 and counts above 256 with steps >= 0.05 (the work cap)."""
    s = common.step_axis()
    pairs = [(s[3], 25), (s[0], 2), (s[5], 4096), (s[2], 26), (s[7], 1000), (s[1], 0), (s[4], 255), (s[3], 1), (s[6], 4095),
             (s[2], 63), (s[5], 3), (s[3], 256)]
    assert len(pairs) == 12 and all(a != b for a, b in zip(pairs, pairs[1:]))
    return pairs


def burst_cases(cone):
    return [Case("noise", SMALL, POSES[1], 0, raymarching_step_size=step, use_importance_rendering=1, use_cone_importance_check=cone,
                 importance_check_ahead_steps=count) for step, count in burst_pairs()]


# ---- the rest ----------------------------------------------------------------------------------------------------------------------

def pick_steps():
    s = common.step_axis()
    return [s[2], s[3], s[7]]


def mgpu_cases():
    s = common.step_axis()
    return [Case("noise", (96, 64), POSES[1], 0, raymarching_step_size=step, use_importance_rendering=1, use_cone_importance_check=1,
                 importance_check_ahead_steps=25) for step in (s[2], s[3])]


def refusal_cases():
    """the frame before the refusals, and the two accepted corners of the ranges"""
    s = common.step_axis()
    kw = dict(use_importance_rendering=1)
    return [Case("noise", SMALL, POSES[1], 0, raymarching_step_size=0.05, importance_check_ahead_steps=3, **kw),
            Case("noise", SMALL, POSES[1], 0, raymarching_step_size=s[0], importance_check_ahead_steps=0, **kw),
            Case("noise", SMALL, POSES[1], 0, raymarching_step_size=s[7], importance_check_ahead_steps=4096, **kw)]


def pick_case(step):
    """the boxed noise: its distance field is not all zeros, so a pick after the first frame leaps where one before it marches"""
    return Case("boxed", SIZES[1], POSES[1], 0, raymarching_step_size=step)


def device_cases():
    """Every Case the GPU file draws with fixed uniforms (the GUI test's come out of scene.State): what the oracle test vets"""
    out = []
    for i, s in step_axis_ids():
        for _, _, per_filter in step_axis_cases(i, s):
            for _, modes in per_filter:
                out += [c for _, c in modes]
    for step in culling_steps():
        out += [c for _, c in culling_cases(step)]
    for count in common.ahead_axis():
        for cone in (0, 1):
            out += ahead_cases(count, cone)
    for cone in (0, 1):
        out += burst_cases(cone)
    out += mgpu_cases() + refusal_cases() + [pick_case(step) for step in pick_steps()]
    seen, uniq = set(), []
    for c in out:
        if c.key not in seen:
            seen.add(c.key)
            uniq.append(c)
    return uniq
