"""Segment importances on the device (volym_set_labels / volym_set_segment_importances).  Every frame after an edit is
compared with what volym_set_importances(host map) gives under the same context settings (rgba8 and f32 bit-equal, fetch
counters equal) and with the CPU oracle (<= 1e-4, <= 1 rgba8 LSB)."""
import numpy as np
import pytest

from tests import common

TOL = 1e-4
W, H = 96, 64
PARAMS = {
    "straight": dict(use_importance_rendering=1, importance_check_ahead_steps=15),
    "cone": dict(use_importance_rendering=1, importance_check_ahead_steps=15, use_cone_importance_check=1),
    "colouring": dict(use_importance_rendering=1, importance_check_ahead_steps=15, use_importance_coloring=1),
}


def _table(**imp):
    t = np.zeros(256, np.uint8)
    for l, v in imp.items():
        t[int(l[1:])] = v
    return t


# bonsai labels: 2 canopy, 3 trunk, 4 pot, 0 the rest
BONSAI_TABLES = {
    "canopy": _table(l2=255),
    "trunk only": _table(l3=255, l2=40),
    "nothing": _table(l2=127, l3=10),
    "everything 255": np.full(256, 255, np.uint8),
    "label 0": _table(l0=255, l4=90),
}


def _uniforms(oracle, w, h, pose=(0.0, 0.0, 0.0), **kw):
    from volym_amd import _lib
    cam = oracle.benchmark_camera_uniforms(w / h, *pose)
    par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01, **kw)
    return cam, par, _lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par))


def _bonsai():
    raw, labels = common.bonsai(64)
    from volym_amd import scene
    dims = (64, 64, 64)
    return dims, scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)


def _ragged():
    """97 x 80 x 71 (no dimension a multiple of 4): a cup with a core, labelled 1 (shell), 2 (core), 5 (a blob at a corner)."""
    dims = (97, 80, 71)
    zz, yy, xx = np.meshgrid(*(np.linspace(0.0, 1.0, d) for d in dims[::-1]), indexing="ij")
    r = np.sqrt((xx - 0.5) ** 2 + (yy - 0.5) ** 2 + (zz - 0.5) ** 2)
    shell = np.abs(r - 0.38) < 0.06
    core = np.sqrt((xx - 0.45) ** 2 + (yy - 0.55) ** 2 + (zz - 0.5) ** 2) < 0.13
    blob = np.sqrt((xx - 0.85) ** 2 + (yy - 0.2) ** 2 + (zz - 0.8) ** 2) < 0.1
    rng = np.random.default_rng(5)
    vol = (np.where(shell, 110, 0) + np.where(core, 200, 0) + np.where(blob, 150, 0) + rng.integers(0, 6, shell.shape)).clip(0, 255)
    labels = np.where(blob, 5, np.where(core, 2, np.where(shell, 1, 0)))
    return dims, vol.astype(np.uint8).ravel(), labels.astype(np.uint8).ravel()


RAGGED_TABLES = {
    "core": _table(l2=255),
    "shell only": _table(l1=200),
    "nothing": _table(l1=100),
    "everything 255": np.full(256, 255, np.uint8),
    "label 0": _table(l0=255),
}


def _ctx(layout, opts=()):
    from volym_amd import _lib, demo
    c = demo.GpuContext(W, H, 0)
    c.set_option(_lib.OPT_WRITE_F32, 1)
    c.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
    for k, v in opts:
        c.set_option(k, v)
    return c


def _frame(ctx, cu, pu, update=True):
    if update:
        ctx.update(cu, pu)
    ctx.compute_pass()
    ctx.sync()
    return ctx.read_rgba32f(), ctx.read_rgba8()


def _check(oracle, what, vol, imp, dims, cam, par, f32, u8, host_f32=None, host_u8=None):
    if host_u8 is not None:
        assert np.array_equal(u8, host_u8), "%s: rgba8 differs from the host-mapped importances" % what
        assert np.array_equal(f32.view(np.uint32), host_f32.view(np.uint32)), "%s: f32 differs from the host-mapped importances" % what
    ref_f32, ref_u8, _ = oracle.render(vol, imp, dims, oracle.tf_default_lut(), cam, par, W, H)
    err, over, du8, _ = common.compare_images(f32, u8, ref_f32, ref_u8, TOL)
    assert over == 0 and err <= TOL and du8 <= 1, (what, err, over, du8)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_table_sequence_matches_host_map(oracle, volym_lib, volume, layout):
    from volym_amd import scene
    dims, vol, labels = _bonsai() if volume == "bonsai64" else _ragged()
    tables = BONSAI_TABLES if volume == "bonsai64" else RAGGED_TABLES
    lut = scene.default_lut()
    with _ctx(layout) as dev, _ctx(layout) as host:
        for c in (dev, host):
            c.set_volume(vol, dims, 0)
            c.set_transfer_function(lut)
        dev.set_labels(labels, dims)
        assert np.array_equal(dev.label_counts(), np.bincount(labels, minlength=256).astype(np.uint64))
        for tname, table in tables.items():
            dev.set_segment_importances(table)
            imp = table[labels]
            host.set_importances(imp, dims)
            for pname, kw in PARAMS.items():
                cam, par, cu, pu = _uniforms(oracle, W, H, **kw)
                f32, u8 = _frame(dev, cu, pu)
                h32, h8 = _frame(host, cu, pu)
                _check(oracle, (volume, layout, tname, pname), vol, imp, dims, cam, par, f32, u8, h32, h8)
                assert dev.stats_pass() == host.stats_pass(), (volume, layout, tname, pname)


CORNER_POSE = (-30.0, -20.0, 0.0)


def _corner_scene():
    """The ragged volume with two small important candidates inside the cup, in opposite corners of it: label 5 around
    (0.64, 0.36, 0.36), label 6 around (0.33, 0.66, 0.38).  Seen from CORNER_POSE the shell hides them, so the look-ahead decides
    pixels, and a reject box of the wrong label rejects the probes that should have found the important one."""
    dims, vol, labels = _ragged()
    zz, yy, xx = np.meshgrid(*(np.linspace(0.0, 1.0, d) for d in dims[::-1]), indexing="ij")

    def ball(c, r):
        return (np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) < r).ravel()
    a, b = ball((0.64, 0.36, 0.36), 0.08), ball((0.33, 0.66, 0.38), 0.08)
    labels = np.where(a, 5, np.where(b, 6, labels)).astype(np.uint8)
    vol = np.where(a | b, 160, vol).astype(np.uint8)
    return dims, vol, labels


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_corner_segment_and_edit_without_update(oracle, volym_lib, layout):
    """An important segment confined to a corner, then a table that moves the important box to the opposite corner followed
    by passes with NO volym_update: the frames must follow the new table (a stale reject box would drop its probes)."""
    from volym_amd import scene
    dims, vol, labels = _corner_scene()
    lut = scene.default_lut()
    t5, t6 = _table(l5=255), _table(l6=255)
    for pname in ("straight", "cone"):
        cam, par, cu, pu = _uniforms(oracle, W, H, pose=CORNER_POSE, **PARAMS[pname])
        with _ctx(layout) as dev:
            dev.set_volume(vol, dims, 0)
            dev.set_transfer_function(lut)
            dev.set_labels(labels, dims)
            dev.set_segment_importances(t5)
            f32, u8 = _frame(dev, cu, pu)
            _check(oracle, (layout, pname, "corner 5"), vol, t5[labels], dims, cam, par, f32, u8)
            first = u8
            # what a stale box (label 5's) would give: label 6's probes rejected, as if nothing were important there
            _, none_u8, _ = oracle.render(vol, np.zeros_like(labels), dims, oracle.tf_default_lut(), cam, par, W, H)
            _, t6_u8, _ = oracle.render(vol, t6[labels], dims, oracle.tf_default_lut(), cam, par, W, H)
            assert (np.abs(none_u8.astype(int) - t6_u8.astype(int)) > 1).any(), "the scene must tell a stale box from the new one"
            dev.set_segment_importances(t6)                          # no volym_update from here on
            for k in range(3):
                f32, u8 = _frame(dev, cu, pu, update=False)
                _check(oracle, (layout, pname, "corner 6, pass %d without update" % k), vol, t6[labels], dims, cam, par, f32, u8)
            assert not np.array_equal(u8, first), "the edit must change the frame"


@pytest.mark.gpu
def test_two_frames_in_flight_alternate_edits(oracle, volym_lib):
    """VOLYM_OPT_FRAMES_IN_FLIGHT = 2: edits alternate with passes (some with, some without a volym_update); every frame after
    an edit matches the new table, whichever slot renders it."""
    from volym_amd import _lib, scene
    dims, vol, labels = _corner_scene()
    lut = scene.default_lut()
    cam, par, cu, pu = _uniforms(oracle, W, H, pose=CORNER_POSE, **PARAMS["straight"])
    tables = [_table(l5=255), _table(l6=255), _table(l2=255, l6=200), _table(l1=130)]
    refs = {}
    with _ctx(-1, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)]) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        dev.set_labels(labels, dims)
        dev.set_segment_importances(tables[0])
        dev.update(cu, pu)
        for step in range(8):
            i = step % len(tables)
            dev.set_segment_importances(tables[i])
            if step % 2:
                dev.update(cu, pu)
            for n_pass in (1, 2):                                     # the frame of each slot
                for _ in range(n_pass):
                    dev.compute_pass()
                dev.sync()
                f32, u8 = dev.read_rgba32f(), dev.read_rgba8()
                if i not in refs:
                    _check(oracle, ("in flight", step, n_pass), vol, tables[i][labels], dims, cam, par, f32, u8)
                    refs[i] = (f32, u8)
                else:
                    assert np.array_equal(u8, refs[i][1]) and np.array_equal(f32.view(np.uint32), refs[i][0].view(np.uint32)), (step, n_pass)


@pytest.mark.gpu
def test_error_paths(oracle, volym_lib):
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    with _ctx(-1) as c:
        c.set_volume(vol, dims, 0)
        c.set_transfer_function(scene.default_lut())
        for call in (lambda: c.set_segment_importances(BONSAI_TABLES["canopy"]), c.label_counts):
            with pytest.raises(_lib.VolymError) as e:                  # no labels yet
                call()
            assert e.value.code == _lib.E_STATE
        c.set_labels(labels, dims)
        c.set_segment_importances(BONSAI_TABLES["canopy"])
        c.set_importances(BONSAI_TABLES["trunk only"][labels], dims)  # drops the labels
        with pytest.raises(_lib.VolymError) as e:
            c.set_segment_importances(BONSAI_TABLES["canopy"])
        assert e.value.code == _lib.E_STATE
        # labels of other dims: the table is accepted, volym_update refuses the mismatch as it does for importances
        small = (32, 32, 32)
        c.set_labels(labels[:32 * 32 * 32], small)
        c.set_segment_importances(BONSAI_TABLES["canopy"])
        _, _, cu, pu = _uniforms(oracle, W, H)
        with pytest.raises(_lib.VolymError) as e:
            c.update(cu, pu)
        assert e.value.code == _lib.E_STATE
        # the right labels again: the context renders
        c.set_labels(labels, dims)
        c.set_segment_importances(BONSAI_TABLES["canopy"])
        c.update(cu, pu)
        c.compute_pass()
        c.sync()


@pytest.mark.gpu
def test_simple_set_segments(oracle, volym_lib):
    """demo.Simple.set_segments: the device table, and the host fall-back for a label-0 segment on a short label file."""
    from volym_amd import demo, scene
    raw, labels_raw = common.bonsai(64)
    dims = (64, 64, 64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01, use_importance_rendering=1)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    short = labels_raw[: labels_raw.size - 64 * 64 * 5]
    cases = [(labels_raw, [{"label_value": 3, "importance": 255}, {"label_value": 3, "importance": 0}]),
             (short, [{"label_value": 2, "importance": 255}]),
             (short, [{"label_value": 0, "importance": 255}]),            # host fall-back
             (short, [{"label_value": 4, "importance": 255}])]            # back on the device
    with demo.GpuContext(W, H, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        current = None
        for lraw, segs in cases:
            if lraw is not current:
                d.set_labels(ctx, lraw)
                current = lraw
            d.set_segments(ctx, segs)
            d.update_gpu_state(ctx, state)
            d.compute_pass(ctx)
            ctx.sync()
            got = ctx.read_rgba8()
            with demo.GpuContext(W, H, 0) as ref_ctx:
                demo.Simple.init(ref_ctx, state, volume_raw=raw, labels_raw=lraw, segments=segs, dims=dims).compute_pass(ref_ctx)
                ref_ctx.sync()
                assert np.array_equal(got, ref_ctx.read_rgba8()), segs


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3])
def test_mgpu_virtual_ranks_after_edit(oracle, volym_lib, world):
    from volym_amd import demo, mgpu, scene
    dims, vol, labels = _corner_scene()
    lut = scene.default_lut()
    w, h = 310, 170
    _, _, cu, pu = _uniforms(oracle, w, h, pose=CORNER_POSE, **PARAMS["straight"])
    with demo.GpuContext(w, h, 0) as solo, mgpu.MultiGpu(w, h, devices=[0] * world, transport=mgpu.COPY) as mg:
        solo.set_volume(vol, dims, 0)
        solo.set_transfer_function(lut)
        solo.set_labels(labels, dims)
        mg.set_volume(vol, dims, 0)
        mg.set_transfer_function(lut)
        mg.set_labels(labels, dims)
        for table in (_table(l5=255), _table(l6=255)):
            solo.set_segment_importances(table)
            solo.update(cu, pu)
            solo.compute_pass()
            solo.sync()
            mg.set_segment_importances(table)
            mg.update(cu, pu)
            mg.prepare(0)
            t = mg.run(2, use_graph=False)
            assert t["overflowed"] == 0
            assert np.array_equal(mg.read_rgba8(), solo.read_rgba8()), world


@pytest.mark.gpu
def test_config4_1024cube_labels_two_edits(oracle, volym_lib):
    """BASELINE configs[4] (1024^3 + labels at 3840x2160, bricked by size): two edits, each checked against the oracle on
    sampled rows."""
    from volym_amd import _lib, demo, scene
    raw, labels = common.bonsai(1024)
    dims = (1024, 1024, 1024)
    vol = scene.prepare_volume(raw, dims, True)
    lab = scene.prepare_volume(labels, dims, True)
    del raw, labels
    common._cache.pop(("bonsai", 1024), None)
    w, h = 3840, 2160
    lut, lut_o = scene.default_lut(), oracle.tf_default_lut()
    rows = list(range(5, h, 64))
    cam, par, cu, pu = _uniforms(oracle, w, h, **PARAMS["straight"])
    with demo.GpuContext(w, h, 0) as ctx:
        ctx.set_option(_lib.OPT_WRITE_F32, 1)
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(lut)
        ctx.set_labels(lab, dims)
        counts = ctx.label_counts()
        assert int(counts.sum()) == 1024 ** 3
        assert np.array_equal(counts, np.bincount(lab, minlength=256).astype(np.uint64))
        for table in (_table(l2=255), _table(l3=255, l4=200)):
            ctx.set_segment_importances(table)
            imp = table[lab]
            ref_f32, ref_u8, _ = oracle.render(vol, imp, dims, lut_o, cam, par, w, h, rowlist=rows)
            ctx.update(cu, pu)
            ctx.compute_pass()
            ctx.sync()
            f32, u8 = ctx.read_rgba32f(), ctx.read_rgba8()
            err, over, du8, _ = common.compare_images(f32[rows], u8[rows], ref_f32[rows], ref_u8[rows], TOL)
            assert over == 0 and err <= TOL and du8 <= 1, (err, over, du8)
            assert u8[rows][..., :3].any()
            del imp
