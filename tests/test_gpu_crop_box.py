"""Crop box on the device (volym_set_crop_box).  A frame with crop box B is the frame of the scene whose density AND importance
bytes outside B are 0: the expected pictures come from oracle.render on scene.crop_volume-zeroed inputs (<= 1e-4 on f32, <= 1
rgba8 LSB), and a twin context that receives the zeroed bytes through set_volume / set_importances must give bit-equal rgba8
and f32.  After every edit three frames of the standing view are read (the first runs without tile mask and depth bounds, the
later ones with them) and must be bit-equal to each other."""
import ctypes as C

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

TOL = 1e-4
W, H = 96, 64
PARAMS = {
    "base": dict(),
    "no opacity": dict(use_opacity=0),
    "smoothing": dict(use_gaussian_smoothing=1),
    "straight": dict(use_importance_rendering=1, importance_check_ahead_steps=15),
    "cone": dict(use_importance_rendering=1, importance_check_ahead_steps=15, use_cone_importance_check=1),
    "colouring": dict(use_importance_rendering=1, importance_check_ahead_steps=15, use_importance_coloring=1),
}


def _table(**imp):
    t = np.zeros(256, np.uint8)
    for l, v in imp.items():
        t[int(l[1:])] = v
    return t


CANOPY = _table(l2=255)            # common.BONSAI_SEGMENTS as a table
POT = _table(l4=255)               # the pot important, canopy and trunk 0


def _uniforms(oracle, w, h, pose=(0.0, 0.0, 0.0), **kw):
    from volym_amd import _lib
    cam = oracle.benchmark_camera_uniforms(w / h, *pose)
    par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01, **kw)
    return cam, par, _lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par))


def _bonsai(n=64):
    from volym_amd import scene
    raw, labels = common.bonsai(n)
    dims = (n, n, n)
    return dims, scene.prepare_volume(raw, dims, True), scene.prepare_volume(labels, dims, True)


def _ragged():
    """97 x 80 x 71 (no dimension a multiple of 4): a cup with a core, labelled 1 (shell), 2 (core), 5 (a blob at a corner).
    (The scene of tests/test_gpu_segment_importances.py.)"""
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


def _ctx(layout, opts=(), w=W, h=H):
    from volym_amd import _lib, demo
    c = demo.GpuContext(w, h, 0)
    c.set_option(_lib.OPT_WRITE_F32, 1)
    c.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
    for k, v in opts:
        c.set_option(k, v)
    return c


def _frame(ctx, cu=None, pu=None):
    if cu is not None:
        ctx.update(cu, pu)
    ctx.compute_pass()
    ctx.sync()
    return ctx.read_rgba32f(), ctx.read_rgba8()


def _three(ctx, what, cu=None, pu=None):
    """Three frames of the standing view (an update before the first when uniforms are given): bit-equal, the first returned."""
    f32, u8 = _frame(ctx, cu, pu)
    for k in (2, 3):
        g32, g8 = _frame(ctx)
        assert np.array_equal(g8, u8), "%s: rgba8 of frame %d after the edit differs from frame 1" % (what, k)
        assert np.array_equal(g32.view(np.uint32), f32.view(np.uint32)), "%s: f32 of frame %d after the edit differs from frame 1" % (what, k)
    return f32, u8


def _same(what, a, b):
    assert np.array_equal(a[1], b[1]), "%s: rgba8 differs" % (what,)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "%s: f32 differs" % (what,)


def _oracle(oracle, vol, imp, dims, cam, par, w=W, h=H, **kw):
    return oracle.render(vol, imp, dims, oracle.tf_default_lut(), cam, par, w, h, **kw)


def _near(what, got, ref, rows=None):
    sel = slice(None) if rows is None else rows
    err, over, du8, _ = common.compare_images(got[0][sel], got[1][sel], ref[0][sel], ref[1][sel], TOL)
    assert over == 0 and err <= TOL and du8 <= 1, (what, err, over, du8)


def _changed(a_u8, b_u8):
    """fraction of the pixels whose rgba8 differs"""
    return float((a_u8 != b_u8).any(axis=-1).mean())


def _sequence(dims):
    nx, ny, nz = dims
    return [
        ("far z face by 1", (0, 0, 0), (nx, ny, nz - 1)),
        ("far z face by 5 more", (0, 0, 0), (nx, ny, nz - 6)),
        ("the opposite face", (0, 0, 7), (nx, ny, nz - 6)),
        ("all six faces at once", (5, 7, 9), (nx - 14, ny - 3, nz - 21)),
        ("aligned to 4 on no axis", (13, 3, 6), (nx - 10, ny - 18, nz - 1)),
        ("keep the near z part", (0, 0, 0), (nx, ny, 40 * nz // 64)),
        ("one texel thick", (30 * nx // 64, 0, 0), (30 * nx // 64 + 1, ny, nz)),
        ("one x face by 1", (30 * nx // 64, 0, 0), (30 * nx // 64 + 2, ny, nz)),
        ("empty", (10, 0, 0), (10, ny, nz)),
        ("growing again", (2, 2, 2), (nx // 2, ny - 2, nz - 2)),
        ("growing on y", (2, 1, 2), (nx // 2, ny, nz - 2)),
        ("full", (0, 0, 0), (nx, ny, nz)),
    ]


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_edit_sequence(oracle, volym_lib, volume, layout):
    """Box after box on one context against a twin that is handed the host-zeroed bytes, and against the oracle.  bonsai: the
    importances come from labels on the device (their own uncropped source); ragged: uploaded importances (a device copy)."""
    from volym_amd import scene
    pose = (35.0, 20.0, 0.0)
    if volume == "bonsai64":
        dims, vol, labels = _bonsai()
        table = CANOPY
    else:
        dims, vol, labels = _ragged()
        table = _table(l2=255)
    imp = table[labels]
    lut = scene.default_lut()
    modes = {k: _uniforms(oracle, W, H, pose, **PARAMS[k]) for k in ("base", "straight")}
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        if volume == "bonsai64":
            dev.set_labels(labels, dims)
            dev.set_segment_importances(table)
        else:
            dev.set_importances(imp, dims)
        twin.set_transfer_function(lut)
        assert dev.crop_box() == ((0, 0, 0), dims)
        before = {k: _three(dev, (k, "uncropped"), cu, pu) for k, (cam, par, cu, pu) in modes.items()}
        uncropped = {k: _oracle(oracle, vol, imp, dims, cam, par) for k, (cam, par, cu, pu) in modes.items()}
        for k in modes:
            _near((volume, layout, k, "uncropped"), before[k], uncropped[k])
        cutting = 0
        for step, (name, lo, hi) in enumerate(_sequence(dims)):
            cvol, cimp = scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi)
            twin.set_volume(cvol, dims, 0)
            twin.set_importances(cimp, dims)
            for k, (cam, par, cu, pu) in modes.items():
                what = (volume, layout, name, k)
                if k == "base":
                    dev.update(cu, pu)                      # the view of this mode, then the edit with NO update after it
                    _frame(dev)
                    dev.set_crop_box(lo, hi)
                    assert dev.crop_box() == (lo, hi)
                    got = _three(dev, what)
                else:
                    got = _three(dev, what, cu, pu)
                _same(what + ("twin",), got, _frame(twin, cu, pu))
                ref = _oracle(oracle, cvol, cimp, dims, cam, par)
                _near(what, got, ref)
                if k == "base" and _changed(ref[1], uncropped[k][1]) > 0.01:
                    cutting += 1
                if name == "full":
                    _same(what + ("equals the frame before any crop",), got, before[k])
        assert cutting >= 3, "the sequence must cut into the picture: %d boxes change more than 1 %% of the pixels" % cutting


MODE_BOX = ((5, 7, 9), (50, 61, 43))
MODE_POSE = (35.0, 20.0, 0.0)
# importance cases in which cropping the importances matters (see test_modes): (table, pose, box, least fraction of pixels)
IMP_CASES = {
    "pot, lower half": (POT, (0.0, -80.0, 0.0), ((0, 0, 0), (64, 32, 64)), 0.01),
    "pot, middle": (POT, (0.0, -80.0, 0.0), ((0, 20, 0), (64, 44, 64)), 0.01),
    "canopy, upper half": (CANOPY, (0.0, 80.0, 0.0), ((0, 32, 0), (64, 64, 64)), 0.0),
}


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_modes(oracle, volym_lib, layout):
    """Every mode on an off-centre box.  The importance cases are ones where oracle(cropped density, cropped importances) differs
    from oracle(cropped density, FULL importances): a library that cropped the density alone would fail them."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    lo, hi = MODE_BOX
    cvol = scene.crop_volume(vol, dims, lo, hi)
    imp = CANOPY[labels]
    cimp = scene.crop_volume(imp, dims, lo, hi)
    for filt in (0, 1):
        with _ctx(layout) as dev, _ctx(layout) as twin:
            dev.set_volume(vol, dims, filt)
            dev.set_importances(imp, dims)
            dev.set_transfer_function(lut)
            twin.set_volume(cvol, dims, filt)
            twin.set_importances(cimp, dims)
            twin.set_transfer_function(lut)
            dev.set_crop_box(lo, hi)
            for name in (("base", "no opacity", "smoothing", "colouring") if filt == 0 else ("base", "straight")):
                cam, par, cu, pu = _uniforms(oracle, W, H, MODE_POSE, **PARAMS[name])
                ref = _oracle(oracle, cvol, cimp, dims, cam, par, filter=filt)
                if name == "base" and filt == 0:
                    assert _changed(ref[1], _oracle(oracle, vol, imp, dims, cam, par)[1]) > 0.01, "the box must cut into the picture"
                got = _three(dev, (layout, filt, name), cu, pu)
                _same((layout, filt, name, "twin"), got, _frame(twin, cu, pu))
                _near((layout, filt, name), got, ref)
    for cname, (table, pose, (lo, hi), least) in IMP_CASES.items():
        imp = table[labels]
        cvol, cimp = scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi)
        with _ctx(layout) as dev, _ctx(layout) as twin:
            dev.set_volume(vol, dims, 0)
            dev.set_labels(labels, dims)
            dev.set_segment_importances(table)
            dev.set_transfer_function(lut)
            twin.set_volume(cvol, dims, 0)
            twin.set_importances(cimp, dims)
            twin.set_transfer_function(lut)
            dev.set_crop_box(lo, hi)
            for name in ("straight", "cone"):
                cam, par, cu, pu = _uniforms(oracle, W, H, pose, **PARAMS[name])
                ref = _oracle(oracle, cvol, cimp, dims, cam, par)
                density_only = _oracle(oracle, cvol, imp, dims, cam, par)
                frac = _changed(ref[1], density_only[1])
                print("%s, %s: cropping the importances changes %d of %d pixels" % (cname, name, round(frac * W * H), W * H))
                assert frac > least, (cname, name, frac)
                got = _three(dev, (layout, cname, name), cu, pu)
                _same((layout, cname, name, "twin"), got, _frame(twin, cu, pu))
                _near((layout, cname, name), got, ref)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_order_of_calls(oracle, volym_lib, layout):
    """The box belongs to the scene: importances that arrive after a crop are cropped, in whatever order the calls come."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    table, pose, (lo, hi), _ = IMP_CASES["canopy, upper half"]
    table2 = _table(l2=100, l4=90)             # nothing important: 39 pixels of this view differ from the canopy's
    cam, par, cu, pu = _uniforms(oracle, W, H, pose, **PARAMS["straight"])
    cvol = scene.crop_volume(vol, dims, lo, hi)

    def twin_frame(tab):
        with _ctx(layout) as twin:
            twin.set_volume(cvol, dims, 0)
            twin.set_importances(scene.crop_volume(tab[labels], dims, lo, hi), dims)
            twin.set_transfer_function(lut)
            return _frame(twin, cu, pu)

    want, want2 = twin_frame(table), twin_frame(table2)
    _near("twin against the oracle", want, _oracle(oracle, cvol, scene.crop_volume(table[labels], dims, lo, hi), dims, cam, par))
    assert not np.array_equal(want[1], want2[1]), "the two tables must give different pictures"
    with _ctx(layout) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        dev.set_crop_box(lo, hi)                                     # crop, then set_importances
        dev.set_importances(table[labels], dims)
        _same("crop then set_importances", _three(dev, "crop then set_importances", cu, pu), want)
        dev.set_labels(labels, dims)                                 # crop, then set_labels + set_segment_importances
        _same("set_labels alone leaves the importances", _three(dev, "set_labels"), want)
        dev.set_segment_importances(table2)
        _same("crop then labels + table", _three(dev, "crop then labels + table"), want2)
        dev.set_segment_importances(table)                           # a table edit after the crop
        _same("table edit after crop", _three(dev, "table edit after crop"), want)
        dev.set_labels(labels, dims)                                 # labels again while cropped: the mapped importances stay
        dev.set_crop_box((0, 0, 0), (64, 40, 64))
        dev.set_crop_box(lo, hi)
        _same("labels replaced while cropped", _three(dev, "labels replaced while cropped"), want)
        dev.set_segment_importances(table)
        dev.set_crop_box((0, 0, 0), dims)                            # crop after a table edit
        dev.set_segment_importances(table2)
        dev.set_crop_box(lo, hi)
        _same("crop after table edit", _three(dev, "crop after table edit"), want2)
        assert int(dev.label_counts().sum()) == 64 ** 3              # the whole label volume, whatever the box
        # set_volume resets the box, and the importances get their texels back
        dev.set_volume(vol, dims, 0)
        assert dev.crop_box() == ((0, 0, 0), dims)
        got = _three(dev, "set_volume after a crop", cu, pu)
        _near("set_volume after a crop", got, _oracle(oracle, vol, table2[labels], dims, cam, par))
        dev.set_crop_box(lo, hi)
        dev.set_importances(table[labels], dims)
        dev.set_volume(vol, dims, 0)                                 # the same with uploaded importances
        _near("set_volume after a crop, uploaded importances", _three(dev, "set_volume 2", cu, pu), _oracle(oracle, vol, table[labels], dims, cam, par))


@pytest.mark.parametrize("slots", [1, 2], ids=["one slot", "two in flight"])
def test_edit_between_enqueued_passes(oracle, volym_lib, slots):
    """A pass enqueued before the edit shows the old box, the two enqueued after it the new one, with no volym_update and no
    sync by the caller in between; with VOLYM_OPT_FRAMES_IN_FLIGHT = 2 the later two come from both frame slots."""
    from volym_amd import _lib, scene
    import torch
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    lut = scene.default_lut()
    boxes = [((0, 0, 0), dims), ((0, 0, 0), (64, 64, 40)), ((30, 0, 0), (31, 64, 64)), ((5, 7, 9), (50, 61, 43)), ((0, 0, 0), dims)]
    cam, par, cu, pu = _uniforms(oracle, W, H, (35.0, 20.0, 0.0), **PARAMS["straight"])
    refs = [_oracle(oracle, scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi), dims, cam, par) for lo, hi in boxes]
    assert _changed(refs[1][1], refs[0][1]) > 0.01 and _changed(refs[2][1], refs[1][1]) > 0.01
    bufs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    with _ctx(-1, [(_lib.OPT_FRAMES_IN_FLIGHT, slots)]) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_importances(imp, dims)
        dev.set_transfer_function(lut)
        dev.update(cu, pu)
        for i in range(1, len(boxes)):
            # every pass into a buffer of its own, as a swap chain would have it
            dev.bind_output(None, bufs[0].data_ptr())
            dev.compute_pass()
            dev.set_crop_box(*boxes[i])
            for b in (1, 2):
                dev.bind_output(None, bufs[b].data_ptr())
                dev.compute_pass()
            dev.sync()
            old, new1, new2 = (b.cpu().numpy() for b in bufs)
            for what, got, ref in (("before the edit", old, refs[i - 1]), ("first after", new1, refs[i]), ("second after", new2, refs[i])):
                du8 = int(np.abs(got.astype(np.int32) - ref[1].astype(np.int32)).max())
                assert du8 <= 1, (slots, i, what, du8)
            assert np.array_equal(new1, new2), (slots, i)
        dev.bind_output(None, None)


def test_headline_frame_and_512_bricked(oracle, volym_lib):
    """The path the benchmark times (bonsai 256^3, 1920x1080, no float buffer, cost feedback on) with a crop, then 512^3 in
    bricks; rows sampled."""
    from volym_amd import _lib, demo, scene
    for n, (w, h), pose, layout, boxes in ((256, (1920, 1080), (0.0, 0.0, 0.0), -1, [((0, 0, 0), (256, 256, 160)), ((21, 30, 37), (200, 243, 171)), ((0, 0, 0), (256, 256, 256))]),
                                           (512, (1280, 720), (-30.0, 15.0, 0.0), 1, [((101, 0, 50), (407, 512, 330))])):
        dims, vol, _ = _bonsai(n)
        zero = np.zeros(n ** 3, np.uint8)
        rows = list(range(3, h, 24))
        cam, par, cu, pu = _uniforms(oracle, w, h, pose)
        with demo.GpuContext(w, h, 0) as ctx:
            ctx.set_option(_lib.OPT_VOLUME_LAYOUT, layout)
            ctx.set_volume(vol, dims, 0)
            ctx.set_importances(zero, dims)
            ctx.set_transfer_function(scene.default_lut())
            ctx.update(cu, pu)
            for _ in range(4):
                ctx.compute_pass()
            ctx.settle()
            for lo, hi in boxes:
                ctx.set_crop_box(lo, hi)
                ref = _oracle(oracle, scene.crop_volume(vol, dims, lo, hi), zero, dims, cam, par, w, h, rowlist=rows, want_f32=False)
                first = None
                for k in range(5):                                  # the feedback re-deals the lists along the way
                    ctx.compute_pass()
                    ctx.sync()
                    u8 = ctx.read_rgba8()
                    first = u8 if first is None else first
                    assert np.array_equal(u8, first), (n, lo, hi, k)
                du8 = int(np.abs(u8[rows].astype(np.int32) - ref[1][rows].astype(np.int32)).max())
                assert du8 <= 1, (n, lo, hi, du8)
                assert u8[rows][..., :3].any()
        common._cache.pop(("bonsai", n), None)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_first_crop_of_a_large_volume_and_back(oracle, volym_lib, layout):
    """The first crop makes the uncropped device copies (512^3: 128 MiB each, density and uploaded importances) and at once
    zeroes a thick slab of their sources: the copies must be taken before the slab kernels write.  Widening back to the whole
    volume restores from the copies, so the frame must be bit-equal to the frame before the crop; the cropped frames in
    between are checked against the oracle on sampled rows."""
    from volym_amd import scene
    n, w, h = 512, 640, 360
    dims, vol, labels = _bonsai(n)
    imp = CANOPY[labels]
    del labels
    rows = list(range(2, h, 12))
    cam, par, cu, pu = _uniforms(oracle, w, h, (35.0, 20.0, 0.0), **PARAMS["straight"])
    with _ctx(layout, w=w, h=h) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_importances(imp, dims)
        dev.set_transfer_function(scene.default_lut())
        before = _three(dev, (layout, "before the first crop"), cu, pu)
        _near((layout, "before"), before, _oracle(oracle, vol, imp, dims, cam, par, w, h, rowlist=rows), rows)
        for lo, hi in (((0, 0, 0), (n, n, 300)), ((0, 0, 0), (n, 330, n)), ((171, 0, 0), (n, n, n))):
            dev.set_crop_box(lo, hi)                               # from the whole volume: a thick slab is zeroed
            got = _three(dev, (layout, lo, hi))
            ref = _oracle(oracle, scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi), dims, cam, par, w, h, rowlist=rows)
            _near((layout, lo, hi), got, ref, rows)
            assert not np.array_equal(got[1], before[1]), "the box must cut into the picture"
            dev.set_crop_box((0, 0, 0), dims)
            _same((layout, lo, hi, "back to the whole volume"), _three(dev, (layout, "whole again")), before)
            if lo == (0, 0, 0) and hi[2] == 300:
                # the copies are made again by the first crop after volym_set_volume and after volym_set_importances
                dev.set_volume(vol, dims, 0)
                dev.set_importances(imp, dims)
                dev.update(cu, pu)
    common._cache.pop(("bonsai", n), None)


@pytest.mark.parametrize("world", [2, 4])
def test_mgpu_virtual_ranks(oracle, volym_lib, world):
    from volym_amd import mgpu, scene
    dims, vol, labels = _bonsai()
    table, pose, (lo, hi), _ = IMP_CASES["pot, lower half"]
    imp = table[labels]
    w, h = 310, 170
    cam, par, cu, pu = _uniforms(oracle, w, h, pose, **PARAMS["straight"])
    with mgpu.MultiGpu(w, h, devices=[0] * world, transport=mgpu.COPY) as mg:
        mg.set_volume(vol, dims, 0)
        mg.set_transfer_function(scene.default_lut())
        mg.set_labels(labels, dims)
        mg.set_segment_importances(table)
        def check(what, blo, bhi, t):
            assert t["overflowed"] == 0, (world, what, blo, bhi)
            ref = _oracle(oracle, scene.crop_volume(vol, dims, blo, bhi), scene.crop_volume(imp, dims, blo, bhi), dims, cam, par, w, h, want_f32=False)
            du8 = int(np.abs(mg.read_rgba8().astype(np.int32) - ref[1].astype(np.int32)).max())
            assert du8 <= 1, (world, what, blo, bhi, du8)

        for blo, bhi in ((lo, hi), ((5, 7, 9), (50, 61, 43)), ((0, 0, 0), dims)):
            mg.set_crop_box(blo, bhi)
            mg.update(cu, pu)
            mg.prepare(0)
            check("plain enqueues", blo, bhi, mg.run(3, use_graph=False))
        # The captured loop at a standing view: an edit changes no uniform, so nothing but the set-up call itself tells the loop
        # that the graph it holds was captured for another scene.  The messages were sized for the whole volume just above, which
        # stores the most tiles; the box shrinks, then grows (stale culling would then cut into the picture), with no
        # volym_mgpu_update and no volym_mgpu_prepare in between.  16 frames: a run that captures spends two cycles of the four
        # rotating buffers on warm-up frames, the rest are replays, and the frame read back is a replayed one.
        t = mg.run(4 * 4, use_graph=True)
        assert t["graph_replays"] >= 1
        check("graph, whole volume", (0, 0, 0), dims, t)
        for blo, bhi in (((30, 0, 0), (31, 64, 64)), (lo, hi), ((5, 7, 9), (50, 61, 43)), ((0, 0, 0), dims)):
            mg.set_crop_box(blo, bhi)
            t = mg.run(4 * 4, use_graph=True)
            assert t["graph_replays"] >= 1
            check("graph after an edit at a standing view", blo, bhi, t)


def test_errors_leave_the_context_rendering(oracle, volym_lib):
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    cam, par, cu, pu = _uniforms(oracle, W, H, (35.0, 20.0, 0.0))
    with _ctx(-1) as c:
        for call in (lambda: c.set_crop_box((0, 0, 0), (1, 1, 1)), c.crop_box):
            with pytest.raises(_lib.VolymError) as e:                  # no volume yet
                call()
            assert e.value.code == _lib.E_STATE
        c.set_volume(vol, dims, 0)
        c.set_importances(imp, dims)
        c.set_transfer_function(scene.default_lut())
        lo, hi = (0, 0, 0), (64, 64, 40)
        c.set_crop_box(lo, hi)
        for blo, bhi in (((3, 0, 0), (2, 64, 64)), ((0, 0, 0), (65, 64, 64)), ((0, 0, 0), (64, 64, 2 ** 31)), ((0, 65, 0), (64, 65, 64))):
            with pytest.raises(_lib.VolymError) as e:
                c.set_crop_box(blo, bhi)
            assert e.value.code == _lib.E_INVALID
            assert c.crop_box() == (lo, hi)
        assert _lib.lib().volym_set_crop_box(c.handle, None, (C.c_uint32 * 3)(1, 1, 1)) == _lib.E_INVALID
        got = _three(c, "after the refused boxes", cu, pu)
        _near("after the refused boxes", got, _oracle(oracle, scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi), dims, cam, par))


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_fetch_counters(oracle, volym_lib, layout):
    """volym_stats_pass counts the reference's fetches (the instrumented launch takes the general form and counts a look-ahead
    probe whether or not the reject box spares its fetch), so after a crop they equal the twin's, whose reject box comes from a
    scan of the zeroed bytes and may be tighter, and the oracle's on the zeroed inputs."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    table, pose, (lo, hi), _ = IMP_CASES["pot, lower half"]
    imp = table[labels]
    cvol, cimp = scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi)
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_importances(imp, dims)
        dev.set_transfer_function(scene.default_lut())
        dev.set_crop_box(lo, hi)
        twin.set_volume(cvol, dims, 0)
        twin.set_importances(cimp, dims)
        twin.set_transfer_function(scene.default_lut())
        for name in ("base", "straight", "cone"):
            cam, par, cu, pu = _uniforms(oracle, W, H, pose, **PARAMS[name])
            dev.update(cu, pu)
            twin.update(cu, pu)
            got, want = dev.stats_pass(), twin.stats_pass()
            assert got == want, (name, got, want)
            ref = _oracle(oracle, cvol, cimp, dims, cam, par)[2]
            for k in ("n_vol", "n_imp", "n_steps", "n_dense", "n_hit"):
                assert got[k] == ref[k], (name, k, got[k], ref[k])


def test_simple_set_crop(oracle, volym_lib):
    """demo.Simple.set_crop: unit-cube coordinates, texel = floor(p * n + 0.5)."""
    from volym_amd import demo, scene
    raw, labels_raw = common.bonsai(64)
    dims = (64, 64, 64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    with demo.GpuContext(W, H, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        lo, hi = d.set_crop(ctx, (0.0, 0.1, 0.0), (1.0, 1.0, 0.625))
        assert (lo, hi) == ((0, 6, 0), (64, 64, 40)) and ctx.crop_box() == (lo, hi)
        d.compute_pass(ctx)
        ctx.sync()
        vol, imp = common.oracle_scene(oracle, raw, labels_raw, common.BONSAI_SEGMENTS, dims)
        cam = oracle.benchmark_camera_uniforms(W / H)
        par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01)
        ref = _oracle(oracle, scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi), dims, cam, par, want_f32=False)
        assert int(np.abs(ctx.read_rgba8().astype(np.int32) - ref[1].astype(np.int32)).max()) <= 1
