"""The slice pass on the device (volym_slice_pass / volym_read_slice / volym_slice_device_ptr).

The expected image is scene.slice_frame, the host twin of the rule (pinned to a plain triple loop by tests/test_slice_host.py), of the
prepared arrays the context was given and the cut state it was put in.  Every comparison is over every byte of every pixel: the rule
is integer, so there is no tolerance and no pixel is left out.

The volume is 37 x 22 x 19: no axis is a multiple of 4, so the bricked layout's padding is exercised; the output sizes 70 x 9 and
65 x 17 are ragged against 64 lanes, 8 x 8 and 16 x 16 blocks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_crop_box import CANOPY, _bonsai, _uniforms, _ctx

pytestmark = pytest.mark.gpu

DIMS = (37, 22, 19)
SIZES = ((70, 9), (65, 17))
BACKGROUND, CUT_RGBA = (9, 80, 200, 33), (250, 30, 60, 140)
BOX = ((3, 2, 1), (33, 20, 17))
PLANE = ((5, -3, 7), 150)
HIDDEN = [2]


def _same(what, got, want):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:6].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


class Host:
    """what the context was given, and the cut state it is in: the arguments of scene.slice_frame"""

    def __init__(self, dims=DIMS, seed=7):
        rng = np.random.default_rng(seed)
        nx, ny, nz = dims
        self.dims = dims
        self.vol = rng.integers(1, 256, nx * ny * nz).astype(np.uint8)         # no zero byte: a cut texel shows
        zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        self.labels = (((xx // 5) + (yy // 4) * 2 + (zz // 3)) % 5).astype(np.uint8).ravel()
        self.table = rng.integers(0, 256, 256).astype(np.uint8)
        self.lut = rng.integers(0, 256, (7, 4)).astype(np.uint8)
        self.palette = rng.integers(0, 256, (256, 4)).astype(np.uint8)
        self.palette[1, 3], self.palette[3, 3] = 0, 255
        self.cut = None                 # never cut
        self.ever_cut = False

    def upload(self, ctx, labels_layout=None, labels=True):
        from volym_amd import _lib
        ctx.set_volume(self.vol, self.dims, 0)
        ctx.set_transfer_function(self.lut)
        if labels:
            if labels_layout is not None:
                ctx.set_option(_lib.OPT_VOLUME_LAYOUT, labels_layout)
            ctx.set_labels(self.labels, self.dims)
            ctx.set_segment_importances(self.table)

    def set_cut(self, ctx, box=None, plane=None, hidden=None):
        """put the context and this record into the cut state (box, plane, hidden labels); None: that cut is lifted"""
        from volym_amd import scene
        if self.cut is None:
            self.cut = {"box": ((0, 0, 0), self.dims), "plane": ((0, 0, 0), 0), "visible": np.ones(256, np.uint8)}
        new = {"box": box or ((0, 0, 0), self.dims), "plane": plane or ((0, 0, 0), 0), "visible": scene.visibility_mask(hidden or [])}
        if new["box"] != self.cut["box"]:
            ctx.set_crop_box(*new["box"])
        if new["plane"] != self.cut["plane"]:
            ctx.set_clip_plane(*new["plane"])
        if not np.array_equal(new["visible"], self.cut["visible"]):
            ctx.set_segment_visibility(new["visible"])
        self.cut = new
        self.ever_cut = self.ever_cut or box is not None or plane is not None or bool(hidden)

    def want(self, s):
        from volym_amd import scene
        now = scene.cut_volume(self.vol, self.dims, self.cut, self.labels)
        imp = scene.cut_volume(self.table[self.labels], self.dims, self.cut, self.labels)
        return scene.slice_frame(now, self.dims, s, lut=self.lut, labels=self.labels, importances=imp, cut=self.cut,
                                 uncut=self.vol if self.ever_cut else None)


def _geometries(dims=DIMS):
    """(name, slice): every geometry of the issue at both output sizes.  Colours, mode and flags are set by the caller."""
    from volym_amd import scene
    nx, ny, nz = dims
    out = []
    for axis, n in zip("xyz", dims):
        for index in (0, n // 2, n - 1):
            s = scene.slice_axis(axis, index, dims)
            out.append(("axis %s at %d, its own size" % (axis, index), s))
            for w, h in SIZES:                                   # the same map over a ragged output: the volume ends inside it
                out.append(("axis %s at %d, %d x %d" % (axis, index, w, h), s.replace(width=w, height=h)))
    centre = (nx / 2.0, ny / 2.0, nz / 2.0)
    for w, h in SIZES:
        # oblique, fractional steps, a negative du component
        out.append(("oblique %d x %d" % (w, h), scene.Slice((2 * 65536 + 777, 21 * 65536 + 40000, 3 * 65536), (31000, -17011, 9000), (20000, 7001, 60500), w, h)))
        out.append(("slice_through %d x %d" % (w, h), scene.slice_through(centre, (5, -3, 7), (0, 0, 1), (w, h), 0.6)))
        # magnified: 0.25 texel per pixel; minified: 3.5
        out.append(("magnified %d x %d" % (w, h), scene.Slice((10 * 65536 + 100, 9 * 65536 + 0x8000, 8 * 65536 + 0x8000), (16384, 0, 0), (0, 16384, 0), w, h)))
        out.append(("magnified oblique %d x %d" % (w, h), scene.slice_through(centre, (1, 1, 1), (0, 1, 0), (w, h), 0.25)))
        out.append(("minified %d x %d" % (w, h), scene.Slice((-40 * 65536, 0x8000, -5 * 65536), (229376, 0, 0), (0, 0, 229376), w, h)))
        out.append(("minified oblique %d x %d" % (w, h), scene.slice_through(centre, (2, -1, 3), (0, 1, 0), (w, h), 3.5)))
        # leaves the volume on two sides: starts left of x = 0 and ends above y = ny
        out.append(("two sides %d x %d" % (w, h), scene.Slice((-6 * 65536 - 1, 15 * 65536, 9 * 65536 + 0x8000), (65536, 0, 0), (0, 65536, 0), w, h)))
        # wholly outside: beyond z = nz, and at negative coordinates
        out.append(("outside %d x %d" % (w, h), scene.Slice((0x8000, 0x8000, nz * 65536), (65536, 0, 0), (0, 65536, 0), w, h)))
        out.append(("outside, negative %d x %d" % (w, h), scene.Slice((-1, 0x8000, 0x8000), (0, 65536, 0), (0, 0, 65536), w, h)))
    # products that wrap 32 bits: 8192 pixels, a step of almost +-2 texels; du[1] < 0 is a large unsigned number and i * du[1] wraps
    # from the second pixel on, i * du[0] passes 2^30.  Pixel 4096 shows texel (0, 10, 5).
    wrap = scene.Slice((-4096 * 131071 + 20000, 4096 * 130001 + 10 * 65536 + 100, 5 * 65536 + 0x8000), (131071, -130001, 0), (0, 0, 0), 8192, 1)
    assert scene.slice_texel(wrap, 4096, 0) == (0, 10, 5)
    out.append(("wrap 8192 x 1", wrap))
    out.append(("wrap 1 x 8192", scene.Slice(wrap.origin, (0, 0, 0), wrap.du, 1, 8192)))
    return [(name, scene.check_slice(s)) for name, s in out]


def _dress(s, host, mode=0, flags=0):
    return s.replace(mode=mode, flags=flags, background=BACKGROUND, cut_rgba=CUT_RGBA, palette=host.palette)


def _check(ctx, host, what, s):
    ctx.slice_pass(s)
    got = ctx.read_slice()
    want = host.want(s)
    _same(what, got, want)
    return want


MODES_FLAGS = [(m, f) for m in (0, 1, 2) for f in range(8) if not (m == 2 and f & 1)]


# ---- 1. geometry, modes and flags, both layouts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_every_geometry_in_every_mode(volym_lib, layout):
    host = Host()
    inside = outside = 0
    with _ctx(layout) as ctx:
        host.upload(ctx)
        assert ctx.slice_device_ptr() is None
        for k, (name, s) in enumerate(_geometries()):
            # every geometry in DENSITY and in the fullest combination; every mode and flag combination on a rotating subset
            combos = [(0, 0), (1, 6), (2, 6)] + [MODES_FLAGS[(k + i * 7) % len(MODES_FLAGS)] for i in range(3)]
            for mode, flags in combos:
                want = _check(ctx, host, (name, mode, flags), _dress(s, host, mode, flags))
            bg = (want == np.array(BACKGROUND, np.uint8)).all(-1)
            inside += int((~bg).sum())
            outside += int(bg.sum())
            if name.startswith("outside"):
                assert bg.all(), name
            if name.startswith(("two sides", "wrap")):
                assert bg.any() and not bg.all(), name
        assert inside > 5000 and outside > 5000


@pytest.mark.parametrize("layout", [0, 1])
def test_every_mode_and_flag_combination(volym_lib, layout):
    """all twenty valid combinations on an oblique slice under a crop box, a plane and a hidden segment"""
    host = Host()
    with _ctx(layout) as ctx:
        host.upload(ctx)
        host.set_cut(ctx, BOX, PLANE, HIDDEN)
        geo = dict(_geometries())
        for name in ("oblique 70 x 9", "slice_through 65 x 17", "axis y at 11, 65 x 17"):
            seen = set()
            for mode, flags in MODES_FLAGS:
                want = _check(ctx, host, (name, mode, flags), _dress(geo[name], host, mode, flags))
                seen.add(want.tobytes())
            assert len(seen) == len(MODES_FLAGS), (name, len(seen))            # no two combinations show the same image


@pytest.mark.parametrize("tf_n", [1, 7, 256])
def test_transfer_function_tables(volym_lib, tf_n):
    from volym_amd import _lib
    host = Host()
    host.lut = np.random.default_rng(tf_n).integers(0, 256, (tf_n, 4)).astype(np.uint8)
    geo = dict(_geometries())
    for layout in (0, 1):
        with _ctx(layout) as ctx:
            host.upload(ctx)
            for name in ("oblique 65 x 17", "axis z at 9, its own size"):
                want = _check(ctx, host, (name, tf_n, layout), _dress(geo[name], host, _lib.SLICE_TF, 0))
                shown = want[(want != np.array(BACKGROUND, np.uint8)).any(-1)]
                assert len(shown) > 100
                if tf_n == 1:
                    assert (shown == np.append(host.lut[0, :3], 255)).all()


@pytest.mark.parametrize("layout", [0, 1])
def test_labels_in_the_other_layout_than_the_volume(volym_lib, layout):
    from volym_amd import _lib
    host = Host()
    geo = dict(_geometries())
    with _ctx(layout) as ctx:
        host.upload(ctx, labels_layout=1 - layout)
        for name in ("oblique 70 x 9", "axis x at 18, 65 x 17", "minified oblique 65 x 17"):
            for mode in (0, 1, 2):
                _check(ctx, host, (name, mode), _dress(geo[name], host, mode, _lib.SLICE_LABELS | _lib.SLICE_MARK_CUT))


# ---- 2. cuts: MARK_CUT and UNCUT before and after each edit, no volym_update in between ---------------------------------------------
@pytest.mark.parametrize("layout", [0, 1])
def test_mark_cut_and_uncut_follow_every_edit(volym_lib, layout):
    from volym_amd import _lib
    host = Host()
    geo = dict(_geometries())
    names = ("oblique 65 x 17", "axis z at 9, 70 x 9", "slice_through 70 x 9")
    combos = [(0, 0), (0, _lib.SLICE_UNCUT), (0, _lib.SLICE_MARK_CUT), (0, _lib.SLICE_MARK_CUT | _lib.SLICE_UNCUT), (1, 7), (2, 6)]

    def look(step):
        images = []
        for name in names:
            for mode, flags in combos:
                images.append(_check(ctx, host, (step, name, mode, flags), _dress(geo[name], host, mode, flags)))
        return images

    with _ctx(layout) as ctx:                                    # no volym_update anywhere in this test
        host.upload(ctx)
        never = look("never cut")
        steps = [("box", BOX, None, None), ("box + plane", BOX, PLANE, None), ("box + plane + hidden", BOX, PLANE, HIDDEN),
                 ("plane + hidden", None, PLANE, HIDDEN), ("hidden", None, None, HIDDEN), ("all lifted", None, None, None)]
        before = never
        for step, box, plane, hidden in steps:
            host.set_cut(ctx, box, plane, hidden)
            after = look(step)
            if step != "all lifted":
                assert any(not np.array_equal(a, b) for a, b in zip(before, after)), step     # the edit shows
            for k, name in enumerate(names):                    # UNCUT without MARK_CUT never changes
                assert np.array_equal(after[k * len(combos) + 1], never[k * len(combos) + 1]), (step, name)
            before = after
        for a, b in zip(after, never):
            assert np.array_equal(a, b)


def test_uncut_in_a_context_that_never_cut(volym_lib):
    from volym_amd import _lib
    host = Host()
    geo = dict(_geometries())
    for layout in (0, 1):
        with _ctx(layout) as ctx:
            host.upload(ctx)
            for name in ("oblique 70 x 9", "axis y at 11, its own size"):
                plain = _check(ctx, host, (name, "plain"), _dress(geo[name], host, 0, 0))
                for mode in (0, 1):
                    _check(ctx, host, (name, mode, "uncut"), _dress(geo[name], host, mode, _lib.SLICE_UNCUT | _lib.SLICE_MARK_CUT))
                _same((name, "uncut is plain"), _check(ctx, host, (name, "uncut"), _dress(geo[name], host, 0, _lib.SLICE_UNCUT)), plain)


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def _bonsai_scene(ctx, oracle):
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    ctx.set_volume(vol, dims, 0)
    ctx.set_transfer_function(scene.default_lut())
    ctx.set_labels(labels, dims)
    ctx.set_segment_importances(CANOPY)
    return dims, vol, labels


def _bonsai_slice(dims, flags=0, mode=1):
    from volym_amd import scene
    pal = np.zeros((256, 4), np.uint8)
    pal[2], pal[3], pal[4] = (0, 255, 0, 90), (160, 82, 45, 90), (200, 200, 200, 90)
    return scene.slice_through((32.0, 30.0, 33.0), (1, 2, -1), (0, 0, 1), (70, 65), 1.0, mode=mode, flags=flags, palette=pal, background=BACKGROUND)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_a_frame_is_the_same_with_and_without_slice_passes(oracle, volym_lib, in_flight):
    from volym_amd import _lib, scene
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, in_flight)], w=160, h=96) as ctx:
        dims, vol, labels = _bonsai_scene(ctx, oracle)
        s = _bonsai_slice(dims, _lib.SLICE_LABELS)
        want = scene.slice_frame(vol, dims, s, lut=scene.default_lut(), labels=labels)
        assert len(np.unique(want.reshape(-1, 4), axis=0)) > 20, "the slice must be a picture"
        # before any volym_update or compute pass
        ctx.slice_pass(s)
        _same("before any update", ctx.read_slice(), want)
        cam, par, cu, pu = _uniforms(oracle, 160, 96, (35.0, 20.0, 0.0))
        ctx.update(cu, pu)
        for _ in range(in_flight):
            ctx.compute_pass()
        frame = ctx.read_rgba8()
        assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 50, "the frame must be a picture"
        ctx.slice_pass(s)
        _same("frame read after a slice pass", ctx.read_rgba8(), frame)
        for k in range(3):                                      # slices between frames that alternate between the slots
            ctx.compute_pass()
            ctx.slice_pass(s)
            ctx.compute_pass()
            _same(("frame", k), ctx.read_rgba8(), frame)
            _same(("slice", k), ctx.read_slice(), want)


def test_a_sharded_context_slices_the_whole_volume(oracle, volym_lib):
    from volym_amd import _lib, scene
    with _ctx(0, w=160, h=96) as ctx:
        ctx.set_shard(1, 2)
        dims, vol, labels = _bonsai_scene(ctx, oracle)
        for flags in (0, _lib.SLICE_LABELS | _lib.SLICE_MARK_CUT):
            s = _bonsai_slice(dims, flags)
            ctx.slice_pass(s)
            _same(("sharded", flags), ctx.read_slice(), scene.slice_frame(vol, dims, s, lut=scene.default_lut(), labels=labels))


# ---- 4. targets -------------------------------------------------------------------------------------------------------------------
def test_targets(volym_lib):
    host = Host()
    geo = dict(_geometries())
    with _ctx(1) as ctx:
        host.upload(ctx)
        assert ctx.slice_device_ptr() is None
        small = _dress(geo["oblique 70 x 9"], host, 1, 6)
        other = _dress(geo["oblique 70 x 9"], host, 0, 2)
        large = _dress(geo["slice_through 65 x 17"], host, 0, 2)
        assert not np.array_equal(host.want(small), host.want(other))
        # the own target grows, then shrinks: the read is that of the latest pass, and no smaller buffer is made
        _check(ctx, host, "small", small)
        assert ctx.slice_device_ptr()
        _check(ctx, host, "grown", large)
        p_large = ctx.slice_device_ptr()
        _check(ctx, host, "shrunk", small)
        assert ctx.slice_device_ptr() == p_large
        # a caller's tensor, with a guard behind it; the own target and its read stay what they were
        n = small.width * small.height * 4
        holder = torch.full((n + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.slice_pass(other, target_ptr=holder.data_ptr())
        ctx.sync()
        got = holder.cpu().numpy()
        _same("caller's tensor", got[:n].reshape(other.height, other.width, 4), host.want(other))
        assert (got[n:] == 0xA5).all(), "the pass wrote behind its target"
        _same("own target after a pass into a caller's", ctx.read_slice(), host.want(small))
        # slice_device_ptr is the buffer read_slice reads: a pass of the same size into it, as a caller's target, shows in the read
        ctx.slice_pass(other, target_ptr=ctx.slice_device_ptr())
        _same("a pass into slice_device_ptr", ctx.read_slice(), host.want(other))


def test_size_check_1024_squared_of_256_cubed(volym_lib):
    """the one large case: 1024 x 1024 pixels of a 256^3 synthetic volume with labels, oblique, every flag"""
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai(256)
    rng = np.random.default_rng(1)
    pal = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    lut = scene.default_lut()
    cut = {"box": ((10, 20, 30), (250, 240, 230)), "plane": ((3, 1, -2), 300), "visible": scene.visibility_mask([3])}
    with _ctx(-1) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_transfer_function(lut)
        ctx.set_labels(labels, dims)
        ctx.set_crop_box(*cut["box"])
        ctx.set_clip_plane(*cut["plane"])
        ctx.set_segment_visibility(cut["visible"])
        now = scene.cut_volume(vol, dims, cut, labels)
        for s in (scene.slice_through((128.0, 128.0, 128.0), (1, 2, 3), (0, 0, 1), (1024, 1024), 0.3, mode=1, flags=7, palette=pal, cut_rgba=CUT_RGBA),
                  scene.slice_axis("x", 128, dims).replace(width=1024, height=1024, du=(0, 16384, 0), dv=(0, 0, 16384), flags=6, palette=pal,
                                                           cut_rgba=CUT_RGBA, background=BACKGROUND)):
            ctx.slice_pass(s)
            _same("1024 x 1024", ctx.read_slice(), scene.slice_frame(now, dims, s, lut=lut, labels=labels, cut=cut, uncut=vol))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *a, **kw):
    from volym_amd import _lib
    with pytest.raises(_lib.VolymError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals(volym_lib):
    from volym_amd import _lib, scene
    host = Host()
    s = _dress(scene.slice_axis("z", 3, DIMS), host)
    with _ctx(0) as ctx:
        _refused(_lib.E_STATE, ctx.slice_pass, s)                               # no volume
        _refused(_lib.E_STATE, ctx.read_slice)
        host.upload(ctx, labels=False)
        ctx.slice_pass(s)                                                       # DENSITY needs the volume alone
        _refused(_lib.E_STATE, ctx.slice_pass, s.replace(flags=_lib.SLICE_LABELS))         # no labels
        _refused(_lib.E_STATE, ctx.slice_pass, s.replace(mode=_lib.SLICE_IMPORTANCE))      # no importances
        ctx.slice_pass(s.replace(flags=_lib.SLICE_MARK_CUT))                    # MARK_CUT needs no labels: box and plane alone
        # labels and importances of other dimensions than the volume's count as absent
        other = (DIMS[0] + 1, DIMS[1], DIMS[2])
        ctx.set_labels(np.zeros(other[0] * other[1] * other[2], np.uint8), other)
        _refused(_lib.E_STATE, ctx.slice_pass, s.replace(flags=_lib.SLICE_LABELS))
        ctx.set_importances(np.zeros(other[0] * other[1] * other[2], np.uint8), other)
        _refused(_lib.E_STATE, ctx.slice_pass, s.replace(mode=_lib.SLICE_IMPORTANCE))
        # invalid slices
        _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(mode=3))
        _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(flags=8))
        _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(mode=_lib.SLICE_IMPORTANCE, flags=_lib.SLICE_UNCUT))
        for w, h in ((0, 4), (4, 0), (8193, 1), (1, 8193)):
            _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(width=w, height=h))
        _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(origin=(1 << 30, 0, 0)))
        _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(origin=(-(1 << 30) - 1, 0, 0)))
        _refused(_lib.E_INVALID, ctx.slice_pass, s.replace(du=(1 << 25, 0, 0), width=64))      # the far corner leaves the range
        assert volym_lib.volym_slice_pass(ctx.handle, None, None) == _lib.E_INVALID
        assert volym_lib.volym_slice_pass(None, C.byref(s.to_c()), None) == _lib.E_INVALID
        assert volym_lib.volym_read_slice(ctx.handle, None) == _lib.E_INVALID
        # a refused pass leaves the latest image readable
        _same("after the refusals", ctx.read_slice(), host.want(s.replace(flags=_lib.SLICE_MARK_CUT)))
    with _ctx(1) as ctx:
        ctx.set_volume(host.vol, DIMS, 0)
        _refused(_lib.E_STATE, ctx.slice_pass, s.replace(mode=_lib.SLICE_TF))   # no transfer function
        holder = torch.zeros(s.width * s.height * 4, dtype=torch.uint8, device="cuda")
        ctx.slice_pass(s, target_ptr=holder.data_ptr())
        ctx.sync()
        _refused(_lib.E_STATE, ctx.read_slice)                                  # no pass into the context's own target yet
        assert ctx.slice_device_ptr() is None
