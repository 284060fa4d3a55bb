"""The frame loops bench.py times, frame by frame against the CPU oracle.

bench.py's timed loop keeps two frames in flight (VOLYM_OPT_FRAMES_IN_FLIGHT = 2: compute passes alternate between the
two frame slots of the context), renders into a caller-owned buffer bound with volym_bind_output, writes no float side buffer (the
16-byte super-fill stores) and runs work lists dealt by the cost feedback.  Its turntable runs up to three frames ahead of
the device, each frame on lists dealt on earlier views.  These tests check every frame of such loops -- frames of both
frame contexts -- against the oracle (rgba8 within 1 LSB), on rows sampled every 8th row and shifted by the frame's index,
so that consecutive frames together cover every row.
"""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu

STEP = 0.01                 # bench.py --step
SENTINEL = 0xA5             # what a buffer holds before a pass: a pixel nobody wrote is 0xa5a5a5a5, never an oracle pixel
ROW_STRIDE = 8

_scenes = {}
_refs = {}


def _scene(O, n):
    """(device inputs as bench.py prepares them, oracle inputs) of bonsai n^3"""
    if n not in _scenes:
        from volym_amd import scene
        raw, labels = common.bonsai(n)
        dims = (n, n, n)
        dev = (scene.prepare_volume(raw, dims, True),
               scene.prepare_volume(scene.map_segments_to_importance(labels, common.BONSAI_SEGMENTS), dims, True),
               scene.default_lut())
        vol, imp = common.oracle_scene(O, raw, labels, common.BONSAI_SEGMENTS, dims)
        _scenes[n] = (dims, dev, (vol, imp, O.tf_default_lut()))
    return _scenes[n]


def _params(importance=0, cone=0):
    from volym_amd import scene
    return scene.StateParameters.benchmark().replace(raymarching_step_size=STEP, use_importance_rendering=importance,
                                                     use_cone_importance_check=cone)


def _params_state(W, H, **kw):
    from volym_amd import scene
    st = scene.State.with_parameters(W / H, _params(**kw))
    st.update()                  # the frame loop's orbit(0,0,0): eye -> (0.5,0.5,1.5)  (src/event_loop.rs:100)
    return st


def _context(O, W, H, n, flight, state):
    """bench.py make_context with its defaults: kernel 2, the library's layout and depth-parallel choice, nearest filter"""
    from volym_amd import _lib, demo
    dims, (volume, importances, lut), _ = _scene(O, n)
    ctx = demo.GpuContext(W, H, 0)
    if flight == 2:
        ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 2)
    ctx.set_option(_lib.OPT_KERNEL, 2)
    ctx.set_volume(volume, dims, _lib.FILTER_NEAREST)
    ctx.set_importances(importances, dims)
    ctx.set_transfer_function(lut)
    ctx.update(state.camera_uniforms(), state.parameter_uniforms())
    return ctx


def _buffer(W, H):
    """a device frame buffer as bench.py allocates it, filled with the sentinel (and the fill finished)"""
    b = torch.empty(W * H * 4, dtype=torch.uint8, device="cuda")
    b.fill_(SENTINEL)
    torch.cuda.synchronize()
    return b


def _host(buf, W, H):
    return buf.cpu().numpy().reshape(H, W, 4)


def _reference(O, n, W, H, cu, pu, rows):
    """oracle rgba8 of the view (camera / parameter uniforms of the library) on `rows` (None: every row)"""
    key = (n, W, H, bytes(cu), bytes(pu), None if rows is None else tuple(rows))
    if key not in _refs:
        dims, _, (vol, imp, lut) = _scene(O, n)
        cam = O.CameraUniforms.from_buffer_copy(bytes(cu))
        par = O.Parameters.from_buffer_copy(bytes(pu))
        _, ref, _ = O.render(vol, imp, dims, lut, cam, par, W, H, rowlist=None if rows is None else list(rows), want_f32=False)
        _refs[key] = ref
    return _refs[key]


def _check(O, n, got, cu, pu, rows, label):
    W, H = got.shape[1], got.shape[0]
    rows = list(range(H)) if rows is None else list(rows)
    ref = _reference(O, n, W, H, cu, pu, None if len(rows) == H else rows)
    d = np.abs(got[rows].astype(np.int32) - ref[rows].astype(np.int32))
    bad = d.max(axis=-1) > 1
    assert not bad.any(), "%s: %d of %d sampled pixels differ from the oracle by more than 1 LSB (max %d; first at row %d)" % (
        label, int(bad.sum()), bad.size, int(d.max()), rows[int(np.argwhere(bad)[0][0])])


def _rows(k, H):
    return range(k % ROW_STRIDE, H, ROW_STRIDE)


def _turntable(W, H, degrees, params):
    """(camera, parameter uniforms) of consecutive views of bench.py's turntable: `degrees` = list of the rotations between views"""
    from volym_amd import scene
    st = scene.State.with_parameters(W / H, params)
    views = []
    for deg in degrees:
        st.process_mouse(-deg / 0.2, 0.0)          # sensitivity 0.2 degrees per pixel (src/state.rs:63)
        st.update()
        views.append((st.camera_uniforms(), st.parameter_uniforms()))
    return views


def _standing(ctx, state):
    """a settled standing view, as bench.py reaches one before its loops"""
    ctx.update(state.camera_uniforms(), state.parameter_uniforms())
    for _ in range(2):                       # a measuring list first, then the final one
        for _ in range(3):
            ctx.compute_pass()
        ctx.sync()
        ctx.settle()


def _run_ahead(ctx, views, kernels=None):
    """bench.py's turntable: per view a buffer of its own bound, update, compute pass, throttle(3); no sync until the end.
    kernels: VOLYM_OPT_KERNEL per view (None: leave it).  Returns the buffers, one per view."""
    from volym_amd import _lib
    bufs = [_buffer(ctx.width, ctx.height) for _ in views]
    for k, (cu, pu) in enumerate(views):
        if kernels is not None:
            ctx.set_option(_lib.OPT_KERNEL, kernels[k])
        ctx.bind_output(None, bufs[k].data_ptr())
        ctx.update(cu, pu)
        ctx.compute_pass()
        ctx.throttle(3)
    ctx.sync()
    assert ctx.frame_device_ptr() == bufs[-1].data_ptr()
    return bufs


# ---- 1. volym_bind_output and volym_frame_device_ptr with a second frame slot ------------------------------------------

def test_bind_output_with_twin(oracle, volym_lib):
    """Both frame contexts render into the bound buffer; NULL gives each its own back; the binding survives the way back
    to one frame in flight.  Each pass renders another view into a buffer refilled with the sentinel, so a pass that went
    elsewhere leaves the sentinel or the previous view behind."""
    from volym_amd import _lib
    W, H, n = 200, 120, 64
    views = _turntable(W, H, [0.0] + [7.0] * 9, _params())
    with _context(oracle, W, H, n, 2, _params_state(W, H)) as ctx:
        buf = _buffer(W, H)
        ctx.bind_output(None, buf.data_ptr())
        for k in range(4):                           # passes 0 and 2 on slot 0, 1 and 3 on slot 1
            cu, pu = views[k]
            buf.fill_(SENTINEL)
            torch.cuda.synchronize()
            ctx.update(cu, pu)
            ctx.compute_pass()
            ctx.sync()
            assert ctx.frame_device_ptr() == buf.data_ptr(), "pass %d: volym_frame_device_ptr is not the bound buffer" % k
            got = _host(buf, W, H)
            _check(oracle, n, got, cu, pu, None, "bound buffer after pass %d (%s)" % (k, "twin" if k & 1 else "context"))
            assert np.array_equal(ctx.read_rgba8(), got), k
        # NULL: each context renders into its own buffer again, and the caller's buffer is left alone
        ctx.bind_output(None, None)
        buf.fill_(SENTINEL)
        torch.cuda.synchronize()
        own = []
        for k in range(4, 6):
            cu, pu = views[k]
            ctx.update(cu, pu)
            ctx.compute_pass()
            ctx.sync()
            own.append(ctx.frame_device_ptr())
            _check(oracle, n, ctx.read_rgba8(), cu, pu, None, "read_rgba8 after pass %d, unbound" % k)
        assert own[0] != own[1] and buf.data_ptr() not in own
        assert (_host(buf, W, H) == SENTINEL).all(), "a pass wrote into the buffer after volym_bind_output(NULL)"
        # back to one frame in flight with a buffer bound: the buffer stays bound
        ctx.bind_output(None, buf.data_ptr())
        ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 1)
        for k in range(6, 8):
            cu, pu = views[k]
            buf.fill_(SENTINEL)
            torch.cuda.synchronize()
            ctx.update(cu, pu)
            ctx.compute_pass()
            ctx.sync()
            assert ctx.frame_device_ptr() == buf.data_ptr()
            got = _host(buf, W, H)
            _check(oracle, n, got, cu, pu, None, "bound buffer after pass %d, one frame in flight" % k)
            assert np.array_equal(ctx.read_rgba8(), got), k


def test_bind_output_before_twin_and_twin_buffer(oracle, volym_lib):
    """A buffer bound before VOLYM_OPT_FRAMES_IN_FLIGHT = 2 is the second frame slot's too; a context that had that slot's own
    buffer bound takes its own back when the slot goes (nothing points at the freed buffer)."""
    from volym_amd import _lib, demo
    W, H, n = 200, 120, 64
    dims, (volume, importances, lut), _ = _scene(oracle, n)
    views = _turntable(W, H, [0.0] + [11.0] * 5, _params(importance=1))
    with demo.GpuContext(W, H, 0) as ctx:
        buf = _buffer(W, H)
        ctx.bind_output(None, buf.data_ptr())
        ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 2)
        ctx.set_volume(volume, dims, _lib.FILTER_NEAREST)
        ctx.set_importances(importances, dims)
        ctx.set_transfer_function(lut)
        for k in range(2):
            cu, pu = views[k]
            buf.fill_(SENTINEL)
            torch.cuda.synchronize()
            ctx.update(cu, pu)
            ctx.compute_pass()
            ctx.sync()
            assert ctx.frame_device_ptr() == buf.data_ptr()
            _check(oracle, n, _host(buf, W, H), cu, pu, None, "buffer bound before the twin, pass %d" % k)
        ctx.bind_output(None, None)
        for k in range(2, 4):
            ctx.update(*views[k])
            ctx.compute_pass()
        ctx.sync()
        twin_own = ctx.frame_device_ptr()            # slot 1 ran the latest pass: its own buffer
        ctx.bind_output(None, twin_own)
        ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 1)
        assert ctx.frame_device_ptr() != twin_own
        cu, pu = views[4]
        ctx.update(cu, pu)
        ctx.compute_pass()
        ctx.sync()
        _check(oracle, n, ctx.read_rgba8(), cu, pu, None, "one frame in flight after the twin's buffer was bound")


# ---- 2. the timed path: bench workload, two frames in flight, a bound buffer --------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(importance=1), dict(importance=1, cone=1)], ids=["base", "importance", "cone"])
def test_timed_path_two_in_flight(oracle, volym_lib, kw):
    """bench.py's steady state: warm-up, sync, settle, then passes of the bench view on both frame contexts.  Every checked
    frame -- the bound buffer, refilled with the sentinel before each pass, and read_rgba8 -- is bit-equal to a fresh
    one-frame context's first frame, and that frame is within 1 LSB of the oracle on every row."""
    W, H, n = 1920, 1080, 256
    state = _params_state(W, H, **kw)
    with _context(oracle, W, H, n, 1, state) as solo:
        solo.compute_pass()
        solo.sync()
        first = solo.read_rgba8()
    _check(oracle, n, first, state.camera_uniforms(), state.parameter_uniforms(), None, "first frame %s" % kw)
    with _context(oracle, W, H, n, 2, state) as ctx:
        buf = _buffer(W, H)
        ctx.bind_output(None, buf.data_ptr())
        for _ in range(20):
            ctx.compute_pass()
        ctx.sync()
        ctx.settle()
        for k in range(4):                           # two pairs: slot 0, slot 1, slot 0, slot 1
            buf.fill_(SENTINEL)
            torch.cuda.synchronize()
            ctx.compute_pass()
            ctx.sync()
            assert ctx.frame_device_ptr() == buf.data_ptr(), k
            got = _host(buf, W, H)
            assert np.array_equal(got, first), "%s pass %d (%s): the bound buffer differs from the first frame in %d bytes" % (
                kw, k, "twin" if k & 1 else "context", int((got != first).sum()))
            assert np.array_equal(ctx.read_rgba8(), first), (kw, k)


# ---- 3. moving views that run ahead of the device ------------------------------------------------------------------------

def _turntable_case(oracle, W, H, n, flight, kw, degrees, kernels=None):
    state = _params_state(W, H, **kw)
    views = _turntable(W, H, degrees, _params(**kw))
    with _context(oracle, W, H, n, flight, state) as ctx:
        standing = _buffer(W, H)
        ctx.bind_output(None, standing.data_ptr())
        _standing(ctx, state)
        bufs = _run_ahead(ctx, views, kernels)
        frames = [_host(b, W, H) for b in bufs]
    for k, ((cu, pu), got) in enumerate(zip(views, frames)):
        _check(oracle, n, got, cu, pu, _rows(k, H), "%dx%d flight %d %s: view %d (%.2f degrees on)" % (
            W, H, flight, kw, k, sum(degrees[:k + 1])))


TURNTABLE = [0.25] * 40 + [5.0] * 8          # bench.py's step, then a stretch of large steps: lists dealt on a distant view


@pytest.mark.parametrize("flight", [1, 2])
@pytest.mark.parametrize("kw", [dict(), dict(importance=1)], ids=["base", "importance"])
def test_turntable_small(oracle, volym_lib, flight, kw):
    """The turntable at 640x360 on bonsai 128^3: where a failure of the 1080p case is cheap to track down"""
    _turntable_case(oracle, 640, 360, 128, flight, kw, [0.25] * 12 + [5.0] * 6)


@pytest.mark.parametrize("flight", [1, 2])
@pytest.mark.parametrize("kw", [dict(), dict(importance=1)], ids=["base", "importance"])
def test_turntable_runs_ahead(oracle, volym_lib, flight, kw):
    """bench.py's turntable (moving_view_ms) at 1920x1080 on bonsai 256^3, from a settled standing view, every view checked"""
    _turntable_case(oracle, 1920, 1080, 256, flight, kw, TURNTABLE)


# ---- 4. kernel switches with a second frame slot ------------------------------------------------------------------------

def test_kernel_switches_under_twin(oracle, volym_lib):
    """VOLYM_OPT_KERNEL 2 and 3 alternate between passes of a moving view with two frames in flight; the pattern 2, 3, 3, 2
    gives frames of either frame context either kernel"""
    degrees = [0.5] * 16 + [5.0] * 4
    _turntable_case(oracle, 1920, 1080, 256, 2, dict(), degrees, kernels=[(2, 3, 3, 2)[k % 4] for k in range(len(degrees))])
