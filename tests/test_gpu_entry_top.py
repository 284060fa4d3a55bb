"""The words a wave starts a work-list entry with -- the entry itself and the tile-mask bits of its tile -- come through LDS and the
scalar cache (raymarch_pq.h, the top of the ticket loop).  What can go wrong there is an address: the wrong word of the mask, the
wrong bit of it, the wrong place of the list.  So the frames are small and their sizes are chosen for the addresses:

  16 x 16     a single 16x16 tile: one mask word, bits 0, 1 and the row behind them;
  200 x 120   25 8x8 tiles per row (a mask row is 26 bits: twice the 13 16x16 tiles): rows start at every even bit of a word, and a
              16x16 tile's two rows lie in different words or at different places of one;
  203 x 77    ragged in both directions;
  264 x 136   33 8x8 tiles per row (a mask row is 34 bits): every row crosses a word boundary.

The first frame of a view has no mask and runs the centre-first list; the frames after it (each adopted with settle()) have the
mask, the depth bounds and a dealt list with super and quarter entries.  They must be bit-equal to the first frame in f32 and
rgba8, with one frame slot and with two (both slots are read), and the first frame lies within the oracle's tolerance.  The
oracle's frame also says that the view exercises the constant-tile paths: it must hold 8x8 tiles that are wholly (0, 0, 0, 1)
(outside the cube) and wholly (0, 0, 0, 0) (inside the cube, nothing dense), and -- from 200 x 120 on -- 16x16 tiles of both kinds
(203 x 77 off axis has the empty ones as 8x8 tiles only).

One large frame takes the other branch of the entry fetch: a workgroup stages PQ_ITEMS_LDS = 512 entries in LDS and reads the rest
of its part of the list from global memory.  4096 x 2176 is 139264 8x8 entries on the first frame, more than 512 for each of the
256 workgroups of an MI355X, and the dealt lists of the later frames (a super entry per constant 16x16 tile) are shorter: the frames
that read the list from global memory are compared with frames that do not.
"""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

TOL = 1e-4
PQ_ITEMS_LDS = 512
POSES = {"headline": (0.0, 0.0, 0.0), "off_axis": (35.0, -25.0, -0.5)}
SIZES = [(16, 16), (200, 120), (203, 77), (264, 136)]

_refs = {}


def _uniforms(oracle, W, H, pose):
    from volym_amd import _lib
    cam = oracle.benchmark_camera_uniforms(W / H, *pose)
    par = oracle.make_parameters()
    return cam, par, _lib.CameraUniforms.from_buffer_copy(bytes(cam)), _lib.ParameterUniforms.from_buffer_copy(bytes(par))


def _reference(oracle, W, H, pose, rows=None):
    """the oracle's frame of bonsai(64), rendered once per (size, pose) and shared by the one-slot and the two-slot case"""
    key = (W, H, pose, None if rows is None else tuple(rows))
    if key not in _refs:
        raw, _ = common.bonsai(64)
        cam, par, _, _ = _uniforms(oracle, W, H, pose)
        vol = oracle.prepare_volume(raw, (64, 64, 64), True)
        f32, u8, _ = oracle.render(vol, np.zeros(64 ** 3, np.uint8), (64, 64, 64), oracle.tf_default_lut(), cam, par, W, H, rowlist=rows)
        f32.setflags(write=False)
        u8.setflags(write=False)
        _refs[key] = (f32, u8)
    return _refs[key]


def constant_tiles(f32, size):
    """(tiles wholly (0, 0, 0, 1), tiles wholly (0, 0, 0, 0)) among the size x size tiles of a frame (ragged tiles by their pixels inside)"""
    H, W = f32.shape[:2]
    miss = empty = 0
    for y in range(0, H, size):
        for x in range(0, W, size):
            t = f32[y:y + size, x:x + size].reshape(-1, 4)
            if not t[:, :3].any():
                miss += int((t[:, 3] == 1.0).all())
                empty += int((t[:, 3] == 0.0).all())
    return miss, empty


def _frames(W, H, cu, pu, slots, n):
    """n frames of one standing view of bonsai(64): the first as it comes, every later one after the re-deal in flight was adopted"""
    from volym_amd import _lib, demo, scene
    raw, _ = common.bonsai(64)
    out = []
    with demo.GpuContext(W, H, 0) as ctx:
        ctx.set_option(_lib.OPT_WRITE_F32, 1)
        if slots == 2:
            ctx.set_option(_lib.OPT_FRAMES_IN_FLIGHT, 2)
        ctx.set_volume(scene.prepare_volume(raw, (64, 64, 64), True), (64, 64, 64), 0)
        ctx.set_importances(np.zeros(64 ** 3, np.uint8), (64, 64, 64))
        ctx.set_transfer_function(scene.default_lut())
        ctx.update(cu, pu)
        for k in range(n):
            if k:
                ctx.settle()
            ctx.compute_pass()
            ctx.sync()
            out.append((ctx.read_rgba32f(), ctx.read_rgba8()))
    return out


def _check(oracle, W, H, pose, slots, n, rows=None):
    _, _, cu, pu = _uniforms(oracle, W, H, pose)
    frames = _frames(W, H, cu, pu, slots, n)
    f32_1, u8_1 = frames[0]
    for i, (f32, u8) in enumerate(frames[1:], start=2):
        assert np.array_equal(f32.view(np.uint32), f32_1.view(np.uint32)), "%dx%d pose %s, %d slot(s): f32 frame %d differs from frame 1" % (W, H, pose, slots, i)
        assert np.array_equal(u8, u8_1), "%dx%d pose %s, %d slot(s): rgba8 frame %d differs from frame 1" % (W, H, pose, slots, i)
    ref_f32, ref_u8 = _reference(oracle, W, H, pose, rows)
    sel = slice(None) if rows is None else rows
    err, over, du8, _ = common.compare_images(f32_1[sel], u8_1[sel], ref_f32[sel], ref_u8[sel], TOL)
    print("%dx%d pose %s, %d slot(s): max |f32 - oracle| %.3g, rgba8 %d" % (W, H, pose, slots, err, du8))
    assert over == 0 and du8 <= 1, "%dx%d pose %s: max |f32 - oracle| %.3g (%d pixels over), rgba8 %d" % (W, H, pose, err, over, du8)
    return ref_f32


@pytest.mark.parametrize("slots", [1, 2], ids=["one_slot", "two_slots"])
@pytest.mark.parametrize("pose", list(POSES.values()), ids=list(POSES))
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_frames_with_mask_and_dealt_list_equal_the_first(oracle, volym_lib, size, pose, slots):
    W, H = size
    # one slot: frames 2.. have the mask; two slots: frames alternate, each slot builds its mask on its second frame, so frames 5-8
    # come from slots with a mask and an adopted list, of both slots
    ref_f32 = _check(oracle, W, H, pose, slots, 4 if slots == 1 else 8)
    miss8, empty8 = constant_tiles(ref_f32, 8)
    miss16, empty16 = constant_tiles(ref_f32, 16)
    print("%dx%d pose %s: constant 8x8 tiles outside the cube %d, inside %d; 16x16 tiles %d, %d" % (W, H, pose, miss8, empty8, miss16, empty16))
    if (W, H) != (16, 16):              # (a single tile, marched in both poses)
        assert miss8 and empty8 and miss16, (miss8, empty8, miss16)
        # 203 x 77 off axis: 18 empty 8x8 tiles inside the cube and no whole 16x16 tile of them; every other view has both
        assert empty16 or (size, pose) == ((203, 77), POSES["off_axis"]), empty16


def test_list_entries_beyond_the_staged_part(oracle, volym_lib):
    import torch
    W, H = 4096, 2176
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (W // 8) * (H // 8) > PQ_ITEMS_LDS * cus, "the first frame's list fits the staged part on this device: no entry is read from global memory"
    # rows of the oracle: the frame's edges (the end of the centre-first list: the entries read from global memory), the middle,
    # and a few between
    rows = sorted(set([0, 1, 7, 8, H - 9, H - 8, H - 2, H - 1] + list(range(5, H, 181))))
    _check(oracle, W, H, POSES["off_axis"], 1, 3, rows=rows)
