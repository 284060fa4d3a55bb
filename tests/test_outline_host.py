"""The outline rule on the host (no GPU): scene.outline_frame, the twin the device pass is compared with byte for byte, against a
brute-force double loop and closed forms; the blend formula; and volym_outline at the C boundary.  Every comparison is over every
pixel and exact: the rule is integer.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("volym_outline_pass", "volym_read_outline", "volym_outline_device_ptr")
# volym_outline of include/volym_hip.h: (field, offset, size)
LAYOUT = [("selected", 0, 256), ("ring_rgba", 256, 4), ("fill_rgba", 260, 4), ("radius", 264, 4)]
RING, FILL = (255, 200, 10, 180), (20, 40, 250, 77)


def records(rng, h, w, labels=6):
    from volym_amd import _lib
    p = np.zeros((h, w), _lib.PICK_DTYPE)
    p["status"] = rng.integers(0, 3, (h, w))
    p["label"] = rng.integers(0, labels, (h, w))             # also in records of status 0 and 1: they must not count
    p["t"] = rng.random((h, w))
    p["x"], p["y"], p["z"] = (rng.integers(0, 60000, (h, w)) for _ in range(3))
    p["density"], p["alpha8"] = rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))
    p["has_labels"] = 1
    return p


def blend1(src, col, a):
    return (src * (255 - a) + col * a + 127) // 255


def brute(frame, picks, rect, selected, ring, fill, radius):
    """the rule of the header, pixel by pixel"""
    H, W = frame.shape[:2]
    x0, y0, w, h = rect
    sel = [[False] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            if x0 <= x < x0 + w and y0 <= y < y0 + h:
                r = picks[y - y0, x - x0]
                sel[y][x] = int(r["status"]) == 2 and selected[int(r["label"])] != 0
    out = frame.copy()
    for y in range(H):
        for x in range(W):
            col = None
            if sel[y][x]:
                col = fill
            else:
                for qy in range(max(0, y - radius), min(H, y + radius + 1)):
                    if any(sel[qy][max(0, x - radius):min(W, x + radius + 1)]):
                        col = ring
                        break
            if col is not None:
                a = col[3]
                s = [int(v) for v in frame[y, x]]
                out[y, x] = [blend1(s[0], col[0], a), blend1(s[1], col[1], a), blend1(s[2], col[2], a), blend1(s[3], 255, a)]
    return out


# (7, 3, 20, 11) is the rect of a part of the 40 x 23 image; the 70 x 9 image is only 9 rows high, so there the same rect is cut to the
# frame, (7, 3, 20, 6), and a second one, (50, 1, 20, 7), straddles the 64-pixel word boundary of the device's bit plane
RECTS = {(40, 23): ((0, 0, 40, 23), (7, 3, 20, 11)), (70, 9): ((0, 0, 70, 9), (7, 3, 20, 6), (50, 1, 20, 7))}


@pytest.mark.parametrize("size", [(40, 23), (70, 9)], ids=["40x23", "70x9"])
def test_twin_against_brute_force(size):
    """random records (statuses 0 / 1 / 2, labels 0..5), a random subset selected, radii 1, 2, 8, the whole frame and rects"""
    from volym_amd import scene
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    for rect in RECTS[size]:
        picks = records(rng, rect[3], rect[2])
        for radius in (1, 2, 8):
            selected = np.zeros(256, np.uint8)
            selected[:6] = rng.integers(0, 2, 6)
            if not selected.any():
                selected[3] = 1
            want = brute(frame, picks, rect, selected, RING, FILL, radius)
            got = scene.outline_frame(frame, picks, rect, selected, RING, FILL, radius)
            assert got.dtype == np.uint8 and got.shape == frame.shape
            assert np.array_equal(got, want), (size, rect, radius, np.argwhere((got != want).any(axis=-1))[:4].tolist())
            assert (got != frame).any()


def one_pixel(W, H, x, y, label=3):
    from volym_amd import _lib
    p = np.zeros((H, W), _lib.PICK_DTYPE)
    p[y, x]["status"], p[y, x]["label"] = 2, label
    return p


@pytest.mark.parametrize("radius", [1, 2, 8])
def test_one_selected_pixel_at_a_corner(radius):
    """the clipped (2r + 1)^2 square minus the centre"""
    from volym_amd import scene
    W, H = 40, 23
    frame = np.random.default_rng(1).integers(16, 240, (H, W, 4), dtype=np.uint8)      # no texel equals either colour
    selected = scene.selection_mask([3])
    yy, xx = np.mgrid[0:H, 0:W]
    for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        got = scene.outline_frame(frame, one_pixel(W, H, cx, cy), (0, 0, W, H), selected, (9, 8, 7, 255), (1, 2, 3, 255), radius)
        ring = (got == np.array([9, 8, 7, 255], np.uint8)).all(axis=-1)
        fill = (got == np.array([1, 2, 3, 255], np.uint8)).all(axis=-1)
        square = (np.abs(xx - cx) <= radius) & (np.abs(yy - cy) <= radius)
        centre = (xx == cx) & (yy == cy)
        assert np.array_equal(fill, centre)
        assert np.array_equal(ring, square & ~centre)
        assert int(ring.sum()) == (radius + 1) ** 2 - 1
        assert np.array_equal(got[~square], frame[~square])


def test_identities():
    from volym_amd import scene
    W, H = 40, 23
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    picks = records(rng, H, W)
    whole = (0, 0, W, H)
    some = scene.selection_mask([1, 2, 5])
    # nothing selected: the frame back
    assert np.array_equal(scene.outline_frame(frame, picks, whole, np.zeros(256, np.uint8), RING, FILL, 2), frame)
    # a selected label that no picked record carries: the frame back
    assert np.array_equal(scene.outline_frame(frame, picks, whole, scene.selection_mask([77]), RING, FILL, 8), frame)
    # A = 0 for both colours: the frame back
    assert np.array_equal(scene.outline_frame(frame, picks, whole, some, (255, 0, 0, 0), (0, 255, 0, 0), 2), frame)
    # A = 255: the colours themselves, alpha 255
    got = scene.outline_frame(frame, picks, whole, some, (9, 8, 7, 255), (1, 2, 3, 255), 1)
    sel = (picks["status"] == 2) & np.isin(picks["label"], [1, 2, 5])
    assert sel.any() and (~sel).any()
    assert (got[sel] == [1, 2, 3, 255]).all()
    changed = (got != frame).any(axis=-1) & ~sel
    assert changed.any() and (got[changed] == [9, 8, 7, 255]).all()
    # the input is left alone and the result is a new array
    before = frame.copy()
    out = scene.outline_frame(frame, picks, whole, some, RING, FILL, 2)
    assert out is not frame and np.array_equal(frame, before)


def test_status_1_with_a_selected_label_is_not_selected():
    from volym_amd import _lib, scene
    W, H = 40, 23
    frame = np.random.default_rng(4).integers(0, 256, (H, W, 4), dtype=np.uint8)
    for status in (0, 1):
        p = np.zeros((H, W), _lib.PICK_DTYPE)
        p["status"], p["label"] = status, 3
        assert np.array_equal(scene.outline_frame(frame, p, (0, 0, W, H), scene.selection_mask([3]), RING, FILL, 2), frame), status
    # has_labels == 0: label 0, and selected[0] then selects every picked pixel
    p = np.zeros((H, W), _lib.PICK_DTYPE)
    p["status"][5:9, 4:30] = 2
    got = scene.outline_frame(frame, p, (0, 0, W, H), scene.selection_mask([0]), (0, 0, 0, 0), (1, 2, 3, 255), 1)
    assert (got[5:9, 4:30] == [1, 2, 3, 255]).all() and np.array_equal(got[9:], frame[9:])
    # a selected pixel outside the rect does not exist: records cover the rect only
    q = np.zeros((4, 5), _lib.PICK_DTYPE)
    q["status"], q["label"] = 2, 3
    got = scene.outline_frame(frame, q, (10, 6, 5, 4), scene.selection_mask([3]), (9, 8, 7, 255), (1, 2, 3, 255), 2)
    assert (got[6:10, 10:15] == [1, 2, 3, 255]).all()
    ringed = np.zeros((H, W), bool)
    ringed[4:12, 8:17] = True
    ringed[6:10, 10:15] = False
    assert (got[ringed] == [9, 8, 7, 255]).all()                     # a ring pixel may lie outside the rect
    outside = np.ones((H, W), bool)
    outside[4:12, 8:17] = False
    assert np.array_equal(got[outside], frame[outside])


def test_blend_formula_against_a_float_reference():
    """all 256 x 256 (src, A) pairs of one colour byte, for several colour bytes: within 1 of round(src + (col - src) * A / 255)"""
    from volym_amd import scene
    src, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for col in (0, 1, 127, 128, 200, 255):
        got = blend1(src, col, a)
        ref = np.round(src + (col - src) * a / 255.0)
        assert np.abs(got - ref).max() <= 1, col
        assert (got[:, 0] == np.arange(256)).all() and (got[:, 255] == col).all()
        # the twin's blend is this formula: r, g, b take col, the alpha byte takes 255
        for A in (0, 1, 77, 254, 255):
            px = np.stack([src[:, 0]] * 4, axis=-1).astype(np.uint8)
            out = scene.outline_blend(px, (col, col, col, A))
            assert (out[:, 0] == blend1(src[:, 0], col, A)).all() and (out[:, 3] == blend1(src[:, 0], 255, A)).all()


def test_twin_refuses_what_the_call_refuses():
    from volym_amd import _lib, scene
    frame = np.zeros((9, 12, 4), np.uint8)
    p = np.zeros((9, 12), _lib.PICK_DTYPE)
    sel = np.zeros(256, np.uint8)
    for radius in (0, 9, -1):
        with pytest.raises(ValueError):
            scene.outline_frame(frame, p, (0, 0, 12, 9), sel, RING, FILL, radius)
    for rect in ((0, 0, 13, 9), (1, 0, 12, 9), (0, 0, 0, 9), (0, 0, 12, 0), (12, 0, 1, 1)):
        with pytest.raises(ValueError):
            scene.outline_frame(frame, p, rect, sel, RING, FILL, 2)
    with pytest.raises(ValueError):
        scene.outline_frame(frame, p[:4], (0, 0, 12, 9), sel, RING, FILL, 2)
    with pytest.raises(ValueError):
        scene.outline_frame(frame, p, (0, 0, 12, 9), sel[:200], RING, FILL, 2)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_library_exports_the_three_calls(volym_lib):
    from volym_amd import _lib
    for name in CALLS:
        assert hasattr(volym_lib, name), name
        assert name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2                  # the calls are additions: the ABI version stays


def test_header_declares_them_and_the_struct():
    text = open(os.path.join(ROOT, "include", "volym_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "sizeof(volym_outline) == 268" in code
    assert re.search(r"#define VOLYM_ABI_VERSION 2\b", code)


def test_struct_is_268_bytes_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Outline) == 268
    for f, off, size in LAYOUT:
        d = getattr(_lib.Outline, f)
        assert (d.offset, d.size) == (off, size), f
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n  printf("%zu", sizeof(volym_outline));\n' +
                   "".join('  printf(" %%zu", offsetof(volym_outline, %s));\n' % f for f, _, _ in LAYOUT) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [268] + [off for _, off, _ in LAYOUT], out


def test_python_faces_exist():
    from volym_amd import demo, scene
    for name in ("outline_pass", "read_outline", "outline_device_ptr"):
        assert callable(getattr(demo.GpuContext, name)), name
    for name in ("highlight", "highlight_at"):
        assert callable(getattr(demo.Simple, name)), name
    assert callable(scene.outline_frame)


def test_null_context_is_refused_without_a_device(volym_lib):
    from volym_amd import _lib
    o = _lib.Outline(radius=2)
    assert volym_lib.volym_outline_pass(None, C.byref(o), None, None, None) == _lib.E_INVALID
    assert volym_lib.volym_read_outline(None, None) == _lib.E_INVALID
    assert volym_lib.volym_outline_device_ptr(None) is None


def test_simple_resolves_names_ids_and_values():
    from volym_amd import demo
    d = demo.Simple((8, 8, 8))
    d._segments = [{"id": "canopy", "name": "Canopy", "label_value": 2, "importance": 255}, {"id": "pot", "name": "Pot", "label_value": 4, "importance": 0}]
    assert d._label_values(["Canopy", "pot", 7, 2]) == [2, 4, 7]
    with pytest.raises(ValueError):
        d._label_values(["nothing of the kind"])
