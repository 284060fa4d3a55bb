"""The fly-through's crop widget (ours; the reference's panel has none): a crop face dragged over its range while the camera
orbits and the other widgets change."""
import json
import os

import numpy as np
import pytest

from tests import common


def test_crop_sweep_script():
    """Opt-in and deterministic: `script` keeps its events, the sweep visits both ends of the face's range and moves every frame."""
    from volym_amd import flythrough as ft
    assert all(e[0] != "crop" for e in ft.script(120))
    sw = ft.crop_sweep(60)
    assert sw == ft.crop_sweep(60) and len(sw) == 60
    z = [hi[2] for lo, hi in sw]
    assert max(z) == ft.CROP_FACE_RANGE[1] and min(z) == ft.CROP_FACE_RANGE[0]
    assert all(lo == (0.0, 0.0, 0.0) and hi[:2] == (1.0, 1.0) for lo, hi in sw)
    assert all(a != b for a, b in zip(z[1:-1], z[2:]))


@pytest.mark.gpu
def test_flythrough_crop_sweep_frames_match_oracle(oracle, volym_lib, tmp_path):
    """`python -m volym_amd flythrough --crop-sweep`: an edit of the box before every frame (each edit waits for the frames
    enqueued before it, so nothing is in flight across an edit); every kept frame against the oracle on the inputs zeroed
    outside the box the frame was rendered with, rgba8 within 1 LSB."""
    from volym_amd import __main__ as cli, image, scene, synth
    out = str(tmp_path)
    assert cli.main(["flythrough", "--width", "192", "--height", "108", "--frames", "48", "--keep-every", "4", "--out", out, "--crop-sweep"]) == 0
    meta = json.load(open(os.path.join(out, "frames.json")))
    W, H = meta["width"], meta["height"]
    raw, labels = common.teapot()
    dims = (256, 256, 256)
    vol, imp = common.oracle_scene(oracle, raw, labels, synth.TEAPOT_SEGMENTS, dims)
    lut = oracle.tf_default_lut()
    boxes, cut = set(), 0
    for fr in meta["frames"]:
        lo, hi = (tuple(b) for b in fr["crop_box"])
        boxes.add((lo, hi))
        cam = oracle.CameraUniforms.from_buffer_copy(bytes.fromhex(fr["camera_uniforms"]))
        par = oracle.Parameters.from_buffer_copy(bytes.fromhex(fr["parameter_uniforms"]))
        _, ref, _ = oracle.render(scene.crop_volume(vol, dims, lo, hi), scene.crop_volume(imp, dims, lo, hi), dims, lut, cam, par, W, H, want_f32=False)
        got = image.read_png_rgba8(os.path.join(out, fr["png"]))
        d = int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max())
        assert d <= 1, (fr["frame"], fr["event"], lo, hi, d)
        _, full, _ = oracle.render(vol, imp, dims, lut, cam, par, W, H, want_f32=False)
        cut += int((ref != full).any(axis=-1).mean() > 0.01)
    assert len(boxes) >= 8 and cut >= 3, (len(boxes), cut)
