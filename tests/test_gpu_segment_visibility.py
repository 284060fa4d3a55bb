"""Segment visibility on the device (volym_set_segment_visibility).  A frame with mask `visible` and crop box B is the frame of
the scene whose density AND importance bytes are 0 in every texel of a hidden label and outside B: the expected pictures come
from oracle.render on scene.hide_segments / scene.crop_volume-zeroed inputs (<= 1e-4 on f32, <= 1 rgba8 LSB), and a twin
context that receives the zeroed bytes through set_volume / set_importances must give bit-equal rgba8 and f32.  After every
edit three frames of the standing view are read and must be bit-equal to each other.  (Criteria, scenes and parameter sets:
tests/test_gpu_crop_box.py.)"""
import json
import os

import numpy as np
import pytest

from tests import common
from tests.test_gpu_crop_box import (CANOPY, H, PARAMS, POT, W, _bonsai, _changed, _ctx, _frame, _near, _oracle, _ragged, _same, _table,
                                     _three, _uniforms)

pytestmark = pytest.mark.gpu

POSE = (35.0, 20.0, 0.0)
ALL = ()
_refs = {}                 # oracle frames, shared by the layouts of a test


def _mask(hidden):
    from volym_amd import scene
    return scene.visibility_mask(hidden)


def _hide(vol, imp, labels, hidden):
    from volym_amd import scene
    return scene.hide_segments(vol, labels, _mask(hidden)), scene.hide_segments(imp, labels, _mask(hidden))


def _ref(oracle, key, vol, imp, dims, cam, par, **kw):
    if key not in _refs:
        _refs[key] = _oracle(oracle, vol, imp, dims, cam, par, **kw)
    return _refs[key]


def _scene(volume):
    if volume == "bonsai64":
        dims, vol, labels = _bonsai()
        # (canopy 2, trunk 3, pot 4; label 200 has no voxels)
        masks = [("hide the canopy", (2,), 0.01), ("hide the pot as well", (2, 4), 0.01), ("show the canopy", (4,), 0.01),
                 ("hide label 0 only", (0,), 0.0), ("toggle a label without voxels", (0, 200), None), ("hide everything", tuple(range(256)), 0.0),
                 ("all visible", ALL, 0.0)]
        return dims, vol, labels, CANOPY, masks
    dims, vol, labels = _ragged()
    # (shell 1, core 2, blob 5; label 77 has no voxels)
    masks = [("hide the shell", (1,), 0.01), ("hide the blob as well", (1, 5), 0.01), ("show the shell", (5,), 0.01),
             ("hide label 0 only", (0,), 0.0), ("toggle a label without voxels", (0, 77), None), ("hide everything", tuple(range(256)), 0.0),
             ("all visible", ALL, 0.0)]
    return dims, vol, labels, _table(l2=255), masks


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("volume", ["bonsai64", "ragged"])
def test_edit_sequence(oracle, volym_lib, volume, layout):
    """Mask after mask on one context against a twin that is handed the host-zeroed bytes, and against the oracle.  bonsai: the
    importances come from labels on the device through a table (the labels are their own source); ragged: uploaded importances,
    then set_labels without a table (the device copy of the importances is their source).  The first two masks run in all six
    parameter sets, the others in two.  The named hiding edits must change at least 1 % of the pixels of the frame before them
    (oracle, 96 x 64, this pose: bonsai canopy 3.8 %, pot 2.3 %; ragged shell 12.5 %, blob 1.4 %)."""
    from volym_amd import scene
    dims, vol, labels, table, masks = _scene(volume)
    imp = table[labels]
    lut = scene.default_lut()
    modes = {k: _uniforms(oracle, W, H, POSE, **PARAMS[k]) for k in PARAMS}
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        if volume == "bonsai64":
            dev.set_labels(labels, dims)
            dev.set_segment_importances(table)
        else:
            dev.set_importances(imp, dims)
            dev.set_labels(labels, dims)
        twin.set_transfer_function(lut)
        assert dev.segment_visibility().all()
        before = {k: _three(dev, (k, "all visible"), cu, pu) for k, (cam, par, cu, pu) in modes.items() if k in ("base", "cone")}
        last_ref = _ref(oracle, (volume, ALL, "base"), vol, imp, dims, *modes["base"][:2])
        _near((volume, layout, "all visible"), before["base"], last_ref)
        for step, (name, hidden, least) in enumerate(masks):
            hvol, himp = _hide(vol, imp, labels, hidden)
            twin.set_volume(hvol, dims, 0)
            twin.set_importances(himp, dims)
            for k in (PARAMS if step < 2 else ("base", "cone")):
                cam, par, cu, pu = modes[k]
                what = (volume, layout, name, k)
                if k == "base":
                    dev.update(cu, pu)                      # the view of this mode, then the edit with NO update after it
                    _frame(dev)
                    dev.set_segment_visibility(_mask(hidden))
                    assert np.array_equal(dev.segment_visibility(), _mask(hidden))
                    got = _three(dev, what)
                else:
                    got = _three(dev, what, cu, pu)
                _same(what + ("twin",), got, _frame(twin, cu, pu))
                ref = _ref(oracle, (volume, tuple(sorted(set(hidden) & set(np.unique(labels).tolist()))), k), hvol, himp, dims, cam, par)
                _near(what, got, ref)
                if k == "base":
                    frac = _changed(ref[1], last_ref[1])
                    print("%s, %s: %.1f %% of the pixels change" % (volume, name, 100.0 * frac))
                    if least is None:
                        assert frac == 0.0, what
                    else:
                        assert frac >= least, (what, frac)
                    last_ref = ref
                if hidden == ALL:
                    _same(what + ("equals the frame before the first edit",), got, before[k])
        assert int(dev.label_counts().sum()) == dims[0] * dims[1] * dims[2]          # the whole label volume, whatever the mask


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("source", ["labels", "uploaded"])
def test_crop_and_mask_interleaved(oracle, volym_lib, source, layout):
    """Any interleaving of crop edits and mask edits that ends at the same (box, mask) gives the same bytes; the twin receives
    crop_volume(hide_segments(...))."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    lut = scene.default_lut()
    full = ((0, 0, 0), dims)
    box, wide = ((5, 7, 9), (50, 61, 43)), ((2, 3, 4), (62, 63, 60))
    steps = [
        ("hide", "mask", (2,)), ("then crop", "box", box),                                   # hide, then crop
        ("full again", "box", full), ("all visible again", "mask", ALL),
        ("crop", "box", box), ("then hide", "mask", (2,)),                                   # crop, then hide: the same state
        ("grow the box over hidden texels", "box", wide),
        ("hide the pot too while cropped", "mask", (2, 4)),
        ("show the canopy while cropped", "mask", (4,)),
        ("an empty box", "box", ((10, 0, 0), (10, 64, 64))),
        ("hide while the box is empty", "mask", (3, 4)),
        ("the box back", "box", box),
        ("back to full", "box", full), ("and all visible", "mask", ALL),
    ]
    modes = {k: _uniforms(oracle, W, H, POSE, **PARAMS[k]) for k in ("base", "straight")}
    seen = {}
    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        if source == "labels":
            dev.set_labels(labels, dims)
            dev.set_segment_importances(CANOPY)
        else:
            dev.set_importances(imp, dims)
            dev.set_labels(labels, dims)
        twin.set_transfer_function(lut)
        before = {k: _three(dev, (k, "before"), cu, pu) for k, (cam, par, cu, pu) in modes.items()}
        cur_box, cur_hidden = full, ALL
        for name, kind, value in steps:
            if kind == "box":
                cur_box = value
                dev.set_crop_box(*value)
            else:
                cur_hidden = value
                dev.set_segment_visibility(_mask(value))
            assert dev.crop_box() == cur_box and np.array_equal(dev.segment_visibility(), _mask(cur_hidden))
            hvol, himp = _hide(vol, imp, labels, cur_hidden)
            cvol, cimp = scene.crop_volume(hvol, dims, *cur_box), scene.crop_volume(himp, dims, *cur_box)
            twin.set_volume(cvol, dims, 0)
            twin.set_importances(cimp, dims)
            for k, (cam, par, cu, pu) in modes.items():
                what = (source, layout, name, k)
                got = _three(dev, what, cu, pu)
                _same(what + ("twin",), got, _frame(twin, cu, pu))
                _near(what, got, _ref(oracle, ("interleaved", cur_box, cur_hidden, k), cvol, cimp, dims, cam, par))
                state = (cur_box, cur_hidden, k)
                if state in seen:
                    _same(what + ("the same state reached another way",), got, seen[state])
                seen[state] = got
                if cur_box == full and cur_hidden == ALL:
                    _same(what + ("equals the frame before",), got, before[k])
        assert _changed(seen[(box, (2,), "base")][1], before["base"][1]) > 0.01


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_lifetime(oracle, volym_lib, layout):
    """The mask belongs to the labels: new importances from a table are hidden too; volym_set_labels, volym_set_importances and
    volym_set_volume each reset the mask and give the bytes back.  Every state against a twin."""
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    cam, par, cu, pu = _uniforms(oracle, W, H, (0.0, -80.0, 0.0), **PARAMS["straight"])     # the pot in front: its importance matters
    ones = np.ones(256, np.uint8)

    def twin_frame(tvol, timp):
        with _ctx(layout) as twin:
            twin.set_volume(tvol, dims, 0)
            twin.set_importances(timp, dims)
            twin.set_transfer_function(lut)
            return _frame(twin, cu, pu)

    with _ctx(layout) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        dev.set_labels(labels, dims)
        dev.set_segment_importances(CANOPY)
        # a table set while a segment is hidden: importances with that segment hidden
        dev.set_segment_visibility(_mask((4,)))
        dev.set_segment_importances(POT)
        assert np.array_equal(dev.segment_visibility(), _mask((4,)))
        hvol, himp = _hide(vol, POT[labels], labels, (4,))
        assert not himp.any()
        got = _three(dev, "table while hidden", cu, pu)
        _same("table while hidden", got, twin_frame(hvol, himp))
        _near("table while hidden", got, _oracle(oracle, hvol, himp, dims, cam, par))
        pot_shown = twin_frame(vol, POT[labels])
        assert _changed(pot_shown[1], twin_frame(hvol, POT[labels])[1]) > 0.0, "the pot's importances must matter in this view"
        both = _table(l2=255, l4=255)
        dev.set_segment_importances(both)                              # canopy and pot important, the pot still hidden
        _same("second table while hidden", _three(dev, "second table while hidden"), twin_frame(*_hide(vol, both[labels], labels, (4,))))
        dev.set_segment_visibility(ones)                               # showing it brings the NEW table's bytes
        _same("shown after the table edit", _three(dev, "shown after the table edit"), twin_frame(vol, both[labels]))
        # volym_set_labels resets the mask; density and importances get their bytes back
        dev.set_segment_importances(POT)
        dev.set_segment_visibility(_mask((2, 4)))
        dev.set_labels(labels, dims)
        assert dev.segment_visibility().all()
        _same("set_labels resets the mask", _three(dev, "set_labels resets the mask"), pot_shown)
        # ... and the labels it brings are the ones the next mask reads (the importances are a plain volume now)
        relabelled = np.where(labels == 4, 9, labels).astype(np.uint8)
        dev.set_labels(relabelled, dims)
        dev.set_segment_visibility(_mask((4,)))                        # no voxel carries 4 any more
        _same("label 4 is unused now", _three(dev, "label 4 is unused now"), pot_shown)
        dev.set_segment_visibility(_mask((9,)))
        _same("label 9 is the pot now", _three(dev, "label 9 is the pot now"), twin_frame(*_hide(vol, POT[labels], labels, (4,))))
        # volym_set_importances drops the labels and the mask
        imp2 = CANOPY[labels]
        dev.set_importances(imp2, dims)
        assert dev.segment_visibility().all()
        _same("set_importances resets the mask", _three(dev, "set_importances resets the mask"), twin_frame(vol, imp2))
        with pytest.raises(_lib.VolymError) as e:
            dev.set_segment_visibility(_mask((2,)))                    # no labels any more
        assert e.value.code == _lib.E_STATE
        # volym_set_volume resets the mask; the importances get their bytes back
        dev.set_labels(labels, dims)
        dev.set_segment_visibility(_mask((2, 3)))
        _same("hidden with uploaded importances", _three(dev, "hidden with uploaded importances"), twin_frame(*_hide(vol, imp2, labels, (2, 3))))
        dev.set_volume(vol, dims, 0)
        assert dev.segment_visibility().all()
        _same("set_volume resets the mask", _three(dev, "set_volume resets the mask", cu, pu), twin_frame(vol, imp2))
        dev.set_segment_visibility(_mask((4,)))                        # the labels are still there
        _same("hide after set_volume", _three(dev, "hide after set_volume"), twin_frame(*_hide(vol, imp2, labels, (4,))))


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
@pytest.mark.parametrize("source", ["labels", "uploaded"])
@pytest.mark.parametrize("call", ["set_volume", "set_labels", "set_importances", "set_segment_importances"])
def test_lifetime_cropped_and_masked(oracle, volym_lib, call, source, layout):
    """The set-up calls on a context that has BOTH a crop box and a mask.  volym_set_volume resets both and gives the importances
    all their bytes back; volym_set_labels and volym_set_importances reset the mask and keep the box; volym_set_segment_importances
    keeps both.  Every state bit-equal to a twin that is handed the host-zeroed bytes, and near the oracle."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    lut = scene.default_lut()
    cam, par, cu, pu = _uniforms(oracle, W, H, (0.0, -80.0, 0.0), **PARAMS["straight"])     # the pot in front: its importance matters
    box, hidden, full = ((5, 7, 9), (50, 61, 43)), (2, 4), ((0, 0, 0), dims)
    first, second = _table(l2=255, l3=255), _table(l3=255, l4=255)
    imp = first[labels]

    def crop(a):
        return scene.crop_volume(a, dims, *box)

    with _ctx(layout) as dev, _ctx(layout) as twin:
        dev.set_volume(vol, dims, 0)
        dev.set_transfer_function(lut)
        if source == "labels":
            dev.set_labels(labels, dims)
            dev.set_segment_importances(first)
        else:
            dev.set_importances(imp, dims)
            dev.set_labels(labels, dims)
        twin.set_transfer_function(lut)
        dev.update(cu, pu)
        _frame(dev)
        dev.set_crop_box(*box)
        dev.set_segment_visibility(_mask(hidden))
        hvol, himp = _hide(vol, imp, labels, hidden)
        tvol, timp = crop(hvol), crop(himp)
        twin.set_volume(tvol, dims, 0)
        twin.set_importances(timp, dims)
        what = (call, source, layout, "cropped and masked")
        cut = _three(dev, what)
        _same(what + ("twin",), cut, _frame(twin, cu, pu))
        _near(what, cut, _ref(oracle, ("both", "cut"), tvol, timp, dims, cam, par))
        if call == "set_volume":
            dev.set_volume(vol, dims, 0)
            want_box, want_hidden, tvol, timp = full, ALL, vol, imp
        elif call == "set_labels":
            dev.set_labels(labels, dims)
            want_box, want_hidden, tvol, timp = box, ALL, crop(vol), crop(imp)
        elif call == "set_importances":
            dev.set_importances(POT[labels], dims)
            want_box, want_hidden, tvol, timp = box, ALL, crop(vol), crop(POT[labels])
        else:
            dev.set_segment_importances(second)
            want_box, want_hidden = box, hidden
            tvol, timp = (crop(a) for a in _hide(vol, second[labels], labels, hidden))
        assert dev.crop_box() == want_box and np.array_equal(dev.segment_visibility(), _mask(want_hidden))
        twin.set_volume(tvol, dims, 0)
        twin.set_importances(timp, dims)
        what = (call, source, layout, "after the call")
        got = _three(dev, what, cu, pu)
        _same(what + ("twin",), got, _frame(twin, cu, pu))
        _near(what, got, _ref(oracle, ("both", call), tvol, timp, dims, cam, par))
        if call != "set_segment_importances":               # (density comes back: the canopy and the pot, or all of the volume)
            assert _changed(got[1], cut[1]) > 0.0, what
        if call != "set_importances":
            # the labels are still there, and the context edits on: the pot hidden inside the (kept or new) box
            dev.set_crop_box(*box)
            dev.set_segment_visibility(_mask((4,)))
            src = second[labels] if call == "set_segment_importances" else imp
            tvol, timp = (crop(a) for a in _hide(vol, src, labels, (4,)))
            twin.set_volume(tvol, dims, 0)
            twin.set_importances(timp, dims)
            what = (call, source, layout, "edited on")
            _same(what + ("twin",), _three(dev, what), _frame(twin, cu, pu))


@pytest.mark.parametrize("slots", [1, 2], ids=["one slot", "two in flight"])
def test_edit_between_enqueued_passes(oracle, volym_lib, slots):
    """A pass enqueued before the edit shows the old mask, the two enqueued after it the new one, with no volym_update and no
    sync by the caller in between; with VOLYM_OPT_FRAMES_IN_FLIGHT = 2 the later two come from both frame slots."""
    from volym_amd import _lib, scene
    import torch
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    lut = scene.default_lut()
    hides = [ALL, (2,), (2, 4), (3,), ALL]
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE, **PARAMS["straight"])
    refs = [_oracle(oracle, *_hide(vol, imp, labels, h), dims, cam, par) for h in hides]
    assert _changed(refs[1][1], refs[0][1]) > 0.01 and _changed(refs[2][1], refs[1][1]) > 0.01
    bufs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    with _ctx(-1, [(_lib.OPT_FRAMES_IN_FLIGHT, slots)]) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_labels(labels, dims)
        dev.set_segment_importances(CANOPY)
        dev.set_transfer_function(lut)
        dev.update(cu, pu)
        for i in range(1, len(hides)):
            dev.bind_output(None, bufs[0].data_ptr())
            dev.compute_pass()
            dev.set_segment_visibility(_mask(hides[i]))
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


@pytest.mark.parametrize("variant", ["kernel 0", "kernel 1", "kernel 2", "kernel 3", "trilinear"])
def test_kernel_variants_and_filter(oracle, volym_lib, variant):
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    lut = scene.default_lut()
    filt = 1 if variant == "trilinear" else 0
    opts = [] if variant == "trilinear" else [(_lib.OPT_KERNEL, int(variant[-1]))]
    with _ctx(-1, opts) as dev, _ctx(-1, opts) as twin:
        dev.set_volume(vol, dims, filt)
        dev.set_labels(labels, dims)
        dev.set_segment_importances(CANOPY)
        dev.set_transfer_function(lut)
        twin.set_transfer_function(lut)
        for mode in ("base", "straight"):
            cam, par, cu, pu = _uniforms(oracle, W, H, POSE, **PARAMS[mode])
            before = _three(dev, (variant, mode, "before"), cu, pu)
            for hidden in ((2,), (3, 4), ALL):
                hvol, himp = _hide(vol, imp, labels, hidden)
                twin.set_volume(hvol, dims, filt)
                twin.set_importances(himp, dims)
                dev.set_segment_visibility(_mask(hidden))
                got = _three(dev, (variant, mode, hidden))
                _same((variant, mode, hidden, "twin"), got, _frame(twin, cu, pu))
                _near((variant, mode, hidden), got, _ref(oracle, ("variants", filt, mode, hidden), hvol, himp, dims, cam, par, filter=filt))
                if hidden == (2,):
                    assert _changed(got[1], before[1]) > 0.01
            _same((variant, mode, "all visible again"), got, before)


def test_first_hide_of_a_large_volume_and_back(oracle, volym_lib):
    """The first hide makes the uncropped device copy of the density (512^3, in bricks by the size rule: 128 MiB) and at once
    zeroes the largest segment in its source: the copy must be taken before the rewrite.  All visible again restores from the
    copy, so the frame must be bit-equal to the frame before; the hidden frame is checked against the oracle on sampled rows."""
    from volym_amd import scene
    n, w, h = 512, 640, 360
    dims, vol, labels = _bonsai(n)
    rows = list(range(2, h, 12))
    cam, par, cu, pu = _uniforms(oracle, w, h, POSE, **PARAMS["straight"])
    with _ctx(-1, w=w, h=h) as dev:
        dev.set_volume(vol, dims, 0)
        dev.set_labels(labels, dims)
        dev.set_segment_importances(CANOPY)
        dev.set_transfer_function(scene.default_lut())
        before = _three(dev, "before the first hide", cu, pu)
        for hidden in ((2,), (3, 4)):
            dev.set_segment_visibility(_mask(hidden))
            got = _three(dev, ("hidden", hidden))
            hvol, himp = _hide(vol, CANOPY[labels], labels, hidden)
            _near(("hidden", hidden), got, _oracle(oracle, hvol, himp, dims, cam, par, w, h, rowlist=rows), rows)
            assert _changed(got[1], before[1]) > 0.01, "the hidden segment must be in the picture"
            del hvol, himp
            dev.set_segment_visibility(np.ones(256, np.uint8))
            _same((hidden, "all visible again"), _three(dev, "all visible again"), before)
            if hidden == (2,):
                dev.set_volume(vol, dims, 0)                       # the copy is made again by the first hide after volym_set_volume
                dev.update(cu, pu)
    common._cache.pop(("bonsai", n), None)


@pytest.mark.parametrize("layout", [0, 1], ids=["linear", "bricked"])
def test_fetch_counters(oracle, volym_lib, layout):
    """volym_stats_pass under a mask equals the twin's (whose reject box comes from a scan of the zeroed bytes and may be tighter)
    and the oracle's on the zeroed inputs: the reject box changes no counter."""
    from volym_amd import scene
    dims, vol, labels = _bonsai()
    table = _table(l2=255, l4=255)
    imp = table[labels]
    for hidden, pose in (((4,), (0.0, -80.0, 0.0)), ((2,), POSE)):
        hvol, himp = _hide(vol, imp, labels, hidden)
        with _ctx(layout) as dev, _ctx(layout) as twin:
            dev.set_volume(vol, dims, 0)
            dev.set_labels(labels, dims)
            dev.set_segment_importances(table)
            dev.set_transfer_function(scene.default_lut())
            dev.set_segment_visibility(_mask(hidden))
            twin.set_volume(hvol, dims, 0)
            twin.set_importances(himp, dims)
            twin.set_transfer_function(scene.default_lut())
            for name in ("straight", "cone"):
                cam, par, cu, pu = _uniforms(oracle, W, H, pose, **PARAMS[name])
                dev.update(cu, pu)
                twin.update(cu, pu)
                got, want = dev.stats_pass(), twin.stats_pass()
                assert got == want, (hidden, name, got, want)
                ref = _oracle(oracle, hvol, himp, dims, cam, par)[2]
                for k in ("n_vol", "n_imp", "n_steps", "n_dense", "n_hit"):
                    assert got[k] == ref[k], (hidden, name, k, got[k], ref[k])


def test_errors_leave_the_context_rendering(oracle, volym_lib):
    from volym_amd import _lib, scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    cam, par, cu, pu = _uniforms(oracle, W, H, POSE)
    ones = np.ones(256, np.uint8)
    with _ctx(-1) as c:
        def refused(code, mask=ones):
            with pytest.raises(_lib.VolymError) as e:
                c.set_segment_visibility(mask)
            assert e.value.code == code

        refused(_lib.E_STATE)                                          # no volume, no labels
        c.set_volume(vol, dims, 0)
        c.set_importances(imp, dims)
        c.set_transfer_function(scene.default_lut())
        refused(_lib.E_STATE, _mask((2,)))                             # a volume, but no labels
        assert c.segment_visibility().all()
        half = (64, 64, 32)
        c.set_labels(labels[:64 * 64 * 32], half)
        refused(_lib.E_STATE, _mask((2,)))                             # label dimensions are not the volume's
        c.set_labels(labels, dims)
        assert _lib.lib().volym_set_segment_visibility(c.handle, None) == _lib.E_INVALID
        assert _lib.lib().volym_get_segment_visibility(c.handle, None) == _lib.E_INVALID
        with pytest.raises(ValueError):
            c.set_segment_visibility(np.ones(255, np.uint8))
        assert c.segment_visibility().all()
        got = _three(c, "after the refused calls", cu, pu)
        _near("after the refused calls", got, _oracle(oracle, vol, imp, dims, cam, par))
        c.set_segment_visibility(_mask((2,)))
        _near("and a mask that is accepted", _three(c, "accepted"), _oracle(oracle, *_hide(vol, imp, labels, (2,)), dims, cam, par))


@pytest.mark.parametrize("world", [2, 4])
def test_mgpu_virtual_ranks(oracle, volym_lib, world):
    """The native loop with virtual ranks: an edit at a standing view drops the captured graph, so the frame after it is the
    single context's frame of the new mask."""
    from volym_amd import demo, mgpu, scene
    dims, vol, labels = _bonsai()
    imp = CANOPY[labels]
    w, h = 310, 170
    cam, par, cu, pu = _uniforms(oracle, w, h, POSE, **PARAMS["straight"])
    with mgpu.MultiGpu(w, h, devices=[0] * world, transport=mgpu.COPY) as mg, demo.GpuContext(w, h, 0) as single:
        for c in (mg, single):
            c.set_volume(vol, dims, 0)
            c.set_transfer_function(scene.default_lut())
            c.set_labels(labels, dims)
            c.set_segment_importances(CANOPY)
        single.update(cu, pu)

        def check(what, hidden, t):
            assert t["overflowed"] == 0, (world, what, hidden)
            got = mg.read_rgba8()
            single.set_segment_visibility(_mask(hidden))
            single.compute_pass()
            single.sync()
            assert np.array_equal(got, single.read_rgba8()), (world, what, hidden)
            ref = _ref(oracle, ("mgpu", hidden), *_hide(vol, imp, labels, hidden), dims, cam, par, w=w, h=h, want_f32=False)
            du8 = int(np.abs(got.astype(np.int32) - ref[1].astype(np.int32)).max())
            assert du8 <= 1, (world, what, hidden, du8)
            return got

        mg.update(cu, pu)
        mg.prepare(0)
        whole = check("plain enqueues, all visible", ALL, mg.run(3, use_graph=False))
        mg.set_segment_visibility(_mask((2,)))
        hidden = check("plain enqueues", (2,), mg.run(3, use_graph=False))
        assert _changed(hidden, whole) > 0.01
        mg.set_segment_visibility(_mask(ALL))
        # the captured loop at a standing view (tests/test_gpu_crop_box.py says why 16 frames): nothing but the set-up call itself
        # tells the loop that its graph was captured for another scene; segments go, then come back
        t = mg.run(4 * 4, use_graph=True)
        assert t["graph_replays"] >= 1
        check("graph, all visible", ALL, t)
        for hid in ((2,), (2, 4), (3,), ALL):
            mg.set_segment_visibility(_mask(hid))
            t = mg.run(4 * 4, use_graph=True)
            assert t["graph_replays"] >= 1
            check("graph after an edit at a standing view", hid, t)


def test_simple_set_hidden(oracle, volym_lib):
    """demo.Simple.set_hidden: ids of the segments JSON or label values; the labels go to the device on the first call."""
    from volym_amd import demo, scene
    raw, labels_raw = common.bonsai(64)
    dims = (64, 64, 64)
    params = scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)
    state = scene.State.with_parameters(W / H, params)
    state.update()
    vol, imp = common.oracle_scene(oracle, raw, labels_raw, common.BONSAI_SEGMENTS, dims)
    labels = oracle.prepare_volume(labels_raw, dims, True)
    cam = oracle.benchmark_camera_uniforms(W / H)
    par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.01)
    with demo.GpuContext(W, H, 0) as ctx:
        d = demo.Simple.init(ctx, state, volume_raw=raw, labels_raw=labels_raw, segments=common.BONSAI_SEGMENTS, dims=dims)
        assert d.set_hidden(ctx, []) == []
        for hidden, values in ((["canopy"], [2]), ([4, "trunk"], [3, 4]), ([], [])):
            assert d.set_hidden(ctx, hidden) == values
            assert np.array_equal(ctx.segment_visibility(), _mask(values))
            d.compute_pass(ctx)
            ctx.sync()
            ref = _oracle(oracle, *_hide(vol, imp, labels, values), dims, cam, par, want_f32=False)
            assert int(np.abs(ctx.read_rgba8().astype(np.int32) - ref[1].astype(np.int32)).max()) <= 1, hidden
        with pytest.raises(ValueError):
            d.set_hidden(ctx, ["no such segment"])


def test_flythrough_hide_frames_match_oracle(oracle, volym_lib, tmp_path):
    """`python -m volym_amd flythrough --hide 3`: the cup of the teapot scene hidden for the whole flight; every kept frame
    against the oracle on scene.hide_segments inputs, rgba8 within 1 LSB (the tolerance of tests/test_flythrough_crop.py)."""
    from volym_amd import __main__ as cli, image, scene, synth
    out = str(tmp_path)
    assert cli.main(["flythrough", "--width", "192", "--height", "108", "--frames", "48", "--keep-every", "6", "--out", out, "--hide", "3"]) == 0
    meta = json.load(open(os.path.join(out, "frames.json")))
    w, h = meta["width"], meta["height"]
    raw, labels_raw = common.teapot()
    dims = (256, 256, 256)
    vol, imp = common.oracle_scene(oracle, raw, labels_raw, synth.TEAPOT_SEGMENTS, dims)
    labels = oracle.prepare_volume(labels_raw, dims, True)
    visible = scene.visibility_mask([3])
    hvol, himp = scene.hide_segments(vol, labels, visible), scene.hide_segments(imp, labels, visible)
    lut = oracle.tf_default_lut()
    changed = 0
    assert len(meta["frames"]) == 8
    for fr in meta["frames"]:
        assert fr["hidden_labels"] == [3] and tuple(fr["crop_box"][1]) == dims
        cam = oracle.CameraUniforms.from_buffer_copy(bytes.fromhex(fr["camera_uniforms"]))
        par = oracle.Parameters.from_buffer_copy(bytes.fromhex(fr["parameter_uniforms"]))
        _, ref, _ = oracle.render(hvol, himp, dims, lut, cam, par, w, h, want_f32=False)
        got = image.read_png_rgba8(os.path.join(out, fr["png"]))
        d = int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max())
        assert d <= 1, (fr["frame"], fr["event"], d)
        _, full, _ = oracle.render(vol, imp, dims, lut, cam, par, w, h, want_f32=False)
        changed += int((ref != full).any(axis=-1).mean() > 0.01)
    assert changed >= 3, changed
