"""The projection pass without a GPU: the C boundary (struct sizes and offsets, volym_project_check, volym_project_samples) and
the host twin scene.project_frame -- its rays against tests/pick_reference.py, closed forms, the image rules."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("volym_project_pass", "volym_project_image_pass", "volym_read_projection", "volym_read_projection_image", "volym_projection_device_ptr",
         "volym_projection_image_device_ptr", "volym_projection_size", "volym_projection_image_size", "volym_project_at", "volym_project_check", "volym_project_samples")
# struct volym_projection / volym_project of include/volym_hip.h: (field, offset, size)
RECORD = [("t", 0, 4), ("x", 4, 2), ("y", 6, 2), ("z", 8, 2), ("max", 10, 1), ("mean", 11, 1), ("label", 12, 1), ("status", 13, 1), ("n_samples", 14, 2)]
REQUEST = [("step", 0, 4), ("mode", 4, 4), ("flags", 8, 4), ("background", 12, 4), ("palette", 16, 1024)]
F = np.float32
W, H = 96, 64
POSES = [(0.0, 0.0, 0.0), (35.0, 20.0, 0.0)]


def _cam(oracle, pose=POSES[0], w=W, h=H):
    from volym_amd import _lib
    return _lib.CameraUniforms.from_buffer_copy(bytes(oracle.benchmark_camera_uniforms(w / h, *pose)))


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def test_library_header_and_binding_agree(volym_lib):
    from volym_amd import _lib, demo, scene
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "volym_hip.h")).read(), flags=re.S)
    for name in CALLS:
        assert hasattr(volym_lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert volym_lib.volym_abi_version() == 2                  # the calls are additions: the ABI version stays
    assert (_lib.PROJECT_MAX, _lib.PROJECT_MEAN, _lib.PROJECT_TF, _lib.PROJECT_LABELS, _lib.PROJECT_NO_SKIP) == (0, 1, 1, 2, 4)
    for name in ("project_pass", "read_projection", "read_projection_image", "project_at"):
        assert callable(getattr(demo.GpuContext, name)), name
    for name in ("project", "project_at", "brightest_slices_at"):
        assert callable(getattr(demo.Simple, name)), name
    for name in ("Projection", "check_projection", "project_samples", "project_frame"):
        assert hasattr(scene, name), name


def test_struct_sizes_and_offsets_on_both_sides(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Projection) == 16 and C.sizeof(_lib.Project) == 1040
    for cls, layout in ((_lib.Projection, RECORD), (_lib.Project, REQUEST)):
        for f, off, size in layout:
            d = getattr(cls, f)
            assert (d.offset, d.size) == (off, size), f
    dt = _lib.PROJECTION_DTYPE
    assert dt.itemsize == 16 and list(dt.names) == [f for f, _, _ in RECORD]
    for f, off, size in RECORD:
        assert dt.fields[f][1] == off and dt.fields[f][0].itemsize == size, f
    assert dt.fields["t"][0] == np.dtype("<f4")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(struct volym_projection), sizeof(volym_project));\n' +
                   "".join('  printf(" %%zu", offsetof(struct volym_projection, %s));\n' % f for f, _, _ in RECORD) +
                   "".join('  printf(" %%zu", offsetof(volym_project, %s));\n' % f for f, _, _ in REQUEST) +
                   '  printf(" %d %d %d %d %d", VOLYM_PROJECT_MAX, VOLYM_PROJECT_MEAN, VOLYM_PROJECT_TF, VOLYM_PROJECT_LABELS, VOLYM_PROJECT_NO_SKIP);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [16, 1040] + [off for _, off, _ in RECORD] + [off for _, off, _ in REQUEST] + [0, 1, 1, 2, 4], out


CHECK_ROWS = [
    ("ok max", dict(step=0.0025), True),
    ("ok mean tf", dict(step=0.0025, mode=1, flags=1), True),
    ("ok every flag", dict(step=0.01, flags=7), True),
    ("ok no_skip mean", dict(step=0.01, mode=1, flags=5), True),
    ("step at the lower end", dict(step=float(F(1.0e-4))), True),
    ("step at the upper end", dict(step=1.0), True),
    ("step below", dict(step=float(np.nextafter(F(1.0e-4), F(0)))), False),
    ("step above", dict(step=float(np.nextafter(F(1), F(2)))), False),
    ("step 0", dict(step=0.0), False),
    ("step negative", dict(step=-0.01), False),
    ("step nan", dict(step=float("nan")), False),
    ("step inf", dict(step=float("inf")), False),
    ("mode 2", dict(step=0.01, mode=2), False),
    ("flag 8", dict(step=0.01, flags=8), False),
    ("flag high", dict(step=0.01, flags=1 << 31), False),
    ("labels with mean", dict(step=0.01, mode=1, flags=2), False),
    ("labels, tf with mean", dict(step=0.01, mode=1, flags=3), False),
]


@pytest.mark.parametrize("name,kw,ok", CHECK_ROWS, ids=[r[0] for r in CHECK_ROWS])
def test_project_check_rows(volym_lib, name, kw, ok):
    from volym_amd import _lib, scene
    p = scene.Projection(**kw)
    c = p.to_c()
    assert volym_lib.volym_project_check(C.byref(c)) == (_lib.OK if ok else _lib.E_INVALID)
    if ok:
        assert scene.check_projection(p) is p
        back = scene.Projection.from_c(c)
        assert (F(back.step), back.mode, back.flags, back.background) == (F(p.step), p.mode, p.flags, p.background)
    else:
        with pytest.raises(ValueError):
            scene.check_projection(p)


def test_project_check_null_and_round_trip(volym_lib):
    from volym_amd import _lib, scene
    assert volym_lib.volym_project_check(None) == _lib.E_INVALID
    pal = np.random.default_rng(1).integers(0, 256, (256, 4), dtype=np.uint8)
    p = scene.Projection(0.005, _lib.PROJECT_MAX, _lib.PROJECT_LABELS, (1, 2, 3, 4), pal)
    back = scene.Projection.from_c(p.to_c())
    assert back.background == (1, 2, 3, 4) and np.array_equal(back.palette, pal)
    with pytest.raises(TypeError):
        p.replace(nope=1)
    assert p.replace(step=0.5).step == 0.5


def _samples_c(lib, te, tx, st):
    n = C.c_uint32()
    out = np.zeros(len(te), np.int64)
    for i in range(len(te)):
        assert lib.volym_project_samples(float(te[i]), float(tx[i]), float(st[i]), C.byref(n)) == 0, (te[i], tx[i], st[i])
        out[i] = n.value
    return out


def test_project_samples_against_the_loop(volym_lib):
    """12 000 triples: random steps over [1e-4, 1] (log-uniform) with step 1e-4 and step 1 among them, t_entry up to 66, paths up to
    sqrt(3); for a third of them t_exit is placed exactly on a t_k, and one ulp below and above it."""
    from volym_amd import _lib, scene
    rng = np.random.default_rng(11)
    n = 4000
    st = np.exp(rng.uniform(np.log(1.0e-4), 0.0, n)).astype(F).clip(F(1.0e-4), F(1.0))
    st[:200] = F(1.0e-4)
    st[200:400] = F(1.0)
    st[400:600] = F(0.0025)
    te = rng.uniform(0.0, 66.0, n).astype(F)
    te[::7] = F(0.0)
    te[1::7] = F(66.0)
    k = np.minimum(rng.integers(0, 20000, n), np.floor(1.7 / st.astype(np.float64)).astype(np.int64))      # a path of at most ~sqrt(3)
    on = (te + k.astype(F) * st).astype(F)                                    # exactly t_k
    te3 = np.concatenate([te, te, te])
    st3 = np.concatenate([st, st, st])
    third = n // 3
    tx = rng.uniform(0.0, 1.733, n).astype(F) + te
    tx[:third] = on[:third]
    below, above = np.nextafter(tx, F(-np.inf)), np.nextafter(tx, F(np.inf))
    tx3 = np.concatenate([tx, np.where(np.arange(n) < third, below, tx - F(0.5)).astype(F).clip(0, None), np.where(np.arange(n) < third, above, tx + F(0.25)).astype(F)])
    want = scene.project_samples(te3, tx3, st3)
    got = _samples_c(volym_lib, te3, tx3, st3)
    assert got.size >= 10000
    bad = got != want
    assert not bad.any(), (int(bad.sum()), te3[bad][:4], tx3[bad][:4], st3[bad][:4], got[bad][:4], want[bad][:4])
    # on a t_k: exactly k samples (t_k itself does not exist), one ulp above: k + 1 -- unless t_k == t_{k-1} or t_{k+1} in f32, which
    # the loop settles; the loop is the reference, this pins the sense of the comparison where steps are clean
    clean = (np.arange(n) < third) & (st == F(1.0)) & (te == F(0.0))
    assert clean.any() and np.array_equal(want[:n][clean], k[clean]) and np.array_equal(want[2 * n:][clean], k[clean] + 1)
    assert want.max() <= 65535 and (want[tx3 > te3] >= 1).all() and (want[tx3 <= te3] == 0).all()
    # refusals
    m = C.c_uint32()
    assert volym_lib.volym_project_samples(0.0, 1.0, 0.01, None) == _lib.E_INVALID
    for bad_args in ((0.0, 1.0, 0.0), (0.0, 1.0, 2.0), (0.0, 1.0, float("nan")), (-1.0, 1.0, 0.01), (0.0, 129.0, 0.01), (float("nan"), 1.0, 0.01),
                     (0.0, float("inf"), 0.01)):
        assert volym_lib.volym_project_samples(*bad_args, C.byref(m)) == _lib.E_INVALID, bad_args
    assert volym_lib.volym_project_samples(1.0, 1.0, 0.01, C.byref(m)) == 0 and m.value == 0
    assert volym_lib.volym_project_samples(2.0, 1.0, 0.01, C.byref(m)) == 0 and m.value == 0


# ---- the twin's rays --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", POSES, ids=["benchmark", "yawed"])
def test_twin_rays_equal_the_pick_references(oracle, volym_lib, pose):
    from tests import pick_reference as R
    from volym_amd import scene
    cam = oracle.benchmark_camera_uniforms(W / H, *pose)
    par = oracle.make_parameters(density_threshold=0.15, raymarching_step_size=0.05)
    dims = (4, 4, 4)
    zeros = np.zeros(64, np.uint8)
    gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ref = R.march(zeros, zeros, dims, oracle.tf_default_lut(), cam, par, W, H, gx.ravel(), gy.ravel(), 0.0)
    o, d, t_entry, t_exit, hit = scene.project_rays(_cam(oracle, pose), W, H, gx.ravel(), gy.ravel())
    assert hit.sum() > W * H // 3 and not hit.all()
    assert np.array_equal(hit, ref["hit"])
    assert np.array_equal(o.view(np.uint32), ref["eye"].astype(F).view(np.uint32))
    assert np.array_equal(d.view(np.uint32), ref["d"].astype(F).view(np.uint32))
    assert np.array_equal(t_entry.view(np.uint32), ref["t_entry"].view(np.uint32))
    assert (t_exit[hit] > t_entry[hit]).all()


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def test_constant_cube(oracle, volym_lib):
    from volym_amd import scene
    dims = (5, 7, 6)
    cam = _cam(oracle, POSES[1])
    for c in (1, 77, 255):
        rec, img = scene.project_frame(np.full(5 * 7 * 6, c, np.uint8), dims, cam, W, H, scene.Projection(0.01))
        _, _, t_entry, t_exit, hit = scene.project_rays(cam, W, H, *np.meshgrid(np.arange(W), np.arange(H)))
        hit, t_entry = hit.reshape(H, W), t_entry.reshape(H, W)
        assert hit.any() and not hit.all()
        assert (rec["status"][hit] == 2).all() and (rec["status"][~hit] == 0).all()
        assert (rec["max"][hit] == c).all() and (rec["mean"][hit] == c).all()
        assert np.array_equal(rec["t"][hit].view(np.uint32), t_entry[hit].view(np.uint32))          # k* = 0
        assert (rec["n_samples"][hit] >= 1).all() and (rec["n_samples"][~hit] == 0).all()
        assert np.array_equal(rec["n_samples"].ravel(), scene.project_samples(t_entry.ravel(), t_exit, F(0.01)) * hit.ravel())
        assert (rec["t"][~hit] == -1).all() and (rec["max"][~hit] == 0).all() and (rec["mean"][~hit] == 0).all()
        assert (img[hit] == (c, c, c, 255)).all() and (img[~hit] == (0, 0, 0, 255)).all()


def test_one_bright_voxel(oracle, volym_lib):
    from volym_amd import scene
    dims = (9, 8, 10)
    texel = (5, 3, 6)
    vol = np.zeros(dims[::-1], np.uint8)
    vol[texel[2], texel[1], texel[0]] = 200
    lab = np.zeros_like(vol)
    lab[texel[2], texel[1], texel[0]] = 9
    for pose in POSES:
        rec, _ = scene.project_frame(vol.ravel(), dims, _cam(oracle, pose), W, H, scene.Projection(0.002), labels=lab.ravel())
        found = rec["status"] == 2
        assert found.sum() > 10
        assert ((rec["x"][found], rec["y"][found], rec["z"][found]) == np.array(texel)[:, None]).all()
        assert (rec["max"][found] == 200).all() and (rec["label"][found] == 9).all() and (rec["t"][found] > 0).all()
        other = rec["status"] == 1
        assert other.sum() > found.sum()
        for f in ("x", "y", "z", "max", "mean", "label"):
            assert (rec[f][other] == 0).all(), f
        assert (rec["t"][other] == -1).all() and (rec["n_samples"][other] >= 1).all()


def test_smallest_k_wins_a_tie(oracle, volym_lib):
    """two equal plateaus along a ray: t is that of the first sample in the nearer one"""
    from volym_amd import scene
    dims = (8, 8, 8)
    cam = _cam(oracle)
    vol = np.full(512, 50, np.uint8)
    rec, _ = scene.project_frame(vol, dims, cam, W, H, scene.Projection(0.01))
    _, _, t_entry, _, hit = scene.project_rays(cam, W, H, *np.meshgrid(np.arange(W), np.arange(H)))
    hit = hit.reshape(H, W)
    assert np.array_equal(rec["t"][hit], t_entry.reshape(H, W)[hit])
    vol2 = vol.copy().reshape(8, 8, 8)
    vol2[:, :, :] = 50
    vol2[2:6, 2:6, 2:6] = 49                                     # a dimmer core: the maximum is still first met at entry
    rec2, _ = scene.project_frame(vol2.ravel(), dims, cam, W, H, scene.Projection(0.01))
    assert np.array_equal(rec2["t"], rec["t"]) and (rec2["mean"][hit] <= 50).all() and (rec2["mean"][hit] >= 49).all()


# ---- the image --------------------------------------------------------------------------------------------------------------------
def test_image_rules(oracle, volym_lib):
    from volym_amd import _lib, scene
    dims, vol, labels = (32, 32, 32), *[scene.prepare_volume(a, (32, 32, 32), True) for a in common.bonsai(32)]
    cam = _cam(oracle)
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (256, 4), dtype=np.uint8)
    pal[0] = (9, 9, 9, 0)                                        # A = 0 leaves the base
    bg = (10, 20, 30, 40)
    base_p = scene.Projection(0.01, background=bg, palette=pal)
    rec, img = scene.project_frame(vol, dims, cam, W, H, base_p, labels=labels)
    hit, found = rec["status"] > 0, rec["status"] == 2
    assert hit.sum() > W * H // 2 and found.sum() > 0.9 * hit.sum() and (rec["max"] != rec["mean"])[hit].any()
    assert (img[~hit] == bg).all()
    grey = lambda v: np.stack([v, v, v, np.full_like(v, 255)], -1)
    assert np.array_equal(img[hit], grey(rec["max"][hit]))
    rec_m, img_m = scene.project_frame(vol, dims, cam, W, H, base_p.replace(mode=_lib.PROJECT_MEAN), labels=labels)
    assert np.array_equal(rec_m.view(np.uint8), rec.view(np.uint8))                 # a record holds both, whatever the mode
    assert np.array_equal(img_m[hit], grey(rec["mean"][hit])) and (img_m[~hit] == bg).all()
    _, img_n = scene.project_frame(vol, dims, cam, W, H, base_p.replace(flags=_lib.PROJECT_NO_SKIP), labels=labels)
    assert np.array_equal(img_n, img)
    for tf_n in (1, 7, 256):
        lut = rng.integers(0, 256, (tf_n, 4), dtype=np.uint8)
        for mode, v in ((_lib.PROJECT_MAX, rec["max"]), (_lib.PROJECT_MEAN, rec["mean"])):
            _, im = scene.project_frame(vol, dims, cam, W, H, base_p.replace(mode=mode, flags=_lib.PROJECT_TF), lut=lut.ravel(), labels=labels)
            want = lut[(v[hit].astype(np.int64) * tf_n) >> 8].copy()
            want[:, 3] = 255
            assert np.array_equal(im[hit], want) and (im[~hit] == bg).all(), (tf_n, mode)
        _, im = scene.project_frame(vol, dims, cam, W, H, base_p.replace(flags=_lib.PROJECT_TF | _lib.PROJECT_LABELS), lut=lut.ravel(), labels=labels)
        base = lut[(rec["max"].astype(np.int64) * tf_n) >> 8].copy()
        base[..., 3] = 255
        want = base.copy()
        want[found] = scene_blend(base[found], pal[rec["label"][found]])
        assert np.array_equal(im[hit], want[hit])
    _, im = scene.project_frame(vol, dims, cam, W, H, base_p.replace(flags=_lib.PROJECT_LABELS), labels=labels)
    want = grey(rec["max"])
    want[found] = scene_blend(want[found], pal[rec["label"][found]])
    assert np.array_equal(im[hit], want[hit])
    zero_label = found & (rec["label"] == 0)
    if zero_label.any():
        assert np.array_equal(im[zero_label], grey(rec["max"])[zero_label])
    assert (rec["label"][found] != 0).any(), "the overlay must have something to colour"
    with pytest.raises(ValueError):
        scene.project_frame(vol, dims, cam, W, H, base_p.replace(flags=_lib.PROJECT_LABELS))            # no labels
    with pytest.raises(ValueError):
        scene.project_frame(vol, dims, cam, W, H, base_p.replace(flags=_lib.PROJECT_TF))                # no table
    with pytest.raises(ValueError):
        scene.project_frame(vol, dims, cam, W, H, base_p, rect=(90, 0, 10, 4))
    # a rect is the same rays
    r_rec, r_img = scene.project_frame(vol, dims, cam, W, H, base_p, rect=(17, 9, 30, 21), labels=labels)
    assert np.array_equal(r_rec.view(np.uint8), rec[9:30, 17:47].copy().view(np.uint8)) and np.array_equal(r_img, img[9:30, 17:47])


def scene_blend(src, col):
    """the outline's formula with a colour per pixel, written out: (src * (255 - A) + col * A + 127) / 255, alpha from 255"""
    src, col = src.astype(np.int64), col.astype(np.int64)
    a = col[:, 3:4].copy()
    col = col.copy()
    col[:, 3] = 255
    return ((src * (255 - a) + col * a + 127) // 255).astype(np.uint8)


def test_scene_conditions_of_the_gpu_tests(oracle, volym_lib):
    """What tests/test_gpu_project.py relies on, at the benchmark pose: more than half the rays hit, over 98 % of the hit rays have
    max > 0, and over 80 % of them attain their maximum at two or more samples at step 0.0025 (over half at the coarsest step the
    GPU tests use, 0.01, where a texel holds about two samples)."""
    from tests.project_scenes import SCENES, scene_bytes, tie_fraction
    from volym_amd import scene
    for name, (w, h) in SCENES.items():
        dims, vol, labels = scene_bytes(name)
        cam = _cam(oracle, POSES[0], w, h)
        rec, _ = scene.project_frame(vol, dims, cam, w, h, scene.Projection(0.01), labels=labels)
        hit = rec["status"] > 0
        assert hit.sum() > w * h / 2, name
        assert (rec["status"] == 2).sum() > 0.98 * hit.sum(), name
        assert tie_fraction(vol, dims, cam, w, h, 0.01, rec) > 0.5, name
        fine, _ = scene.project_frame(vol, dims, cam, w, h, scene.Projection(0.0025), labels=labels)
        assert tie_fraction(vol, dims, cam, w, h, 0.0025, fine) > 0.8, name


def test_cli_project_argument():
    from volym_amd import __main__ as cli
    assert cli._project_arg("MAX") == ("MAX", None) and cli._project_arg("mean") == ("MEAN", None)
    assert cli._project_arg("max,0.002") == ("MAX", 0.002) and cli._project_arg(" Mean , 1e-3 ") == ("MEAN", 0.001)
    for bad in ("", "MIN", "MAX,", "MAX,x", "MAX,0.1,2"):
        with pytest.raises(SystemExit):
            cli._project_arg(bad)
