"""Shared scene builders for the tests (inputs only; no expected values live here)."""
import itertools

import numpy as np

from volym_amd import synth

BONSAI_SEGMENTS = [
    {"id": "canopy", "name": "Canopy", "index": 0, "label_value": 2, "importance": 255},
    {"id": "trunk", "name": "Trunk", "index": 1, "label_value": 3, "importance": 0},
    {"id": "pot", "name": "Pot", "index": 2, "label_value": 4, "importance": 0},
]

_cache = {}


def bonsai(n):
    """(raw density, raw labels) of synth_bonsai(n)"""
    if ("bonsai", n) not in _cache:
        _cache[("bonsai", n)] = synth.synth_bonsai(n, with_labels=True)
    return _cache[("bonsai", n)]


def teapot():
    if "teapot" not in _cache:
        _cache["teapot"] = synth.synth_teapot()
    return _cache["teapot"]


def oracle_scene(O, raw, labels, segments, dims):
    """Prepared (volume, importances) through the ORACLE's host path."""
    vol = O.prepare_volume(raw, dims, True)
    imp = O.prepare_volume(O.map_segments(labels, segments), dims, True)
    return vol, imp


FLAG_NAMES = ("use_cone_importance_check", "use_importance_coloring", "use_opacity",
              "use_importance_rendering", "use_gaussian_smoothing")


def all_flag_combos():
    for bits in itertools.product((0, 1), repeat=5):
        yield dict(zip(FLAG_NAMES, bits))


def flag_id(f):
    return "".join(str(f[k]) for k in FLAG_NAMES)


def compare_images(got_f32, got_u8, ref_f32, ref_u8, tol=1e-4):
    """-> (max abs float error, #pixels over tol, max rgba8 difference, fraction of bytes differing)"""
    d = np.abs(got_f32.astype(np.float64) - ref_f32.astype(np.float64))
    # NaN-safe: a NaN on either side counts as an error unless both are NaN
    bad = np.isnan(d) & ~(np.isnan(got_f32) & np.isnan(ref_f32))
    d = np.where(np.isnan(d), 0.0, d)
    d[bad] = np.inf
    over = int((d.max(axis=-1) > tol).sum())
    du8 = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    return float(d.max()), over, int(du8.max()), float((du8 > 0).mean())


# ---- the transfer-function and threshold axes (test_oracle_tf_threshold.py, test_gpu_tf_threshold.py) ----------------------

def tf_family(rng):
    """Named RGBA8 transfer-function tables (flat uint8, 4 * n bytes): the default one; random ones of n = 1, 2, 3, 7, 100, 255 and
    256 texels; an opaque, a transparent, a comb (alpha 0 / 255 in turn) and a step table (alpha 0 below texel 96, 255 from
    there on); and one baked from a handful of control points the way a user of scene.TransferFunction gets one."""
    from volym_amd import scene
    out = [("default", scene.default_lut())]
    for n in (1, 2, 3, 7, 100, 255, 256):
        out.append(("random %d" % n, rng.integers(0, 256, 4 * n, dtype=np.uint8)))

    def with_alpha(alpha):
        t = rng.integers(0, 256, (256, 4), dtype=np.uint8)
        t[:, 3] = alpha
        return t.ravel()

    out.append(("opaque", with_alpha(255)))
    out.append(("transparent", with_alpha(0)))
    out.append(("comb", with_alpha(np.where(np.arange(256) % 2 == 0, 0, 255))))
    out.append(("step", with_alpha(np.where(np.arange(256) < 96, 0, 255))))
    tf = scene.TransferFunction()
    for p in ((0.0, 0.1, 0.1, 0.4), (0.25, 0.9, 0.6, 0.1), (0.3, 1.0, 1.0, 1.0), (0.7, 0.2, 0.8, 0.3), (1.0, 1.0, 0.0, 0.0)):
        tf.add_rgb_control_point(*p)
    for p in ((0.0, 0.0), (0.2, 0.0), (0.35, 0.6), (0.5, 0.05), (0.8, 1.0), (1.0, 1.0)):
        tf.add_alpha_control_point(*p)
    out.append(("baked", tf.bake_rgba8()))
    return out


def terraced_volume(dims, levels):
    """Prepared volume bytes (x fastest) of nested box-shaped terraces around the centre: 0 outside, then a plateau of each byte of
    `levels` in turn, the last one in the middle.  Inside a plateau every trilinear or Gaussian sum is a sum of equal values
    under weights that add up to about 1, so an interpolated density lands within an ulp of b/255, on either side."""
    nx, ny, nz = dims
    zz, yy, xx = np.meshgrid(*((np.arange(d) + 0.5) / d for d in (nz, ny, nx)), indexing="ij")
    r = np.maximum(np.maximum(np.abs(xx - 0.5), np.abs(yy - 0.5)), np.abs(zz - 0.5)) / 0.5     # 0 in the centre, 1 on the faces
    values = np.array([0] + list(levels), np.uint8)
    band = np.clip(np.floor((1.0 - r) * 1.15 * len(values)).astype(np.int64), 0, len(values) - 1)
    return values[band].ravel()


def byte_thresholds(bs):
    """float32 thresholds: prev(b/255), b/255 and next(b/255) for every byte b of `bs` (b/255 as float32 division, the value a
    nearest-filter sample of byte b has), then 0, -1, 1, next(1) and 1.5; no value twice."""
    out = []
    for b in bs:
        v = np.float32(b) / np.float32(255)
        out += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    out += [np.float32(0), np.float32(-1), np.float32(1), np.nextafter(np.float32(1), np.float32(2)), np.float32(1.5)]
    seen, uniq = set(), []
    for v in out:
        if float(v) not in seen:
            seen.add(float(v))
            uniq.append(float(np.float32(v)))
    return uniq


# ---- the step-size and look-ahead axes (test_oracle_step_lookahead.py, test_gpu_step_lookahead.py) --------------------------

def _f32_up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def _f32_down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def step_axis():
    """raymarching_step_size from one end of volym_update's range to the other: f32(1e-4) and the float above it, the ends of the
    GUI's slider (0.001, 0.1), 0.25 and 0.5, the float below 1 and 1; every value as the float32 it is stored as."""
    lo = float(np.float32(1e-4))
    return [lo, _f32_up(lo), float(np.float32(0.001)), float(np.float32(0.1)), 0.25, 0.5, _f32_down(1.0), 1.0]


def ahead_axis():
    """importance_check_ahead_steps over volym_update's range: none, the GUI's ends and their neighbours, both sides of a wave of
    64 and of 256, and the top of the range with its neighbour."""
    return [0, 1, 2, 3, 25, 26, 63, 65, 255, 256, 1000, 4095, 4096]


def noise_scene(rng, dims):
    """(volume, importances), prepared bytes: uniform random densities; importance 255 for one voxel in four, 0 for the rest"""
    n = dims[0] * dims[1] * dims[2]
    vol = rng.integers(0, 256, n, dtype=np.uint8)
    imp = np.where(rng.integers(0, 4, n) == 0, 255, 0).astype(np.uint8)
    return vol, imp


def refused_steps():
    """step sizes volym_update refuses: one float outside either end of [f32(1e-4), 1], zero, a negative one, NaN, +inf"""
    return [_f32_down(np.float32(1e-4)), _f32_up(1.0), 0.0, -0.01, float("nan"), float("inf")]
