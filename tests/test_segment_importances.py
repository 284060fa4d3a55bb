"""Segment importances on the device (volym_set_labels / volym_set_segment_importances): the parts that need no GPU."""
import ctypes as C

import numpy as np


def test_segment_symbols_exported(volym_lib):
    """The built library exports the new entry points, the multi-GPU forwards included."""
    from volym_amd import _lib, mgpu
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("volym_set_labels", "volym_set_segment_importances", "volym_label_counts",
                 "volym_mgpu_set_labels", "volym_mgpu_set_segment_importances"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES or name in mgpu.SIGNATURES, name


def _segments(rng, n, with_zero):
    segs = [{"label_value": int(rng.integers(0, 12)), "importance": int(rng.integers(0, 256))} for _ in range(n)]
    if segs:
        segs += [dict(segs[0], importance=int(rng.integers(0, 256)))]       # a duplicate label: the first one wins
    if with_zero:
        segs.insert(int(rng.integers(0, len(segs) + 1)), {"label_value": 0, "importance": 200})
    return segs


def test_segment_table_matches_oracle_map(oracle):
    from volym_amd import scene
    rng = np.random.default_rng(7)
    labels = rng.integers(0, 14, size=20000).astype(np.uint8)        # labels no segment names map to 0
    for trial in range(24):
        segs = _segments(rng, int(rng.integers(0, 8)), with_zero=trial % 2 == 0)
        table = scene.segment_table(segs)
        assert table.dtype == np.uint8 and table.shape == (256,)
        assert np.array_equal(table[labels], np.asarray(oracle.map_segments(labels, segs))), segs


def _box_scan(imp):
    """important_texel_box as a direct scan: texel AABB (x, y, z) of the bytes >= 128, or None."""
    z, y, x = np.nonzero(imp >= 128)
    if x.size == 0:
        return None
    return (x.min(), y.min(), z.min()), (x.max(), y.max(), z.max())


def _box_union(labels, table):
    """The library's rule: per-label boxes from one pass, then the union over the labels with table[l] >= 128."""
    lo, hi = None, None
    for l in np.unique(labels):
        if table[l] < 128:
            continue
        z, y, x = np.nonzero(labels == l)
        blo, bhi = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
        lo = blo if lo is None else np.minimum(lo, blo)
        hi = bhi if hi is None else np.maximum(hi, bhi)
    return None if lo is None else (tuple(lo), tuple(hi))


def test_box_union_equals_scan():
    rng = np.random.default_rng(11)
    nz, ny, nx = 19, 23, 29
    labels = np.zeros((nz, ny, nx), np.uint8)
    for l in range(1, 9):                                             # blobs of labels in random corners
        z0, y0, x0 = rng.integers(0, nz - 3), rng.integers(0, ny - 3), rng.integers(0, nx - 3)
        labels[z0:z0 + rng.integers(1, 6), y0:y0 + rng.integers(1, 6), x0:x0 + rng.integers(1, 6)] = l
    for _ in range(64):
        table = rng.integers(0, 256, size=256).astype(np.uint8)
        if rng.random() < 0.25:
            table[:] = rng.integers(0, 128)                           # nothing important
        assert _box_union(labels, table) == _box_scan(table[labels])
