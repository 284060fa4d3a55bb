"""volym_cells_meeting_box, the host function that says which cells of a grid of density maxima (the macro cells, and the finer grid
the tile mask and the depth bounds are built from) an edit of a box of texels must refresh, against brute force; and the default
size of the finer grid.  No GPU.

Brute force, from the definition and not from the library's formulas: cell k of N covers the voxels v of an axis of n whose extent
[v / n, (v + 1) / n) meets [k / N, (k + 1) / N) -- what floor(pos * n) can be for a pos in the cell -- and one voxel more on
either side; it meets the box [lo, hi) when one of them is in it.
"""
import ctypes as C

import numpy as np
import pytest

DIMS = list(range(1, 10)) + [37, 50, 64]
GRIDS = [4, 8, 16, 32, 64, 128]


def _cells(L, n_cells, dim, lo, hi):
    c0, c1 = C.c_uint32(77), C.c_uint32(77)
    assert L.volym_cells_meeting_box(n_cells, dim, lo, hi, C.byref(c0), C.byref(c1)) == 0
    return c0.value, c1.value


def _cell_voxels(k, N, n):
    """bool per voxel of the axis: cell k's voxels, slack included"""
    v = np.arange(n, dtype=np.int64)
    own = (v * N < (k + 1) * n) & ((v + 1) * N > k * n)
    out = own.copy()
    out[:-1] |= own[1:]
    out[1:] |= own[:-1]
    return out


def _brute(N, n, lo, hi):
    box = np.zeros(n, bool)
    box[lo:hi] = True
    return [k for k in range(N) if (_cell_voxels(k, N, n) & box).any()]


@pytest.mark.parametrize("N", GRIDS)
def test_cells_meeting_box_against_brute_force(volym_lib, N):
    rng = np.random.default_rng(N)
    for n in DIMS:
        boxes = [(v, v + 1) for v in range(n)]                         # one voxel
        boxes += [(0, n)]                                               # the whole axis
        boxes += [(v, v) for v in (0, n // 2, n)] + [(n, 0)]           # empty
        for _ in range(8):
            a, b = sorted(int(x) for x in rng.integers(0, n + 1, 2))
            boxes.append((a, b))
        for lo, hi in boxes:
            want = _brute(N, n, lo, hi) if lo < hi else []
            c0, c1 = _cells(volym_lib, N, n, lo, hi)
            assert list(range(c0, c1)) == want, (N, n, lo, hi, c0, c1, want)
            assert c1 <= N
            if not want:
                assert (c0, c1) == (0, 0)


def test_every_cell_has_a_voxel(volym_lib):
    """an axis shorter than the grid still gives every cell a voxel: the whole axis meets every cell"""
    for N in GRIDS:
        for n in DIMS:
            assert _cells(volym_lib, N, n, 0, n) == (0, N)
            for k in range(N):
                assert _cell_voxels(k, N, n).any()


def test_invalid(volym_lib):
    c = C.c_uint32()
    assert volym_lib.volym_cells_meeting_box(0, 8, 0, 1, C.byref(c), C.byref(c)) == -1
    assert volym_lib.volym_cells_meeting_box(8, 0, 0, 1, C.byref(c), C.byref(c)) == -1
    assert volym_lib.volym_cells_meeting_box(8, 8, 0, 1, None, C.byref(c)) == -1


@pytest.mark.parametrize("dims, macro, want", [((256, 256, 256), 32, 64), ((1024, 1024, 1024), 32, 64), ((128, 128, 128), 32, 64), ((100, 90, 127), 32, 32), ((256, 256, 256), 64, 64),
                                               ((64, 64, 64), 32, 32), ((37, 50, 29), 32, 32), ((37, 50, 29), 8, 16), ((32, 32, 32), 8, 16),
                                               ((1, 1, 1), 32, 32), ((1, 1, 1), 4, 4), ((5, 3, 2), 4, 4), ((512, 64, 64), 16, 64)])
def test_default_grid(volym_lib, dims, macro, want):
    """a power of two with cells of at least two voxels on the longest axis, at most 64, never fewer than the macro cells"""
    got = volym_lib.volym_bounds_cells_for((C.c_uint32 * 3)(*dims), macro)
    assert got == want
