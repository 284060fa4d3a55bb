"""What the compiler made of the lasso kernels (no GPU: any machine with hipcc).

lasso.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_brush_resources.py compiles its unit.  volym_lasso_kernel, volym_lasso_journal_kernel and volym_lasso_raster_kernel must have no
scratch, at most 128 VGPRs, and no more LDS than the table and the tally need: the view, the rect and the polygon's edges are uniform
and read through the scalar cache, so that is sizeof(RelabelShared) = 256 + 2 * 1024 + 4 + 24 bytes.  Only the resource remarks are
read, never the instructions.  The figures go to profiles/lasso_kernel_resources.txt.
"""
import os

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, scene_bytes_holds_no_part_of, write_figures

OUT = os.path.join(ROOT, "profiles", "lasso_kernel_resources.txt")
LDS_BAR = 256 + 2 * 1024 + 4 + 24

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit():
    return compile_unit("lasso")


def kernels(res):
    """{name: figures} of the raster kernel and of the plain and the journalling edit kernel"""
    out = {}
    for name, r in res.items():
        if "volym_lasso_journal_kernel" in name:
            out["lasso_journal_kernel"] = r
        elif "volym_lasso_raster_kernel" in name:
            out["lasso_raster_kernel"] = r
        elif "volym_lasso_kernel" in name:
            out["lasso_kernel"] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("lasso")
    assert only_unit_including("lasso_kernels.h", "lasso.hip")
    assert scene_bytes_holds_no_part_of("lasso_kernels.h")


def test_the_kernels_have_no_scratch_128_vgprs_and_the_lds_of_table_and_tally(scene_unit):
    found = kernels(scene_unit)
    assert set(found) == {"lasso_kernel", "lasso_journal_kernel", "lasso_raster_kernel"}, list(scene_unit)
    lines = ["volym_lasso_kernel, volym_lasso_journal_kernel and volym_lasso_raster_kernel (lasso.hip), hipcc with the Makefile's flags, "
             "-Rpass-analysis=kernel-resource-usage",
             "written by tests/test_lasso_resources.py; bar for all three: scratch 0, VGPRs <= 128, LDS <= %d" % LDS_BAR, ""]
    for name, r in sorted(found.items()):
        lines.append("%-22s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= LDS_BAR, (name, r)
