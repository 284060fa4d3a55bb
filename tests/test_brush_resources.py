"""What the compiler made of the brush kernels (no GPU: any machine with hipcc).

brush.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_relabel_resources.py compiles its unit.  volym_brush_kernel and volym_brush_journal_kernel must have no scratch, at most 128
VGPRs, and no more LDS than the table, the tally and the segments need: the segments are read through the scalar cache, so that is
sizeof(RelabelShared) = 256 + 2 * 1024 + 4 + 24 bytes.  Only the resource remarks are read, never the instructions.  The figures go
to profiles/brush_kernel_resources.txt.
"""
import os

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, scene_bytes_holds_no_part_of, write_figures

OUT = os.path.join(ROOT, "profiles", "brush_kernel_resources.txt")
LDS_BAR = 256 + 2 * 1024 + 4 + 24

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit():
    return compile_unit("brush")


def kernels(res):
    """{name: figures} of the plain and the journalling brush kernel"""
    out = {}
    for name, r in res.items():
        if "volym_brush_journal_kernel" in name:
            out["brush_journal_kernel"] = r
        elif "volym_brush_kernel" in name:
            out["brush_kernel"] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("brush")
    assert only_unit_including("brush_kernels.h", "brush.hip")
    assert scene_bytes_holds_no_part_of("brush_kernels.h")


def test_both_kernels_have_no_scratch_128_vgprs_and_the_lds_of_table_and_tally(scene_unit):
    found = kernels(scene_unit)
    assert set(found) == {"brush_kernel", "brush_journal_kernel"}, list(scene_unit)
    lines = ["volym_brush_kernel and volym_brush_journal_kernel (brush.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_brush_resources.py; bar for both: scratch 0, VGPRs <= 128, LDS <= %d" % LDS_BAR, ""]
    for name, r in sorted(found.items()):
        lines.append("%-22s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= LDS_BAR, (name, r)
