"""What the compiler made of the smoothing's vote kernel (no GPU: any machine with hipcc).

smooth.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_brush_resources.py compiles its unit.  Both instantiations of volym_smooth_vote_kernel (9 rows: radius <= 1 across the rows; 49
rows: radius <= 3) must have no scratch, at most 128 VGPRs, and no more LDS than the tile DESIGN.md 4.19 states: the rows of 256
dwords, two columns of votes, the owned dwords as they will be, the label set, the keep masks and their flag, the give and take
tables, and the tally's sizeof(RelabelShared), each of the two rounded up to 16 bytes.  Only the resource remarks are read, never the instructions.  The figures go to
profiles/smooth_kernel_resources.txt.
"""
import os

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, scene_bytes_holds_no_part_of, write_figures

OUT = os.path.join(ROOT, "profiles", "smooth_kernel_resources.txt")
TALLY = 256 + 2 * 1024 + 4 + 24
ROUND = lambda n: (n + 15) // 16 * 16                                   # the two objects are laid out on 16-byte boundaries
LDS_BAR = {rows: ROUND(rows * 1024 + 2 * 1024 + 1024 + 32 + 256 + 4 + 512) + ROUND(TALLY) for rows in (9, 49)}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit():
    return compile_unit("smooth")


def kernels(res):
    """{rows: figures} of the instantiations of the vote kernel (the template argument is mangled as ILj<rows>E)"""
    out = {}
    for name, r in res.items():
        if "volym_smooth_vote_kernel" in name:
            for rows in LDS_BAR:
                if "ILj%dE" % rows in name:
                    out[rows] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("smooth")
    assert only_unit_including("smooth_kernels.h", "smooth.hip")
    assert scene_bytes_holds_no_part_of("smooth_kernels.h")
    # the launch sites: the vote from smooth.hip alone, the swap through the one function of relabel.hip
    launches = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".inc", ".cpp"))}
    assert {f for f, text in launches.items() if "volym_smooth_vote_kernel<" in text} == {"smooth.hip"}
    assert launches["smooth.hip"].count("volym_smooth_vote_kernel<") == 2 and launches["smooth.hip"].count("launch_label_swap(") == 1
    assert [f for f, text in launches.items() if "hipLaunchKernelGGL(volym_label_swap_kernel" in text] == ["relabel.hip"]
    assert launches["relabel.hip"].count("hipLaunchKernelGGL(volym_label_swap_kernel") == 1


def test_both_instantiations_have_no_scratch_128_vgprs_and_the_lds_of_the_tile(scene_unit):
    found = kernels(scene_unit)
    assert set(found) == set(LDS_BAR), [n for n in scene_unit if "smooth" in n]
    assert sum("volym_smooth_vote_kernel" in n for n in scene_unit) == 2, "the instantiations stay few"
    lines = ["volym_smooth_vote_kernel<9> and <49> (smooth.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_smooth_resources.py; bar for both: scratch 0, VGPRs <= 128, LDS <= %d and %d" % (LDS_BAR[9], LDS_BAR[49]), ""]
    for rows, r in sorted(found.items()):
        lines.append("%-26s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % ("smooth_vote_kernel<%d>" % rows, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for rows, r in found.items():
        assert r["scratch"] == 0, (rows, r)
        assert r["vgpr"] <= 128, (rows, r)
        assert r["lds"] <= LDS_BAR[rows], (rows, r)
