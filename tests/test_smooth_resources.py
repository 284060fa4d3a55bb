"""What the compiler made of the smoothing's vote kernel (no GPU: any machine with hipcc).

scene_bytes.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_brush_resources.py compiles it.  Both instantiations of volym_smooth_vote_kernel (9 rows: radius <= 1 across the rows; 49
rows: radius <= 3) must have no scratch, at most 128 VGPRs, and no more LDS than the tile DESIGN.md 4.19 states: the rows of 256
dwords, two columns of votes, the owned dwords as they will be, the label set, the keep masks and their flag, the give and take
tables, and the tally's sizeof(RelabelShared), each of the two rounded up to 16 bytes.  Only the resource remarks are read, never the instructions.  The figures go to
profiles/smooth_kernel_resources.txt.
"""
import os
import subprocess

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_flags, remarks

OUT = os.path.join(ROOT, "profiles", "smooth_kernel_resources.txt")
TALLY = 256 + 2 * 1024 + 4 + 24
ROUND = lambda n: (n + 15) // 16 * 16                                   # the two objects are laid out on 16-byte boundaries
LDS_BAR = {rows: ROUND(rows * 1024 + 2 * 1024 + 1024 + 32 + 256 + 4 + 512) + ROUND(TALLY) for rows in (9, 49)}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("smooth")), "scene_bytes.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "scene_bytes.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return remarks(p.stderr)


def kernels(res):
    """{rows: figures} of the instantiations of the vote kernel (the template argument is mangled as ILj<rows>E)"""
    out = {}
    for name, r in res.items():
        if "volym_smooth_vote_kernel" in name:
            for rows in LDS_BAR:
                if "ILj%dE" % rows in name:
                    out[rows] = r
    return out


def test_the_unit_includes_the_smoothing_after_the_lasso_and_no_other_unit_does():
    unit = open(os.path.join(CSRC, "scene_bytes.hip")).read()
    assert unit.index('#include "relabel_kernels.h"') < unit.index('#include "lasso_kernels.h"') < unit.index('#include "smooth_kernels.h"') < \
        unit.index('#include "relabel.inc"') < unit.index('#include "lasso.inc"') < unit.index('#include "smooth.inc"')
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and f != "scene_bytes.hip":
            text = open(os.path.join(CSRC, f)).read()
            assert '#include "smooth_kernels.h"' not in text and '#include "smooth.inc"' not in text, f
    assert unit.count("volym_smooth_vote_kernel<") == 0                 # launched from smooth.inc alone
    inc = open(os.path.join(CSRC, "smooth.inc")).read()
    assert inc.count("volym_smooth_vote_kernel<") == 2 and "volym_label_swap_kernel" in inc


def test_both_instantiations_have_no_scratch_128_vgprs_and_the_lds_of_the_tile(scene_unit):
    found = kernels(scene_unit)
    assert set(found) == set(LDS_BAR), [n for n in scene_unit if "smooth" in n]
    assert sum("volym_smooth_vote_kernel" in n for n in scene_unit) == 2, "the instantiations stay few"
    lines = ["volym_smooth_vote_kernel<9> and <49> (scene_bytes.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_smooth_resources.py; bar for both: scratch 0, VGPRs <= 128, LDS <= %d and %d" % (LDS_BAR[9], LDS_BAR[49]), ""]
    for rows, r in sorted(found.items()):
        lines.append("%-26s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % ("smooth_vote_kernel<%d>" % rows, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    print("\n".join(lines))
    try:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                  # a read-only checkout still checks the bar
    for rows, r in found.items():
        assert r["scratch"] == 0, (rows, r)
        assert r["vgpr"] <= 128, (rows, r)
        assert r["lds"] <= LDS_BAR[rows], (rows, r)
