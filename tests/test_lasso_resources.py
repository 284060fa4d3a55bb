"""What the compiler made of the lasso kernels (no GPU: any machine with hipcc).

scene_bytes.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_brush_resources.py compiles it.  volym_lasso_kernel, volym_lasso_journal_kernel and volym_lasso_raster_kernel must have no
scratch, at most 128 VGPRs, and no more LDS than the table and the tally need: the view, the rect and the polygon's edges are uniform
and read through the scalar cache, so that is sizeof(RelabelShared) = 256 + 2 * 1024 + 4 + 24 bytes.  Only the resource remarks are
read, never the instructions.  The figures go to profiles/lasso_kernel_resources.txt.
"""
import os
import subprocess

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_flags, remarks

OUT = os.path.join(ROOT, "profiles", "lasso_kernel_resources.txt")
LDS_BAR = 256 + 2 * 1024 + 4 + 24

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("lasso")), "scene_bytes.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "scene_bytes.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return remarks(p.stderr)


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


def test_the_unit_includes_the_lasso_after_the_edit_and_the_brush_and_no_other_unit_does():
    unit = open(os.path.join(CSRC, "scene_bytes.hip")).read()
    assert unit.index('#include "relabel_kernels.h"') < unit.index('#include "brush_kernels.h"') < unit.index('#include "lasso_kernels.h"') < \
        unit.index('#include "relabel.inc"') < unit.index('#include "brush.inc"') < unit.index('#include "lasso.inc"')
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and f != "scene_bytes.hip":
            text = open(os.path.join(CSRC, f)).read()
            assert '#include "lasso_kernels.h"' not in text and '#include "lasso.inc"' not in text, f


def test_the_kernels_have_no_scratch_128_vgprs_and_the_lds_of_table_and_tally(scene_unit):
    found = kernels(scene_unit)
    assert set(found) == {"lasso_kernel", "lasso_journal_kernel", "lasso_raster_kernel"}, list(scene_unit)
    lines = ["volym_lasso_kernel, volym_lasso_journal_kernel and volym_lasso_raster_kernel (scene_bytes.hip), hipcc with the Makefile's flags, "
             "-Rpass-analysis=kernel-resource-usage",
             "written by tests/test_lasso_resources.py; bar for all three: scratch 0, VGPRs <= 128, LDS <= %d" % LDS_BAR, ""]
    for name, r in sorted(found.items()):
        lines.append("%-22s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    print("\n".join(lines))
    try:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                  # a read-only checkout still checks the bar
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= LDS_BAR, (name, r)
