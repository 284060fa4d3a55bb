"""What the compiler made of the outline kernels (no GPU: any machine with hipcc).

outline.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_pick_resources.py compiles the pick unit.  Both kernels -- pack (records -> bit plane) and blend (ring and blend) -- must
have no scratch and at most 64 VGPRs: a byte test, a ballot and four integer blends per lane need far fewer.  Only the resource
remarks are read.  The figures go to profiles/outline_kernel_resources.txt.
"""
import os

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_builds, makefile_flags, remarks, write_figures

OUT = os.path.join(ROOT, "profiles", "outline_kernel_resources.txt")
KERNELS = ("volym_outline_pack_kernel", "volym_outline_blend_kernel")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def outline_unit(tmp_path_factory):
    import subprocess
    out = os.path.join(str(tmp_path_factory.mktemp("outline")), "outline.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "outline.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return remarks(p.stderr)


def test_the_makefile_builds_and_links_the_unit():
    assert makefile_builds("outline")


def test_both_kernels_have_no_scratch_and_at_most_64_vgprs(outline_unit):
    res = outline_unit
    assert len(res) == 2, list(res)                   # the unit holds its two kernels and nothing else
    by_kernel = {k: next(r for name, r in res.items() if k in name) for k in KERNELS}
    lines = ["kernels of outline.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_outline_resources.py; bar for both: scratch 0, VGPRs <= 64", ""]
    for k, r in by_kernel.items():
        lines.append("%-27s vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (k, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for k, r in by_kernel.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] <= 64, (k, r)


def test_the_unit_holds_no_frame_pick_or_scene_kernel(outline_unit):
    assert not [n for n in outline_unit if "volym_raymarch" in n or "volym_pick" in n or "volym_scene" in n], list(outline_unit)
