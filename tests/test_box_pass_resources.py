"""What the compiler made of the kernels the box passes share (no GPU: any machine with hipcc).

box_pass.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_surface_resources.py compiles surface.hip.  The unit holds the three kernels of the offset scan, which the surface and the
components pass both launch, and no other; each must have no scratch, at most 128 VGPRs and at most 64 KB of LDS.  The figures go to
profiles/box_pass_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, write_figures

OUT = os.path.join(ROOT, "profiles", "box_pass_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def box_pass_unit():
    return compile_unit("box_pass")


def test_the_makefile_builds_the_unit_and_only_it_holds_the_scan():
    assert makefile_builds("box_pass")
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")):
            assert bool(re.search(r"__global__[^;{]*_scan_(sums|blocks|rows)_kernel", open(os.path.join(CSRC, f)).read())) == (f == "box_pass.hip"), f


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(box_pass_unit):
    found = {}
    for name, r in box_pass_unit.items():
        m = re.search(r"volym_box_(\w+)_kernel", name)
        found[m.group(1) if m else name] = r
    assert set(found) == {"scan_sums", "scan_blocks", "scan_rows"}, list(box_pass_unit)
    lines = ["the kernels of box_pass.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_box_pass_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("box_pass %-11s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)
