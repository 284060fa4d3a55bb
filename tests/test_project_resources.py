"""What the compiler made of the projection kernels (no GPU: any machine with hipcc).

project.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_pick_resources.py compiles pick.hip.  The linear-layout instantiation must have no scratch and at most 128 VGPRs: the bar
of the pick kernel, whose launch shape and ray set-up it shares and which does more per sample (step state, opacity, alpha).  The
figures of both instantiations go to profiles/project_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_builds, makefile_flags, remarks, write_figures

OUT = os.path.join(ROOT, "profiles", "project_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def project_unit(tmp_path_factory):
    import subprocess
    out = os.path.join(str(tmp_path_factory.mktemp("project")), "project.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "project.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return remarks(p.stderr)


def instantiations(res):
    """{bricked: figures} of the volym_project_kernel<BRICK> instantiations"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_project_kernelILb([01])E", name)
        if m:
            out[m.group(1) == "1"] = r
    return out


def test_the_makefile_builds_and_links_the_unit():
    assert makefile_builds("project")


def test_linear_instantiation_has_no_scratch_and_at_most_128_vgprs(project_unit):
    inst = instantiations(project_unit)
    assert set(inst) == {False, True}, list(project_unit)
    lines = ["volym_project_kernel<BRICK> (project.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_project_resources.py; bar: <false> scratch 0, VGPRs <= 128", ""]
    for brick, r in sorted(inst.items()):
        lines.append("project_kernel<%-5s>  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (
            str(brick).lower(), r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    linear = inst[False]
    assert linear["scratch"] == 0, linear
    assert linear["vgpr"] <= 128, linear


def test_the_unit_holds_no_frame_pick_or_slice_kernel(project_unit):
    for other in ("volym_raymarch", "volym_pick", "volym_slice"):
        assert not [n for n in project_unit if other in n], "project.hip must not instantiate a %s kernel" % other
