"""What the compiler made of the measure kernel (no GPU: any machine with hipcc).

measure.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_project_resources.py compiles project.hip.  Both instantiations of volym_measure_kernel<LABELS> must have no scratch, at
most 128 VGPRs and at most 64 KB of LDS (two workgroups fit the 160 KB of a CU).  The figures go to
profiles/measure_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, scene_bytes_holds_no_part_of, write_figures

OUT = os.path.join(ROOT, "profiles", "measure_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit():
    return compile_unit("measure")


def instantiations(res):
    """{labels: figures} of the volym_measure_kernel<LABELS> instantiations"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_measure_kernelILb([01])E", name)
        if m:
            out[m.group(1) == "1"] = r
    return out


def test_the_makefile_lists_the_new_header_among_the_units_dependencies():
    assert makefile_builds("measure")
    text = open(os.path.join(CSRC, "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*:=\s*\$\(wildcard (.*)\)$", text, re.M).group(1).split()
    assert "$(HERE)*.h" in hdrs and "$(HERE)*.hpp" in hdrs            # measure_kernels.h, scene_chunks.h and scene_bytes.hpp
    assert only_unit_including("measure_kernels.h", "measure.hip")
    assert scene_bytes_holds_no_part_of("measure_kernels.h")


def test_both_instantiations_have_no_scratch_128_vgprs_and_64_kb_of_lds(scene_unit):
    inst = instantiations(scene_unit)
    assert set(inst) == {False, True}, list(scene_unit)
    lines = ["volym_measure_kernel<LABELS> (measure.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_measure_resources.py; bar for both: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for labels, r in sorted(inst.items()):
        lines.append("measure_kernel<%-5s>  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (
            str(labels).lower(), r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for labels, r in inst.items():
        assert r["scratch"] == 0, (labels, r)
        assert r["vgpr"] <= 128, (labels, r)
        assert r["lds"] <= 65536, (labels, r)
