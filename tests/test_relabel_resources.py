"""What the compiler made of the relabel kernel (no GPU: any machine with hipcc).

relabel.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_measure_resources.py compiles its unit.  The four instantiations of volym_relabel_kernel<IDS, DISTANCE> must have no scratch, at
most 128 VGPRs and at most 64 KB of LDS.  The figures go to profiles/relabel_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, scene_bytes_holds_no_part_of, write_figures

OUT = os.path.join(ROOT, "profiles", "relabel_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit():
    return compile_unit("relabel")


def instantiations(res):
    """{(ids, distance): figures} of the volym_relabel_kernel<IDS, DISTANCE> instantiations"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_relabel_kernelILb([01])ELb([01])E", name)
        if m:
            out[(m.group(1) == "1", m.group(2) == "1")] = r
    return out


def test_the_unit_includes_the_new_header_and_no_other_unit_does():
    assert makefile_builds("relabel")
    assert only_unit_including("relabel_kernels.h", "relabel.hip")
    assert scene_bytes_holds_no_part_of("relabel_kernels.h")


def test_the_four_instantiations_have_no_scratch_128_vgprs_and_64_kb_of_lds(scene_unit):
    inst = instantiations(scene_unit)
    assert set(inst) == {(False, False), (False, True), (True, False), (True, True)}, list(scene_unit)
    lines = ["volym_relabel_kernel<IDS, DISTANCE> (relabel.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_relabel_resources.py; bar for all four: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for (ids, distance), r in sorted(inst.items()):
        lines.append("relabel_kernel<%-5s, %-5s>  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (
            str(ids).lower(), str(distance).lower(), r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for key, r in inst.items():
        assert r["scratch"] == 0, (key, r)
        assert r["vgpr"] <= 128, (key, r)
        assert r["lds"] <= 65536, (key, r)
