"""What the compiler made of the distance kernels (no GPU: any machine with hipcc).

distance.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_components_resources.py compiles components.hip.  Every kernel of the unit -- both instantiations of the rows and finish
kernels, and the init, columns and pack kernels -- must have no scratch, at most 128 VGPRs and at most 64 KB of LDS.  The figures go
to profiles/distance_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, write_figures

OUT = os.path.join(ROOT, "profiles", "distance_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

EXPECTED = {"rows<false>", "rows<true>", "finish<false>", "finish<true>", "init", "columns", "pack"}


@pytest.fixture(scope="module")
def distance_unit():
    return compile_unit("distance")


def kernels(res):
    """{name: figures} of the distance kernels, the templates as name<flag>"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_distance_(rows|finish)_kernelILb([01])EE", name)
        if m:
            out["%s<%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")] = r
            continue
        m = re.search(r"volym_distance_(init|columns|pack)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("distance")
    assert '#include "distance_kernels.h"' in open(os.path.join(CSRC, "distance.hip")).read()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and f != "distance.hip":
            assert '#include "distance_kernels.h"' not in open(os.path.join(CSRC, f)).read(), f


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(distance_unit):
    found = kernels(distance_unit)
    assert set(found) == EXPECTED, list(distance_unit)
    lines = ["the kernels of distance.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_distance_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("distance %-14s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)
