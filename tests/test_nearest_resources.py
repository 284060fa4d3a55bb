"""What the compiler made of the nearest pass's and the fill's kernels (no GPU: any machine with hipcc).

nearest.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_distance_resources.py compiles distance.hip.  Every kernel of the unit -- both instantiations of the rows and resolve
kernels, the init, columns and gather kernels and the two fill kernels -- must have no scratch, at most 128 VGPRs and at most 64 KB of
LDS.  Only the resource remarks are read, never the instructions.  The figures go to profiles/nearest_kernel_resources.txt.
distance.hip must still yield exactly its seven kernels.
"""
import os
import re

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, write_figures

OUT = os.path.join(ROOT, "profiles", "nearest_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

EXPECTED = {"rows<false>", "rows<true>", "resolve<false>", "resolve<true>", "init", "columns", "gather", "fill", "fill_journal"}


@pytest.fixture(scope="module")
def nearest_unit():
    return compile_unit("nearest")


def kernels(res):
    """{name: figures} of the nearest kernels, the templates as name<flag>"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_nearest_(rows|resolve)_kernelILb([01])EE", name)
        if m:
            out["%s<%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")] = r
            continue
        m = re.search(r"volym_nearest_(init|columns|gather|fill_journal|fill)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("nearest")
    assert only_unit_including("nearest_kernels.h", "nearest.hip")


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(nearest_unit):
    found = kernels(nearest_unit)
    assert set(found) == EXPECTED and len(nearest_unit) == len(EXPECTED), list(nearest_unit)
    lines = ["the kernels of nearest.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_nearest_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("nearest %-15s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)


def test_the_distance_unit_still_yields_exactly_its_seven_kernels():
    from tests import test_distance_resources as D
    unit = compile_unit("distance")
    assert set(D.kernels(unit)) == D.EXPECTED and len(unit) == 7, list(unit)
