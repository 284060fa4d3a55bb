"""What the compiler made of the geodesic pass's and the flood's kernels (no GPU: any machine with hipcc).

geodesic.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_nearest_resources.py compiles nearest.hip.  Every kernel of the unit -- both instantiations of the init kernel, the zero,
relax, finish and pack kernels and the two flood kernels -- must have no scratch, at most 128 VGPRs and at most 64 KB of LDS.  Only
the resource remarks are read, never the instructions.  The figures go to profiles/geodesic_kernel_resources.txt.  nearest.hip must
still yield exactly its nine kernels and distance.hip its seven.
"""
import os
import re

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, write_figures

OUT = os.path.join(ROOT, "profiles", "geodesic_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

EXPECTED = {"init<false>", "init<true>", "zero", "relax", "finish", "pack", "flood", "flood_journal"}


@pytest.fixture(scope="module")
def geodesic_unit():
    return compile_unit("geodesic")


def kernels(res):
    """{name: figures} of the geodesic kernels, the template as name<flag>"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_geodesic_(init)_kernelILb([01])EE", name)
        if m:
            out["%s<%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")] = r
            continue
        m = re.search(r"volym_geodesic_(zero|relax|finish|pack|flood_journal|flood)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("geodesic")
    assert only_unit_including("geodesic_kernels.h", "geodesic.hip")


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(geodesic_unit):
    found = kernels(geodesic_unit)
    assert set(found) == EXPECTED and len(geodesic_unit) == len(EXPECTED), list(geodesic_unit)
    lines = ["the kernels of geodesic.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_geodesic_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("geodesic %-15s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)


def test_the_nearest_and_distance_units_still_yield_exactly_their_kernels():
    from tests import test_distance_resources as D
    from tests import test_nearest_resources as N
    unit = compile_unit("nearest")
    assert set(N.kernels(unit)) == N.EXPECTED and len(unit) == 9, list(unit)
    unit = compile_unit("distance")
    assert set(D.kernels(unit)) == D.EXPECTED and len(unit) == 7, list(unit)
