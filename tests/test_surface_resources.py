"""What the compiler made of the surface kernels (no GPU: any machine with hipcc).

surface.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_measure_resources.py compiles measure.hip.  Every instantiation of volym_surface_count_kernel<LABELS> and
volym_surface_emit_kernel<LABELS>, and the init kernel, must have no scratch, at most 128 VGPRs and at most 64 KB of LDS (the scan of
the row counts is box_pass.hip's: tests/test_box_pass_resources.py).  The figures go to profiles/surface_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, write_figures

OUT = os.path.join(ROOT, "profiles", "surface_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def surface_unit():
    return compile_unit("surface")


def kernels(res):
    """{name: figures} of the surface kernels, the templates as name<labels>"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_surface_(count|emit)_kernelILb([01])E", name)
        if m:
            out["%s<%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")] = r
            continue
        m = re.search(r"volym_surface_(init)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("surface")
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and f != "surface.hip":
            assert '#include "surface_kernels.h"' not in open(os.path.join(CSRC, f)).read(), f


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(surface_unit):
    found = kernels(surface_unit)
    assert set(found) == {"count<false>", "count<true>", "emit<false>", "emit<true>", "init"}, list(surface_unit)
    lines = ["the kernels of surface.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_surface_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("surface %-13s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)
