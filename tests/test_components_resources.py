"""What the compiler made of the components kernels (no GPU: any machine with hipcc).

components.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_surface_resources.py compiles surface.hip.  Every kernel of the unit -- every instantiation of the rows, merge and number
kernels, and the init, flatten, relabel and pack kernels -- must have no scratch, at most 128 VGPRs and at most 64 KB of LDS (the scan
of the row counts is box_pass.hip's: tests/test_box_pass_resources.py).  The figures go to profiles/components_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, write_figures

OUT = os.path.join(ROOT, "profiles", "components_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

EXPECTED = {"rows<false,false>", "rows<true,false>", "rows<true,true>", "merge<false>", "merge<true>", "number<false>", "number<true>",
            "init", "flatten", "relabel", "pack"}


@pytest.fixture(scope="module")
def components_unit():
    return compile_unit("components")


def kernels(res):
    """{name: figures} of the components kernels, the templates as name<flags>"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_components_(rows|merge|number)_kernelI((?:Lb[01]E)+)E", name)
        if m:
            flags = ",".join("true" if b == "1" else "false" for b in re.findall(r"Lb([01])E", m.group(2)))
            out["%s<%s>" % (m.group(1), flags)] = r
            continue
        m = re.search(r"volym_components_(init|flatten|relabel|pack)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("components")
    assert '#include "components_kernels.h"' in open(os.path.join(CSRC, "components.hip")).read()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and f != "components.hip":
            assert '#include "components_kernels.h"' not in open(os.path.join(CSRC, f)).read(), f


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(components_unit):
    found = kernels(components_unit)
    assert set(found) == EXPECTED, list(components_unit)
    lines = ["the kernels of components.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_components_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("components %-19s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)
