"""What the compiler made of the kernels of the label history (no GPU: any machine with hipcc).

relabel.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_relabel_resources.py compiles its unit.  The four instantiations of volym_relabel_journal_kernel<IDS, DISTANCE> and
volym_label_swap_kernel must have no scratch, at most 128 VGPRs and at most 64 KB of LDS.  Only the resource remarks are read, never
the instructions.  The figures go to profiles/label_history_kernel_resources.txt.
"""
import os
import re

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, write_figures

OUT = os.path.join(ROOT, "profiles", "label_history_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit():
    return compile_unit("relabel")


def kernels(res):
    """{name: figures} of the journalling instantiations and the swap kernel"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_relabel_journal_kernelILb([01])ELb([01])E", name)
        if m:
            out["relabel_journal_kernel<%-5s, %-5s>" % (str(m.group(1) == "1").lower(), str(m.group(2) == "1").lower())] = r
        elif "volym_label_swap_kernel" in name:
            out["label_swap_kernel"] = r
    return out


def test_the_journalling_instantiations_and_the_swap_kernel_have_no_scratch_128_vgprs_and_64_kb_of_lds(scene_unit):
    found = kernels(scene_unit)
    assert len(found) == 5 and "label_swap_kernel" in found, list(scene_unit)
    lines = ["volym_relabel_journal_kernel<IDS, DISTANCE> and volym_label_swap_kernel (relabel.hip), hipcc with the Makefile's flags, "
             "-Rpass-analysis=kernel-resource-usage",
             "written by tests/test_label_history_resources.py; bar for all five: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("%-38s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)
