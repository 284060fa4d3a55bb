"""What the compiler made of the measure kernel (no GPU: any machine with hipcc).

scene_bytes.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_project_resources.py compiles project.hip.  Both instantiations of volym_measure_kernel<LABELS> must have no scratch, at
most 128 VGPRs and at most 64 KB of LDS (two workgroups fit the 160 KB of a CU).  The figures go to
profiles/measure_kernel_resources.txt.
"""
import os
import re
import subprocess

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_flags, remarks

OUT = os.path.join(ROOT, "profiles", "measure_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def scene_unit(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("measure")), "scene_bytes.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "scene_bytes.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return remarks(p.stderr)


def instantiations(res):
    """{labels: figures} of the volym_measure_kernel<LABELS> instantiations"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_measure_kernelILb([01])E", name)
        if m:
            out[m.group(1) == "1"] = r
    return out


def test_the_makefile_lists_the_new_header_among_the_units_dependencies():
    text = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^\$\(HERE\)scene_bytes\$\(SFX\)\.o:(.*)\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -c", text, re.M)
    assert rule and "$(HDRS)" in rule.group(1)
    hdrs = re.search(r"^HDRS\s*:=\s*\$\(wildcard (.*)\)$", text, re.M).group(1).split()
    assert "$(HERE)*.h" in hdrs and "$(HERE)*.inc" in hdrs            # measure_kernels.h and measure.inc
    assert os.path.exists(os.path.join(CSRC, "measure_kernels.h")) and os.path.exists(os.path.join(CSRC, "measure.inc"))
    unit = open(os.path.join(CSRC, "scene_bytes.hip")).read()
    assert unit.index('#include "scene_kernels.h"') < unit.index('#include "measure_kernels.h"')
    others = [f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and f != "scene_bytes.hip"]
    for f in others:                                                  # scene_bytes.hip stays the only unit with these kernels
        assert '#include "measure_kernels.h"' not in open(os.path.join(CSRC, f)).read(), f


def test_both_instantiations_have_no_scratch_128_vgprs_and_64_kb_of_lds(scene_unit):
    inst = instantiations(scene_unit)
    assert set(inst) == {False, True}, list(scene_unit)
    lines = ["volym_measure_kernel<LABELS> (scene_bytes.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_measure_resources.py; bar for both: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for labels, r in sorted(inst.items()):
        lines.append("measure_kernel<%-5s>  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (
            str(labels).lower(), r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    print("\n".join(lines))
    try:
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                  # a read-only checkout still checks the bar
    for labels, r in inst.items():
        assert r["scratch"] == 0, (labels, r)
        assert r["vgpr"] <= 128, (labels, r)
        assert r["lds"] <= 65536, (labels, r)
