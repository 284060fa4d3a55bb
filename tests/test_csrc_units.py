"""The units of volym_amd/csrc and the Makefile that builds them (no GPU, no compiler: the files are read).

Every *.hip is a unit of its own: it is in the Makefile's UNITS list, which the one pattern rule compiles and the link line is derived
from.  Nothing is pasted onto the end of a unit but mgpu.inc, the native multi-GPU loop of raymarch.hip.
"""
import os
import re

from tests.kernel_listing import CSRC, makefile_builds, makefile_units


def test_every_hip_file_is_a_unit_the_makefile_builds_and_links():
    on_disk = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(makefile_units()) == on_disk
    for unit in on_disk:
        assert makefile_builds(unit), unit
    # one unit has flags of its own, through a target-specific variable: raymarch_common keeps COMFLAGS
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.findall(r"^(\S+): UNITFLAGS\s*:?=\s*(.*)$", text, re.M) == [("$(HERE)raymarch_common$(SFX).o", "$(COMFLAGS)")]


def test_no_inc_file_remains_but_the_multi_gpu_loop():
    assert [f for f in os.listdir(CSRC) if f.endswith(".inc")] == ["mgpu.inc"]
