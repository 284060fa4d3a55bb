"""What the compiler made of the pick kernels (no GPU: any machine with hipcc).

pick.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_kernel_resources.py compiles the march units.  The table-mode, linear-layout instantiation -- what a pick of the common
frame runs -- must have no scratch and at most 128 VGPRs: volym_raymarch_kernel<1, false, false, false>, whose launch shape and
leaps it shares, does strictly more per ray (gradient taps, shading, colour) in 96 VGPRs and no scratch
(profiles/r02_kernel_resources.txt).  The figures of every instantiation go to profiles/pick_kernel_resources.txt; the general ones
(look-ahead, smoothing, trilinear, colouring) have no bar.
"""
import os
import re
import subprocess

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_builds, makefile_flags, remarks, write_figures

OUT = os.path.join(ROOT, "profiles", "pick_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def pick_unit(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("pick")), "pick.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "pick.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return open(out).read(), remarks(p.stderr)


def instantiations(res):
    """{(bricked, general): figures} of the volym_pick_kernel<BRICK, GENERAL> instantiations"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_pick_kernelILb([01])ELb([01])E", name)
        if m:
            out[(m.group(1) == "1", m.group(2) == "1")] = r
    return out


def test_the_makefile_builds_and_links_the_unit():
    assert makefile_builds("pick")


def test_common_instantiation_has_no_scratch_and_fits_four_waves(pick_unit):
    inst = instantiations(pick_unit[1])
    assert set(inst) == {(False, False), (False, True), (True, False), (True, True)}, list(pick_unit[1])
    lines = ["volym_pick_kernel<BRICK, GENERAL> (pick.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_pick_resources.py; bar: <false, false> scratch 0, VGPRs <= 128; none for the others", ""]
    for (brick, general), r in sorted(inst.items()):
        lines.append("pick_kernel<%-5s, %-5s>  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (
            str(brick).lower(), str(general).lower(), r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    common = inst[(False, False)]
    assert common["scratch"] == 0, common
    assert common["vgpr"] <= 128, common


def test_the_unit_holds_no_frame_kernel_and_no_scalar_memory_write(pick_unit):
    listing, res = pick_unit
    assert not [n for n in res if "volym_raymarch" in n], "pick.hip must not instantiate the frame kernels"
    # records leave through vector stores: exactly the 16-byte store per lane
    body = [l.strip() for l in listing.split("\n")]
    stores = [l for l in body if l.startswith(("global_store", "flat_store", "buffer_store"))]
    assert stores and all(l.startswith("global_store_dwordx4") for l in stores), sorted(set(s.split()[0] for s in stores))
    assert not [l for l in body if re.match(r"s_(buffer_|scratch_)?(store|atomic)", l)]
