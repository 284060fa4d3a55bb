"""What the compiler made of the slice kernel (no GPU: any machine with hipcc).

slice.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_outline_resources.py compiles the outline unit.  Both instantiations of volym_slice_kernel<BRICK> -- linear and bricked
density -- must have no scratch and at most 64 VGPRs: an address, up to three byte loads and two integer blends per lane need far
fewer.  No scratch also shows that palette and table, which arrive as kernel arguments and are indexed by the thread id on their
way into LDS, are read from the argument segment and not from a private copy.  Only the resource remarks and the kinds of store are
read.  The figures go to profiles/slice_kernel_resources.txt.
"""
import os
import re
import subprocess

import pytest

from tests.kernel_listing import CSRC, HIPCC, ROOT, makefile_builds, makefile_flags, remarks, write_figures

OUT = os.path.join(ROOT, "profiles", "slice_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def slice_unit(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("slice")), "slice.s")
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, "slice.hip"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return open(out).read(), remarks(p.stderr)


def instantiations(res):
    """{bricked: figures} of the volym_slice_kernel<BRICK> instantiations"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_slice_kernelILb([01])E", name)
        if m:
            out[m.group(1) == "1"] = r
    return out


def test_the_makefile_builds_and_links_the_unit():
    assert makefile_builds("slice")


def test_every_instantiation_has_no_scratch_and_at_most_64_vgprs(slice_unit):
    res = slice_unit[1]
    inst = instantiations(res)
    assert len(res) == 2 and set(inst) == {False, True}, list(res)      # the unit holds its two instantiations and nothing else
    lines = ["volym_slice_kernel<BRICK> (slice.hip), hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_slice_resources.py; bar for both: scratch 0, VGPRs <= 64", ""]
    for brick, r in sorted(inst.items()):
        lines.append("slice_kernel<%-5s>  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (
            str(brick).lower(), r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for brick, r in inst.items():
        assert r["scratch"] == 0, (brick, r)
        assert r["vgpr"] <= 64, (brick, r)


def test_the_unit_holds_no_frame_pick_outline_or_scene_kernel(slice_unit):
    res = slice_unit[1]
    assert not [n for n in res if "volym_raymarch" in n or "volym_pick" in n or "volym_outline" in n or "volym_scene" in n], list(res)


def test_a_pixel_leaves_through_one_dword_store(slice_unit):
    body = [l.strip() for l in slice_unit[0].split("\n")]
    stores = [l for l in body if l.startswith(("global_store", "flat_store", "buffer_store", "scratch_store"))]
    assert stores and all(l.startswith("global_store_dword ") for l in stores), sorted(set(s.split()[0] for s in stores))
    assert len(stores) == 2, stores           # one per instantiation
