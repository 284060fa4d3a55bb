"""What the compiler made of the cost pass's kernels (no GPU: any machine with hipcc).

cost.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_geodesic_resources.py compiles geodesic.hip.  Every kernel of the unit -- both instantiations of the init kernel and the
zero, relax, finish and pack kernels; the spread launches the flood's kernel of geodesic.hip, so the unit holds no edit kernel -- must
have no scratch, at most 128 VGPRs and at most 64 KB of LDS, and the relax kernel no more LDS than its arrays add up to: the keys and
the bytes of a tile with its halo, one word of face bits and three of iteration flags.  Only the resource remarks are read, never the
instructions.  The figures go to profiles/cost_kernel_resources.txt.  geodesic.hip must still yield exactly its eight kernels, nearest.hip its nine and
distance.hip its seven.
"""
import os
import re

import pytest

from tests import cost_scenes as CS
from tests.kernel_listing import CSRC, HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, write_figures

OUT = os.path.join(ROOT, "profiles", "cost_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

EXPECTED = {"init<false>", "init<true>", "zero", "relax", "finish", "pack"}


@pytest.fixture(scope="module")
def cost_unit():
    return compile_unit("cost")


def kernels(res):
    """{name: figures} of the cost kernels, the template as name<flag>"""
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_cost_(init)_kernelILb([01])EE", name)
        if m:
            out["%s<%s>" % (m.group(1), "true" if m.group(2) == "1" else "false")] = r
            continue
        m = re.search(r"volym_cost_(zero|relax|finish|pack)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("cost")
    assert only_unit_including("cost_kernels.h", "cost.hip")
    assert only_unit_including("geodesic_kernels.h", "geodesic.hip")       # the unit copies what it needs of that header
    assert "__global__" not in open(os.path.join(CSRC, "cost.hip")).read()


def test_every_kernel_has_no_scratch_128_vgprs_and_the_relax_kernel_the_lds_of_its_arrays(cost_unit):
    found = kernels(cost_unit)
    assert set(found) == EXPECTED and len(cost_unit) == len(EXPECTED), list(cost_unit)
    tx, ty, tz = CS.tile()
    halo = (tx + 2) * (ty + 2) * (tz + 2)
    arrays = 4 * halo + halo + 4 + 12                               # s_key, s_byte, s_faces, s_lowered
    lines = ["the kernels of cost.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_cost_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536; relax: LDS <= %d, what its arrays add up to" % arrays, ""]
    for name, r in sorted(found.items()):
        lines.append("cost %-15s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)
    assert (tx, ty, tz) == (32, 8, 8) and arrays == 17016
    assert 4 * halo <= found["relax"]["lds"] <= arrays, found["relax"]


def test_the_geodesic_nearest_and_distance_units_still_yield_exactly_their_kernels():
    from tests import test_distance_resources as D
    from tests import test_geodesic_resources as G
    from tests import test_nearest_resources as N
    unit = compile_unit("geodesic")
    assert set(G.kernels(unit)) == G.EXPECTED and len(unit) == 8, list(unit)
    unit = compile_unit("nearest")
    assert set(N.kernels(unit)) == N.EXPECTED and len(unit) == 9, list(unit)
    unit = compile_unit("distance")
    assert set(D.kernels(unit)) == D.EXPECTED and len(unit) == 7, list(unit)
