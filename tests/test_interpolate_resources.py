"""What the compiler made of the interpolate pass's and its edit's kernels (no GPU: any machine with hipcc).

interpolate.hip is compiled device-only with the Makefile's own flags and -Rpass-analysis=kernel-resource-usage, as
tests/test_nearest_resources.py compiles nearest.hip.  Every kernel of the unit -- the four instantiations of the rows kernel, both of
the resolve kernel, the init, keys, columns and gather kernels and the two edit kernels -- must have no scratch, at most 128 VGPRs and
at most 64 KB of LDS.  Only the resource remarks are read, never the instructions.  The figures go to
profiles/interpolate_kernel_resources.txt.  distance.hip, nearest.hip, geodesic.hip and cost.hip must still yield exactly their kernels.
"""
import os
import re

import pytest

from tests.kernel_listing import HIPCC, ROOT, compile_unit, makefile_builds, only_unit_including, write_figures

OUT = os.path.join(ROOT, "profiles", "interpolate_kernel_resources.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

EXPECTED = {"rows<false,false>", "rows<false,true>", "rows<true,false>", "rows<true,true>", "resolve<false>", "resolve<true>", "init", "keys", "columns", "gather", "edit",
            "edit_journal"}


@pytest.fixture(scope="module")
def interpolate_unit():
    return compile_unit("interpolate")


def kernels(res):
    """{name: figures} of the interpolate kernels, the templates as name<flags>"""
    flag = {"0": "false", "1": "true"}
    out = {}
    for name, r in res.items():
        m = re.search(r"volym_interpolate_rows_kernelILb([01])ELb([01])EE", name)
        if m:
            out["rows<%s,%s>" % (flag[m.group(1)], flag[m.group(2)])] = r
            continue
        m = re.search(r"volym_interpolate_resolve_kernelILb([01])EE", name)
        if m:
            out["resolve<%s>" % flag[m.group(1)]] = r
            continue
        m = re.search(r"volym_interpolate_(init|keys|columns|gather|edit_journal|edit)_kernel", name)
        if m:
            out[m.group(1)] = r
    return out


def test_the_makefile_builds_the_unit_and_only_it_holds_the_kernels():
    assert makefile_builds("interpolate")
    assert only_unit_including("interpolate_kernels.h", "interpolate.hip")
    assert only_unit_including("distance_kernels.h", "distance.hip")        # the unit copies the column sweep rather than include it


def test_every_kernel_has_no_scratch_128_vgprs_and_64_kb_of_lds(interpolate_unit):
    found = kernels(interpolate_unit)
    assert set(found) == EXPECTED and len(interpolate_unit) == len(EXPECTED), list(interpolate_unit)
    lines = ["the kernels of interpolate.hip, hipcc with the Makefile's flags, -Rpass-analysis=kernel-resource-usage",
             "written by tests/test_interpolate_resources.py; bar for all: scratch 0, VGPRs <= 128, LDS <= 65536", ""]
    for name, r in sorted(found.items()):
        lines.append("interpolate %-18s  vgpr %3d  sgpr %3d  scratch %4d  occupancy %d  lds %5d" % (name, r["vgpr"], r["sgpr"], r["scratch"], r["occ"], r["lds"]))
    write_figures(OUT, lines)
    for name, r in found.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] <= 65536, (name, r)


def test_the_unit_yields_its_twelve_kernels_and_the_distance_nearest_geodesic_and_cost_units_still_theirs(interpolate_unit):
    """interpolate.hip yields its twelve kernels, and distance.hip, nearest.hip, geodesic.hip and cost.hip still exactly theirs"""
    from tests import test_cost_resources as K
    from tests import test_distance_resources as D
    from tests import test_geodesic_resources as G
    from tests import test_nearest_resources as N
    found = {"interpolate": (set(kernels(interpolate_unit)), len(interpolate_unit))}
    for unit_name, mod in (("distance", D), ("nearest", N), ("geodesic", G), ("cost", K)):
        unit = compile_unit(unit_name)
        found[unit_name] = (set(mod.kernels(unit)), len(unit))
    assert found == {"interpolate": (EXPECTED, 12), "distance": (D.EXPECTED, 7), "nearest": (N.EXPECTED, 9), "geodesic": (G.EXPECTED, 8), "cost": (K.EXPECTED, 6)}, found
