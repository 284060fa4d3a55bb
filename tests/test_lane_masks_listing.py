"""The march's lane predicates are wave masks in scalar registers (no GPU: any machine with hipcc).

raymarch_common.hip is compiled as tests/test_kernel_resources.py compiles it, and the three hot loops of the headline
instantiation -- the depth-parallel march, the classic march, the shading of the queue -- are read for what the compiler makes of
a predicate that is not kept as a mask:

  * a lane mask turned into a 0/1 integer per lane (v_cndmask_b32 vX, 0, 1, mask) and back into the same mask
    (v_cmp_ne_u32 ..., 0, vX) a few instructions later: a ballot of a bool that is not itself a compare, or a bool carried round
    the loop;
  * an SDWA compare of two such materialised predicates (a comparison of two bools).

Neither computes anything; both sit in the slow issue class (profiles/r02_valu_classes.txt).  The VALU bounds are those of the
listing of this hipcc: 380 for the classic loop (397 before the masks), 438 for the depth-parallel loop (444 less its three pairs).
"""
import os
import re

import pytest

from tests.test_kernel_resources import HEADLINE, HIPCC, compile_listing, hot_loops, kernel_body, makefile_flags

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

WINDOW = 8                  # "within the next few instructions"
CLASSIC_VALU_MAX = 380
DEPTH_PARALLEL_VALU_MAX = 438


@pytest.fixture(scope="module")
def hot(tmp_path_factory):
    listing, _ = compile_listing(tmp_path_factory.mktemp("lane_masks"), "raymarch_common.hip", makefile_flags()[1])
    body, labels = kernel_body(listing, HEADLINE)
    found = hot_loops(body, labels)
    assert len(found) == 3, found
    return body, found


def materialised(seg):
    """[(index, register)] of every v_cndmask_b32 vX, 0, 1, <mask> of a loop"""
    out = []
    for i, ins in enumerate(seg):
        m = re.match(r"v_cndmask_b32(?:_e32|_e64)?\s+(v\d+),\s*0,\s*1,\s*(vcc|s\[\d+:\d+\])$", ins)
        if m:
            out.append((i, m.group(1)))
    return out


def round_trips(seg):
    """[(the v_cndmask, the v_cmp_ne_u32 that reads its result back as a mask)]"""
    out = []
    for i, reg in materialised(seg):
        for j in range(i + 1, min(i + 1 + WINDOW, len(seg))):
            if re.match(r"v_cmp_ne_u32(?:_e32|_e64)?\s+(vcc|s\[\d+:\d+\]),\s*0,\s*%s$" % reg, seg[j]):
                out.append((seg[i], seg[j]))
                break
            if re.match(r"v_\w+\s+%s\b" % reg, seg[j]):         # overwritten: no longer the predicate
                break
    return out


def sdwa_bool_compares(seg):
    """SDWA compares with an operand that a v_cndmask 0, 1 of this loop wrote"""
    regs = {reg for _, reg in materialised(seg)}
    out = []
    for ins in seg:
        if re.match(r"v_cmp\w*_sdwa\b", ins) and regs & set(re.findall(r"\bv\d+\b", ins)):
            out.append(ins)
    return out


def names(body, found):
    """(depth-parallel march, classic march, shading of the queue): the marches in the order of the source, the shading last and
    by far the smallest"""
    by_size = sorted(found, key=lambda ab: sum(x.startswith("v_") for x in body[ab[0]:ab[1] + 1]))
    flush = by_size[0]
    dp, classic = sorted(by_size[1:])
    return {"depth-parallel march": dp, "classic march": classic, "shading of the queue": flush}


def valu(body, ab):
    return sum(x.startswith("v_") for x in body[ab[0]:ab[1] + 1])


def test_no_mask_is_turned_into_an_integer_and_back(hot):
    body, found = hot
    bad = []
    for name, (a, b) in names(body, found).items():
        seg = body[a:b + 1]
        pairs = round_trips(seg)
        print("%-22s %5d..%5d  valu %4d  v_cndmask 0,1: %2d  mask -> int -> mask pairs: %d" % (name, a, b, valu(body, (a, b)), len(materialised(seg)), len(pairs)))
        bad += [(name,) + p for p in pairs]
    assert not bad, bad


def test_no_sdwa_compare_of_materialised_predicates(hot):
    body, found = hot
    bad = []
    for name, (a, b) in names(body, found).items():
        cmps = sdwa_bool_compares(body[a:b + 1])
        print("%-22s SDWA compares of bools: %d" % (name, len(cmps)))
        bad += [(name, c) for c in cmps]
    assert not bad, bad


def test_march_loops_are_no_longer_than_the_listing_bounds(hot):
    body, found = hot
    n = names(body, found)
    classic, dp = valu(body, n["classic march"]), valu(body, n["depth-parallel march"])
    print("classic march: %d VALU (at most %d), depth-parallel march: %d VALU (at most %d), shading: %d VALU" %
          (classic, CLASSIC_VALU_MAX, dp, DEPTH_PARALLEL_VALU_MAX, valu(body, n["shading of the queue"])))
    assert classic <= CLASSIC_VALU_MAX
    assert dp <= DEPTH_PARALLEL_VALU_MAX
