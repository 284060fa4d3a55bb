"""The twin of the headline instantiation for volumes of 256 texels on every axis (no GPU: any machine with hipcc).

raymarch_common.hip is compiled as tests/test_kernel_resources.py compiles it.  volym_raymarch_cube256_kernel is the headline
instantiation's body with one difference: a texel address is the three clamped coordinates as bytes side by side, one v_cvt_pk_u8_f32
each (raymarch_device.h, texel256_insert), where the general kernel converts (v_cvt_flr_i32_f32), clamps (v_med3_i32) and folds
(v_mad_u32_u24).  The listing is read for what that is worth and for what the headline instantiation is held to:

  * the twin exists once, has no scratch, at most 128 VGPRs, four waves per SIMD, and reads FrameParams from the place the code
    object's metadata gives the argument;
  * it has the three hot loops, without v_readlane, v_writelane or scratch access;
  * in them no v_med3_i32 at all, and no v_mad_u32_u24 whose result is the address of a global_load_ubyte;
  * each loop holds at least 4 (depth-parallel march), 8 (classic march) and 11 (shading of the queue) VALU instructions fewer than
    the same loop of the general instantiation in the same listing: the counts of voxel-address instructions the packed form saves
    per iteration (2 samples per lane, 4 samples, 6 taps and the centre);
  * the entry top of the twin has no flat access, no uniform word through vector memory, and stores its constant tiles without
    draining vector memory (tests/test_entry_top_listing.py).
"""
import os
import re

import pytest

from tests.test_entry_top_listing import VM_DRAIN, flat_accesses, uniform_word_round_trips
from tests.test_kernel_resources import HEADLINE, HIPCC, compile_listing, hot_loops, kernel_body, kernels_metadata, loops, makefile_flags, remarks
from tests.test_lane_masks_listing import names, valu

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

# the same template arguments as the headline instantiation, under the twin's name
TWIN = HEADLINE.replace("volym_raymarch_pq_kernel", "volym_raymarch_cube256_kernel")
SAVED = {"depth-parallel march": 4, "classic march": 8, "shading of the queue": 11}


@pytest.fixture(scope="module")
def common(tmp_path_factory):
    return compile_listing(tmp_path_factory.mktemp("cube256"), "raymarch_common.hip", makefile_flags()[1])


def twin_hot_loops(body, labels):
    """hot_loops of tests/test_kernel_resources.py with its floor of 80 VALU instructions lowered by the 11 that the packed form takes
    out of the shading loop: that loop has 89 in the general instantiation and 78 here, and the next smaller loops (the replay of
    empty steps) have 40 in both."""
    floor = 80 - SAVED["shading of the queue"]
    cand = []
    for a, b in loops(body, labels):
        seg = body[a:b + 1]
        if any(x.startswith(("global_store", "global_atomic", "flat_store", "buffer_store")) for x in seg):
            continue
        if sum(1 for x in seg if x.startswith("v_")) >= floor:
            cand.append((a, b))
    return sorted(set((a, b) for a, b in cand if not any((c <= a and b <= d) and (c, d) != (a, b) for c, d in cand)))


@pytest.fixture(scope="module")
def twin(common):
    body, labels = kernel_body(common[0], TWIN)
    return body, twin_hot_loops(body, labels)


def address_registers(ins):
    """the VGPRs a global load takes its address from: the pair of a 64-bit address, or the 32-bit offset beside a scalar base"""
    m = re.match(r"global_load_\w+\s+v\d+,\s*(v\[(\d+):(\d+)\]|v(\d+))", ins)
    if not m:
        return set()
    return {"v%s" % m.group(2), "v%s" % m.group(3)} if m.group(2) else {"v%s" % m.group(4)}


def mads_feeding_byte_loads(seg):
    """[(v_mad_u32_u24, global_load_ubyte)]: the multiply-add writes a register that the load, later in the loop, takes its address
    from, with nothing in between that writes the register again"""
    out = []
    for i, ins in enumerate(seg):
        m = re.match(r"v_mad_u32_u24\s+(v\d+),", ins)
        if not m:
            continue
        reg = m.group(1)
        for later in seg[i + 1:]:
            if later.startswith("global_load_ubyte") and reg in address_registers(later):
                out.append((ins, later))
                break
            if re.match(r"v_\w+\s+%s\b" % reg, later) or re.match(r"(global|ds)_load\w*\s+%s\b" % reg, later):
                break
    return out


def test_twin_exists_once_without_scratch(common):
    listing, err = common
    res = {k: v for k, v in remarks(err).items() if "volym_raymarch_cube256_kernel" in k}
    assert len(res) == 1 and TWIN in next(iter(res)), list(remarks(err))
    r = next(iter(res.values()))
    print("volym_raymarch_cube256_kernel:", r)
    assert r["scratch"] == 0
    assert r["vgpr"] <= 128
    assert r["occ"] == 4
    body, _ = kernel_body(listing, TWIN)
    assert not [x for x in body if x.startswith("scratch_")]
    assert sum(x.startswith("v_cvt_pk_u8_f32") for x in body) >= 27       # 3 x (2 + 4) samples, 3 + 6 for a shading batch


def test_twin_reads_frame_params_where_the_code_object_has_them(common):
    listing, _ = common
    meta = kernels_metadata(listing)
    name = next(k for k in meta if TWIN in k)
    general = next(k for k in meta if HEADLINE in k)
    assert meta[name] == meta[general], "the twin's argument list is not the general kernel's"
    by_value = [a for a in meta[name] if a[2] == "by_value" and a[1] > 256]
    assert len(by_value) == 1, meta[name]
    lines = listing.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    used = [int(m.group(1), 0) for l in lines[start:end] for m in [re.search(r"frame_params_here: kernarg offset (\w+)", l)] if m]
    assert used and all(u == by_value[0][0] for u in used), (used, by_value)


def test_twin_hot_loops_hold_no_spill_code_and_no_general_addressing(twin):
    body, hot = twin
    assert len(hot) == 3, hot
    assert all(any(x.startswith("global_load_ubyte") for x in body[a:b + 1]) for a, b in hot)
    assert all(sum(x.startswith("ds_add_u32") for x in body[a:b + 1]) >= 3 for a, b in hot)
    for name, (a, b) in names(body, hot).items():
        seg = body[a:b + 1]
        spill = [x for x in seg if x.startswith(("v_readlane", "v_writelane", "scratch_"))]
        med3 = [x for x in seg if x.startswith("v_med3_i32")]
        mads = mads_feeding_byte_loads(seg)
        print("%-22s %5d..%5d  v_cvt_pk_u8_f32 %2d  v_floor_f32 %2d  v_med3_i32 %d  v_mad_u32_u24 into a byte load's address %d" %
              (name, a, b, sum(x.startswith("v_cvt_pk_u8_f32") for x in seg), sum(x.startswith("v_floor_f32") for x in seg), len(med3), len(mads)))
        assert not spill, (name, spill[:5])
        assert not med3, (name, med3[:5])
        assert not mads, (name, mads[:5])


def test_twin_loops_are_shorter_by_the_address_instructions(common, twin):
    body, hot = twin
    gbody, glabels = kernel_body(common[0], HEADLINE)
    ghot = hot_loops(gbody, glabels)
    assert len(ghot) == 3, ghot
    mine, general = names(body, hot), names(gbody, ghot)
    short = []
    for name, saved in SAVED.items():
        v, gv = valu(body, mine[name]), valu(gbody, general[name])
        print("%-22s %4d VALU, the general instantiation %4d: %3d fewer (at least %d)" % (name, v, gv, gv - v, saved))
        if v > gv - saved:
            short.append((name, v, gv, saved))
    assert not short, short


def test_twin_entry_top(common, twin):
    body, hot = twin
    assert not flat_accesses(body)
    assert not uniform_word_round_trips(body)
    # tests/test_entry_top_listing.py::test_headline_constant_tiles_are_stored_without_draining_vector_memory, for the twin
    barrier = next(i for i, x in enumerate(body) if x.startswith("s_barrier"))
    first_loop = min(a for a, _ in hot)
    fills = [i for i in range(barrier + 1, first_loop) if body[i].startswith("global_store")]
    assert fills, "no constant-tile store found between the barrier and the march loops"
    drains = [(i, body[i]) for i in range(barrier + 1, fills[0]) if VM_DRAIN.match(body[i])]
    assert not drains, drains
    ticket = next(i for i in range(barrier + 1, fills[0]) if body[i].startswith("ds_add_rtn_u32"))
    loads = [(i, body[i]) for i in range(ticket, fills[0]) if body[i].startswith(("global_load", "flat_load", "buffer_load"))]
    assert not loads, loads
