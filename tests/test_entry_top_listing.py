"""A wave starts a work-list entry without a vector-memory round trip (no GPU: any machine with hipcc).

raymarch_common.hip and raymarch.hip are compiled as tests/test_kernel_resources.py compiles them, and the listings are read for
what the top of an entry was made of before its words came through LDS and the scalar cache (raymarch_pq.h, the top of the
ticket loop; raymarch_device.h, launch_constant):

  (a) a flat access: the select between the staged copy of the list in LDS and the list in global memory was a select between two
      generic addresses, and the entry's two words two flat_load_dword one after the other;
  (b) a wave-uniform word fetched by a vector load, waited for and moved to a scalar register (global_load_dword, s_waitcnt vmcnt(0),
      v_readfirstlane of the loaded register): the tile-mask bits, four of them in a row for a 16x16 tile;
  (c) in the headline instantiation, a wait for ALL vector memory between the workgroup's barrier and the pixel stores of the
      constant-tile paths: it would drain the stores of the wave's previous entry before the entry's kind is known.

(a) and (b) hold for every volym_raymarch_pq_kernel instantiation: the code is shared.
"""
import os
import re

import pytest

from tests.test_kernel_resources import HEADLINE, HIPCC, compile_listing, hot_loops, kernel_body, makefile_flags

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

WINDOW = 4                  # "within four instructions"
VM_DRAIN = re.compile(r"s_waitcnt\s+(.*\b)?vmcnt\(0\)")


@pytest.fixture(scope="module")
def common(tmp_path_factory):
    return compile_listing(tmp_path_factory.mktemp("entry_top_common"), "raymarch_common.hip", makefile_flags()[1])[0]


@pytest.fixture(scope="module")
def rest(tmp_path_factory):
    return compile_listing(tmp_path_factory.mktemp("entry_top_rest"), "raymarch.hip", [])[0]


def pq_kernels(listing):
    """mangled names of the volym_raymarch_pq_kernel instantiations a listing defines"""
    return sorted(set(m.group(1) for m in re.finditer(r"^(_ZN\w*volym_raymarch_pq_kernel\w+):", listing, re.M)))


def flat_accesses(body):
    return [x for x in body if x.startswith("flat_")]


def uniform_word_round_trips(body):
    """[(global_load_dword vX, the s_waitcnt vmcnt(0), the v_readfirstlane of vX)] with both inside the next WINDOW instructions"""
    out = []
    for i, ins in enumerate(body):
        m = re.match(r"global_load_dword\s+(v\d+),", ins)
        if not m:
            continue
        nxt = body[i + 1:i + 1 + WINDOW]
        wait = next((j for j, x in enumerate(nxt) if VM_DRAIN.match(x)), None)
        if wait is None:
            continue
        read = next((x for x in nxt[wait + 1:] if re.match(r"v_readfirstlane_b32\s+s\d+,\s*%s$" % m.group(1), x)), None)
        if read:
            out.append((ins, nxt[wait], read))
    return out


def test_headline_entry_top_has_no_flat_access(common):
    body, _ = kernel_body(common, HEADLINE)
    bad = flat_accesses(body)
    print("flat accesses in the headline instantiation: %d" % len(bad))
    assert not bad, bad


def test_headline_entry_top_moves_no_uniform_word_through_vector_memory(common):
    body, _ = kernel_body(common, HEADLINE)
    bad = uniform_word_round_trips(body)
    print("global_load_dword -> s_waitcnt vmcnt(0) -> v_readfirstlane triples in the headline instantiation: %d" % len(bad))
    assert not bad, bad


def test_headline_constant_tiles_are_stored_without_draining_vector_memory(common):
    body, labels = kernel_body(common, HEADLINE)
    hot = hot_loops(body, labels)
    assert len(hot) == 3, hot
    barrier = next(i for i, x in enumerate(body) if x.startswith("s_barrier"))
    in_hot = lambda i: any(a <= i <= b for a, b in hot)
    # the constant-tile paths come first in the entry: their pixel stores are the global stores between the barrier and the first
    # hot loop (the marched pixels are stored behind the loops)
    first_loop = min(a for a, _ in hot)
    fills = [i for i in range(barrier + 1, first_loop) if body[i].startswith("global_store")]
    assert fills, "no constant-tile store found between the barrier and the march loops"
    first_store = fills[0]
    drains = [(i, body[i]) for i in range(barrier + 1, first_store) if not in_hot(i) and VM_DRAIN.match(body[i])]
    print("barrier at %d, first constant-tile store at %d (%s), last at %d, march loops from %d: vmcnt(0) waits in front of the first store: %d" %
          (barrier, first_store, body[first_store].split()[0], fills[-1], first_loop, len(drains)))
    assert not drains, drains
    # ... and from the ticket's LDS atomic to that store no vector or flat load at all: the entry's words and the mask bits are
    # LDS and scalar reads
    ticket = next(i for i in range(barrier + 1, first_store) if body[i].startswith("ds_add_rtn_u32"))
    loads = [(i, body[i]) for i in range(ticket, first_store) if body[i].startswith(("global_load", "flat_load", "buffer_load"))]
    assert not loads, loads


def test_no_instantiation_has_a_flat_access_or_a_uniform_round_trip(common, rest):
    seen, bad = 0, []
    for listing in (common, rest):
        for name in pq_kernels(listing):
            body, _ = kernel_body(listing, name)
            f, t = flat_accesses(body), uniform_word_round_trips(body)
            print("%-90s flat %d  round trips %d" % (name[-90:], len(f), len(t)))
            bad += [(name, x) for x in f + t]
            seen += 1
    assert seen >= 15, seen
    assert not bad, bad[:10]
