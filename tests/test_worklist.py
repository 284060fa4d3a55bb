"""The work-list scheduler (volym_amd/csrc/worklist.cpp) and the entry code (worklist_entry.h), on the CPU.

The five functions are pure host arithmetic; the library exports them over flat arrays for this file alone (volym_wl_*, declared in
worklist.hpp, bound here with ctypes).  Everything they are checked against -- the entry code, the split threshold, the dilation,
the priorities, the dealing order -- is restated below in Python, independently of volym_amd/."""
import ctypes as C
import itertools

import numpy as np
import pytest

U32, U16, U8 = C.c_uint32, C.c_uint16, C.c_uint8
E_INVALID = -1


# ---- the entry code, restated -----------------------------------------------------------------------------------------
NO_ITEM = 0xFFFFFFFF
BIT_QUARTER, BIT_SUPER, PRIO_SHIFT, PRIO_MASK = 1 << 31, 1 << 30, 28, 3 << 28


def enc_quarter(item, q):
    return BIT_QUARTER | (item << 2) | q


def enc_super(lt):
    return BIT_SUPER | lt


def with_prio(code, prio):
    return code | (prio << PRIO_SHIFT)


def decode(entry):
    """-> (kind, value, quarter, prio); kind 'pad' | 'item' | 'quarter' (value: the item) | 'super' (value: the local tile)."""
    entry = int(entry)
    if entry == NO_ITEM:
        return ("pad", None, None, None)
    prio, code = (entry >> PRIO_SHIFT) & 3, entry & ~PRIO_MASK
    if code >> 31:
        return ("quarter", (code & 0x7FFFFFFF) >> 2, code & 3, prio)
    if code >> 30 == 1:
        return ("super", code & 0x3FFFFFFF, None, prio)
    return ("item", code, None, prio)


def local_tile_of(entry):
    kind, v, _, _ = decode(entry)
    return v if kind == "super" else v >> 2


# ---- the library's seam -----------------------------------------------------------------------------------------------
class ShardGrid(C.Structure):
    _fields_ = [(k, U32) for k in ("W", "H", "tiles_x", "tiles_y", "rank", "world", "n_local")]


class ListSettings(C.Structure):
    _fields_ = [("dp_min_cost", C.c_int), ("dp_share_pct", U32), ("dp_floor", U32), ("dilate", C.c_int), ("super_fill", C.c_bool),
                ("only_quarters", C.c_bool), ("dev_drop_tenths", U32), ("trim_rounds", U32), ("prio_tenths", U32 * 3)]


class CapturedLaunch(C.Structure):
    _fields_ = [("view_serial", C.c_uint64), ("captured_has_dp", C.c_bool), ("continuous", C.c_bool), ("plain", C.c_bool),
                ("max_grid", U32), ("waves", U32), ("grid", U32)]


class WlList(C.Structure):
    _fields_ = [("entries", C.POINTER(U32)), ("shares", C.POINTER(U16)), ("capacity", U32), ("n", U32), ("grid", U32), ("trim_round", U32),
                ("view_serial", C.c_uint64), ("has_dp", U8), ("trimmable", U8), ("final_for_view", U8)]


def settings(**kw):
    """The library's defaults (worklist.hpp ListSettings), then `kw`."""
    s = ListSettings(-1, 60, 64, -1, True, False, 0, 0, (U32 * 3)(3, 6, 10))
    for k, v in kw.items():
        setattr(s, k, (U32 * 3)(*v) if k == "prio_tenths" else v)
    return s


def launch(waves, max_grid, view_serial=7, captured_has_dp=False, continuous=False, plain=True, grid=0):
    return CapturedLaunch(view_serial, captured_has_dp, continuous, plain, max_grid, waves, grid)


def p32(a):
    return a.ctypes.data_as(C.POINTER(U32))


def p16(a):
    return a.ctypes.data_as(C.POINTER(U16))


class HostList:
    """A WorkList over numpy arrays."""

    def __init__(self, capacity=0, entries=None, shares=None, **kw):
        self.e = np.zeros(capacity, np.uint32) if entries is None else np.ascontiguousarray(entries, np.uint32)
        self.s = np.zeros(len(self.e), np.uint16) if shares is None else np.ascontiguousarray(shares, np.uint16)
        self.c = WlList(p32(self.e), p16(self.s), len(self.e), 0 if entries is None else len(self.e), kw.get("grid", 0), kw.get("trim_round", 0),
                        kw.get("view_serial", 0), kw.get("has_dp", 0), kw.get("trimmable", 0), kw.get("final_for_view", 0))

    @property
    def entries(self):
        return self.e[:self.c.n]

    @property
    def shares(self):
        return self.s[:self.c.n]


@pytest.fixture(scope="module")
def wl(volym_lib):
    from volym_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    G, S, J, LP = C.POINTER(ShardGrid), C.POINTER(ListSettings), C.POINTER(CapturedLaunch), C.POINTER(WlList)
    PU32, PU16, PU8 = C.POINTER(U32), C.POINTER(U16), C.POINTER(U8)
    for name, args in (("volym_wl_build_geometric", [G, PU32, U32, PU32]),
                       ("volym_wl_deal_list", [G, S, J, C.c_int, PU16, PU8, U32, PU32, U32, LP]),
                       ("volym_wl_trim_list", [S, J, U32, LP, PU32, LP]),
                       ("volym_wl_list_to_device_form", [G, PU32, U32, PU32]),
                       ("volym_wl_costs_to_items", [LP, PU16, U32, PU16, U32])):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    return L


# ---- shapes and inputs ------------------------------------------------------------------------------------------------
SHAPES = [(40, 24), (64, 32), (256, 144)]
SHARDS = [(0, 1), (1, 3)]
LAUNCHES = [(2, 4), (16, 256)]                       # (waves, max_grid): a grid that binds and pads, and one that does not
COSTS = ["zero", "equal", "heavy", "three_zero"]
GRIDS = list(itertools.product(SHAPES, SHARDS))


def shard_grid(shape, shard):
    (W, H), (rank, world) = shape, shard
    tx, ty = (W + 15) // 16, (H + 15) // 16
    n_local = (tx * ty - rank + world - 1) // world if tx * ty > rank else 0
    return ShardGrid(W, H, tx, ty, rank, world, n_local)


def sub_origin(g, item):
    tile = (item >> 2) * g.world + g.rank
    return (tile % g.tiles_x) * 16 + (item & 1) * 8, (tile // g.tiles_x) * 16 + ((item >> 1) & 1) * 8


def geometric(wl, g):
    out = np.zeros(g.n_local * 4, np.uint32)
    n = U32(0)
    assert wl.volym_wl_build_geometric(C.byref(g), p32(out), len(out), C.byref(n)) == 0
    return out[:n.value].copy()


def make_costs(kind, g, geo, seed=20261017):
    """Costs by item (4 * n_local).  Items that are not listed carry a cost too: nothing may read it."""
    rng = np.random.default_rng(seed + len(geo))
    cost = np.zeros(g.n_local * 4, np.uint16)
    if kind == "equal":
        cost[:] = 7
    elif kind == "heavy":                            # a few heavy items, a wide range of them, on a zero background
        idx = rng.choice(geo, size=max(2, len(geo) // 8), replace=False)
        cost[idx] = rng.integers(20, 3000, size=len(idx))
        cost[idx[0]] = 65535
    elif kind == "three_zero":                       # every other tile: one heavy item, its three siblings zero
        for lt in range(0, g.n_local, 2):
            cost[lt * 4 + int(rng.integers(0, 4))] = int(rng.integers(100, 2000))
    return cost


def deal(wl, g, set_, job, moving, cost, geo, is_dp=None):
    is_dp = np.zeros(g.n_local * 4, np.uint8) if is_dp is None else is_dp.copy()
    out = HostList(g.n_local * 16 + 2 * job.max_grid * 8 + 64)
    rc = wl.volym_wl_deal_list(C.byref(g), C.byref(set_), C.byref(job), int(moving), p16(cost), is_dp.ctypes.data_as(C.POINTER(U8)), len(cost),
                               p32(geo), len(geo), C.byref(out.c))
    assert rc == 0
    return out, is_dp


# ---- the rules of deal_list, restated ---------------------------------------------------------------------------------
def dilated(g, cost, geo, r):
    if r <= 0:
        return cost.astype(np.int64)
    gw, gh = g.tiles_x * 2, g.tiles_y * 2
    cell = np.zeros((gh, gw), np.int64)
    pos = {}
    for item in geo:
        x0, y0 = sub_origin(g, int(item))
        pos[int(item)] = (y0 // 8, x0 // 8)
        cell[y0 // 8, x0 // 8] = cost[item]
    out = cost.astype(np.int64)
    for item, (y, x) in pos.items():
        out[item] = cell[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].max()
    return out


def restate(g, set_, job, moving, cost, geo, was_dp):
    """What deal_list must decide: per listed item 'item' | 'quarter' | 'super', its share, and the list's flags."""
    r = set_.dilate if set_.dilate >= 0 else (1 if moving else 0)
    k = dilated(g, cost, geo, r)
    total = int(sum(int(k[i]) for i in geo))
    resident = max(1, job.max_grid * job.waves)
    tenths = -set_.dp_min_cost if set_.dp_min_cost < -1 else (12 if job.continuous else 19 if (job.plain and not moving) else 15)
    thr = max(set_.dp_floor, tenths * total // (10 * resident) + 16) if set_.dp_min_cost < 0 else set_.dp_min_cost
    measuring = (not moving) and job.captured_has_dp and set_.dp_min_cost < 0
    dp_ok = set_.dp_min_cost != 0 and not measuring
    listed = {}
    for i in geo:
        listed.setdefault(int(i) >> 2, []).append(int(i))
    fill = {lt for lt, items in listed.items() if set_.super_fill and len(items) == 4 and all(k[i] == 0 for i in items)}
    kind, share = {}, {}
    for i in (int(x) for x in geo):
        ki = int(k[i])
        if i >> 2 in fill:
            kind[i], share[i] = "super", 0
        elif dp_ok and (ki >= thr or (moving and was_dp[i] and set_.dp_min_cost < 0 and 10 * ki >= 7 * thr)):
            kind[i], share[i] = "quarter", (ki * set_.dp_share_pct + 99) // 100
        else:
            kind[i], share[i] = "item", ki
    fair = max(1, total // resident)
    t = list(set_.prio_tenths)

    def prio(s):
        if t[0] == 0 or s == 0:
            return 0
        return 3 if 10 * s >= t[2] * fair else 2 if 10 * s >= t[1] * fair else 1 if 10 * s >= t[0] * fair else 0
    return dict(kind=kind, share=share, prio=prio, thr=thr, measuring=measuring, fill=fill)


def dealing_order(a, G):
    """The list row by row, odd rows reversed: the order in which deal_list laid the sorted entries down."""
    rows = a.reshape(-1, G).copy()
    rows[1::2] = rows[1::2, ::-1]
    return rows.reshape(-1)


def check_dealt(g, set_, job, moving, cost, geo, was_dp, out, is_dp):
    want = restate(g, set_, job, moving, cost, geo, was_dp)
    ent, sh = out.entries, out.shares
    # shape of the list
    n = int((ent != NO_ITEM).sum())
    G = max(1, min((n + job.waves - 1) // job.waves, job.max_grid))
    assert out.c.grid == G and len(ent) == G * ((n + G - 1) // G)
    assert len(ent) <= g.n_local * 16 + 2 * job.max_grid * 8 + 64                      # reset_slot_lists' capacity, one workgroup per CU
    e_deal, s_deal = dealing_order(ent, G), dealing_order(sh, G).astype(np.int64)
    assert (e_deal[:n] != NO_ITEM).all() and (e_deal[n:] == NO_ITEM).all(), "padding is only the tail"
    assert (np.diff(s_deal[:n]) <= 0).all(), "shares never increase in dealing order"
    assert (s_deal[n:] == 0).all()
    # coverage: every listed item exactly once, as itself, as its four quarters or by its tile's super fill
    seen, quarters, supers = {}, {}, set()
    for e, s in zip(ent, sh):
        kind, v, q, p = decode(e)
        if kind == "pad":
            continue
        if kind == "item":
            assert v not in seen and want["kind"].get(v) == "item", (kind, v)
            seen[v] = 1
            share = want["share"][v]
        elif kind == "quarter":
            assert want["kind"].get(v) == "quarter" and q not in quarters.setdefault(v, set()), (kind, v, q)
            quarters[v].add(q)
            share = want["share"][v]
        else:
            assert v in want["fill"] and v not in supers, (kind, v)
            supers.add(v)
            share = 0
        assert int(s) == min(65535, share), (kind, v, int(s), share)
        assert p == want["prio"](share), (kind, v, share, p)
    assert all(qs == {0, 1, 2, 3} for qs in quarters.values())
    covered = set(seen) | set(quarters) | {lt * 4 + sub for lt in supers for sub in range(4)}
    assert covered == {int(i) for i in geo} and len(seen) + len(quarters) + 4 * len(supers) == len(geo)
    # flags
    assert bool(out.c.has_dp) == bool(quarters)
    assert bool(out.c.trimmable) == ((not moving) and not want["measuring"])
    assert bool(out.c.final_for_view) == (bool(out.c.trimmable) and set_.trim_rounds == 0)
    assert out.c.view_serial == job.view_serial and out.c.trim_round == 0
    for i in (int(x) for x in geo):
        assert is_dp[i] == (1 if want["kind"][i] == "quarter" else 0)
    return want, quarters


# ---- tests --------------------------------------------------------------------------------------------------------------
def test_entry_code_round_trip(wl):
    """Encode then decode is the identity at the extremes of every field; PQ_NO_ITEM is padding before it is anything else.  The
    library's decode agrees: list_to_device_form maps every kind of code to its local tile (tile = lt for world 1)."""
    for prio in (0, 3):
        for item in (0, 5, (1 << 28) - 1):
            assert decode(with_prio(item, prio)) == ("item", item, None, prio)
        for item, q in itertools.product((0, 5, (1 << 26) - 1), (0, 3)):
            assert decode(with_prio(enc_quarter(item, q), prio)) == ("quarter", item, q, prio)
        for lt in (0, 9, (1 << 24) - 1):
            assert decode(with_prio(enc_super(lt), prio)) == ("super", lt, None, prio)
    assert decode(NO_ITEM) == ("pad", None, None, None)
    # (without the test for padding it would read as a quarter with every other field set: the order of the tests matters)
    assert NO_ITEM >> 31 == 1 and (NO_ITEM >> PRIO_SHIFT) & 3 == 3
    g = ShardGrid(65536, 65536, 4096, 4096, 0, 1, 1 << 24)
    top = (1 << 24) - 1
    codes = np.array([with_prio(top * 4 + 3, 3), with_prio(enc_quarter(top * 4 + 3, 3), 3), with_prio(enc_super(top), 3), 0, enc_quarter(0, 0),
                      enc_super(0), NO_ITEM], np.uint32)
    dev = np.zeros(2 * len(codes), np.uint32)
    assert wl.volym_wl_list_to_device_form(C.byref(g), p32(codes), len(codes), p32(dev)) == 0
    assert (dev[0::2] == codes).all()
    assert dev[1::2].tolist() == [4095 | 4095 << 16] * 3 + [0, 0, 0, 0]


@pytest.mark.parametrize("shape,shard", GRIDS)
def test_build_geometric(wl, shape, shard):
    g = shard_grid(shape, shard)
    geo = geometric(wl, g)
    assert len(set(geo.tolist())) == len(geo) and all(0 <= i < g.n_local * 4 for i in geo)
    inside = [i for i in range(g.n_local * 4) if sub_origin(g, i)[0] < g.W and sub_origin(g, i)[1] < g.H]
    if g.world == 1:
        assert sorted(geo.tolist()) == inside                       # exactly the sub-tiles with a pixel in the frame
        if shape == (40, 24):
            assert len(inside) == 15 < g.n_local * 4                # ragged on both axes
    else:
        assert sorted(geo.tolist()) == list(range(g.n_local * 4))   # a shard keeps the outside sub-tiles (its layout has room for them)
    ring = [max(abs(2 * x0 + 8 - g.W), abs(2 * y0 + 8 - g.H)) // 32 for x0, y0 in (sub_origin(g, int(i)) for i in geo)]
    assert ring == sorted(ring)
    # NULL and a capacity below the list
    n = U32(0)
    small = np.zeros(max(1, len(geo) - 1), np.uint32)
    assert wl.volym_wl_build_geometric(None, p32(small), len(small), C.byref(n)) == E_INVALID
    assert wl.volym_wl_build_geometric(C.byref(g), p32(small), len(geo) - 1, C.byref(n)) == E_INVALID


MODES = {
    "off": dict(set=dict(dp_min_cost=0), job={}, moving=False),
    "all": dict(set=dict(dp_min_cost=1), job={}, moving=False),
    "plain": dict(set={}, job=dict(plain=True), moving=False),
    "lookahead": dict(set={}, job=dict(plain=False), moving=False),
    "continuous": dict(set={}, job=dict(plain=False, continuous=True), moving=False),
    "moving": dict(set={}, job=dict(plain=True), moving=True),
    "measuring": dict(set={}, job=dict(plain=True, captured_has_dp=True), moving=False),
    "no_prio_rounds": dict(set=dict(prio_tenths=(0, 6, 10), trim_rounds=2), job=dict(plain=True), moving=False),
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("waves,max_grid", LAUNCHES)
@pytest.mark.parametrize("shape,shard", GRIDS)
def test_deal_list(wl, shape, shard, waves, max_grid, costs, mode):
    """Coverage, shape, split rule, priorities and flags of one dealt list against the restated rules."""
    g = shard_grid(shape, shard)
    geo = geometric(wl, g)
    cost = make_costs(costs, g, geo)
    m = MODES[mode]
    set_, job = settings(**m["set"]), launch(waves, max_grid, **m["job"])
    # the hysteresis has something to hold: every third item was split before
    was_dp = (np.arange(g.n_local * 4) % 3 == 0).astype(np.uint8)
    out, is_dp = deal(wl, g, set_, job, m["moving"], cost, geo, was_dp)
    want, quarters = check_dealt(g, set_, job, m["moving"], cost, geo, was_dp, out, is_dp)
    listed_cost = {int(i): int(cost[i]) for i in geo}
    if mode == "off" or mode == "measuring":
        assert not quarters and not out.c.has_dp
    if mode == "measuring":
        assert not out.c.trimmable and not out.c.final_for_view
    if mode == "all":
        assert set(quarters) == {i for i, k in listed_cost.items() if k >= 1}
    if mode == "no_prio_rounds":
        assert all(decode(e)[3] == 0 for e in out.entries if e != NO_ITEM)
        assert out.c.trimmable and not out.c.final_for_view
    if mode in ("plain", "lookahead", "continuous"):
        assert out.c.trimmable and out.c.final_for_view
    # priority: none for share 0, never falling as the share grows
    by_share = sorted((int(s), decode(e)[3]) for e, s in zip(out.entries, out.shares) if e != NO_ITEM)
    assert all(p == 0 for s, p in by_share if s == 0)
    assert all(a[1] <= b[1] for a, b in zip(by_share, by_share[1:]))


def test_split_thresholds_tell_the_modes_apart(wl):
    """1.9x / 1.5x / 1.2x a wave's fair share for the common instantiation / the look-ahead ones / the continuous-rho modes, and the
    0.7x hysteresis with the radius-1 dilation while the camera moves: costs placed between the thresholds."""
    g = shard_grid((256, 144), (0, 1))
    geo = geometric(wl, g)
    assert len(geo) == 576
    cost = np.full(576, 100, np.uint16)
    # isolated items (their neighbours stay at 100): fair share = total / 128 ~ 4.7 x 100, thresholds ~ 580 / 720 / 910
    probes = {lt * 4: k for lt, k in zip((21, 50, 83, 110), (600, 750, 900, 1000))}
    for i, k in probes.items():
        cost[i] = k
    got = {}
    for name, kw in (("plain", dict(plain=True)), ("lookahead", dict(plain=False)), ("continuous", dict(plain=False, continuous=True))):
        set_, job = settings(), launch(16, 8, **kw)
        out, is_dp = deal(wl, g, set_, job, False, cost, geo)
        _, quarters = check_dealt(g, set_, job, False, cost, geo, np.zeros(576, np.uint8), out, is_dp)
        got[name] = sorted(cost[i] for i in quarters)
    assert got == {"plain": [1000], "lookahead": [750, 900, 1000], "continuous": [600, 750, 900, 1000]}
    # moving: the common instantiation deals at 1.5x too, costs are dilated by one item, and an item that was split stays split
    # down to 0.7x the threshold.  dilate = 0 isolates the hysteresis; the default (-1) shows the dilation.
    was = np.zeros(576, np.uint8)
    was[[21 * 4, 50 * 4, 7]] = 1                                     # 600 (>= 0.7 x ~720) holds, 100 does not
    set_, job = settings(dilate=0), launch(16, 8, plain=True)
    out, is_dp = deal(wl, g, set_, job, True, cost, geo, was)
    _, quarters = check_dealt(g, set_, job, True, cost, geo, was, out, is_dp)
    assert sorted(cost[i] for i in quarters) == [600, 750, 900, 1000]
    out, is_dp = deal(wl, g, set_, job, False, cost, geo, was)       # standing: no hysteresis
    _, quarters = check_dealt(g, set_, job, False, cost, geo, was, out, is_dp)
    assert sorted(cost[i] for i in quarters) == [1000]
    set_ = settings()
    out, is_dp = deal(wl, g, set_, job, True, cost, geo)
    want, quarters = check_dealt(g, set_, job, True, cost, geo, np.zeros(576, np.uint8), out, is_dp)
    # every probe above the threshold spreads to its 3x3 neighbourhood (none of the probes sits on the frame's edge)
    n_above = sum(1 for k in probes.values() if k >= want["thr"])
    assert n_above >= 1 and len(quarters) == 9 * n_above


def test_list_to_device_form(wl):
    """x | y << 16 of the entry's own 16x16 tile, lt * world + rank, for every kind of entry of dealt lists; padding gives 0."""
    kinds = set()
    for shape, shard in GRIDS:
        g = shard_grid(shape, shard)
        geo = geometric(wl, g)
        for costs, dp in (("heavy", 1), ("three_zero", -1)):
            out, _ = deal(wl, g, settings(dp_min_cost=dp), launch(2, 3), False, make_costs(costs, g, geo), geo)
            ent = out.entries.copy()
            dev = np.zeros(2 * len(ent), np.uint32)
            assert wl.volym_wl_list_to_device_form(C.byref(g), p32(ent), len(ent), p32(dev)) == 0
            assert (dev[0::2] == ent).all()
            for e, xy in zip(ent, dev[1::2]):
                kinds.add(decode(e)[0])
                if e == NO_ITEM:
                    assert xy == 0
                else:
                    tile = local_tile_of(e) * g.world + g.rank
                    assert xy == (tile % g.tiles_x) | (tile // g.tiles_x) << 16
    assert kinds == {"item", "quarter", "super", "pad"}


def test_costs_to_items(wl):
    """Whole entry: k.  Quarters: 5 + the slowest of the four, capped.  Super fill: 0, or max(1, k / 4) for each of its four.  Positions
    at or beyond n_entries, and padding, are ignored."""
    ent = [3, with_prio(6, 2),
           enc_quarter(9, 0), with_prio(enc_quarter(9, 1), 3), enc_quarter(9, 2), enc_quarter(9, 3),
           enc_quarter(10, 0), enc_quarter(10, 1), enc_quarter(10, 2), enc_quarter(10, 3),
           enc_super(3), enc_super(4), with_prio(enc_super(5), 1), NO_ITEM, 1, 2]
    cost = [17, 65535, 40, 41, 39, 2, 65535, 1, 1, 1, 0, 3, 803, 999, 77, 88]
    lst = HostList(entries=ent)
    items = np.full(24, 1234, np.uint16)
    assert wl.volym_wl_costs_to_items(C.byref(lst.c), p16(np.array(cost, np.uint16)), 14, p16(items), len(items)) == 0   # 14: not the last two
    want = np.full(24, 1234, np.int64)
    want[3], want[6], want[9], want[10] = 17, 65535, 5 + 41, 65535
    want[12:16], want[16:20], want[20:24] = 0, 1, 200
    assert items.tolist() == want.tolist()
    assert wl.volym_wl_costs_to_items(None, p16(items), 0, p16(items), len(items)) == E_INVALID


def dealt_for_trim(wl, waves=2, max_grid=4, shape=(64, 32), shard=(0, 1), **kw):
    g = shard_grid(shape, shard)
    geo = geometric(wl, g)
    job = launch(waves, max_grid)
    out, _ = deal(wl, g, settings(**kw), job, False, make_costs("heavy", g, geo), geo)
    job.grid = out.c.grid
    return g, job, out


def times_of(G, waves, dur, start=5000):
    """The captured launch's times: the end tick of every wave (workgroup-major), then the start tick of every workgroup."""
    t = np.zeros(G * (waves + 1), np.uint32)
    for b in range(G):
        t[b * waves:(b + 1) * waves] = start + int(dur[b]) - np.arange(waves)          # the last wave to end sets the duration
    t[G * waves:] = start
    return t


def trim(wl, set_, job, capacity, lst, times):
    out = HostList(max(int(capacity), 1))
    rc = wl.volym_wl_trim_list(C.byref(set_), C.byref(job), int(capacity), C.byref(lst.c), p32(times), C.byref(out.c))
    return rc, out


def columns(lst, G):
    return [[(int(e), int(s)) for e, s in zip(lst.entries[b::G], lst.shares[b::G]) if e != NO_ITEM] for b in range(G)]


@pytest.mark.parametrize("shape,shard", GRIDS)
@pytest.mark.parametrize("rounds", [1, 3])
def test_trim_list(wl, shape, shard, rounds):
    set_ = settings(trim_rounds=rounds, dp_min_cost=1)
    g, job, lst = dealt_for_trim(wl, shape=shape, shard=shard, trim_rounds=rounds, dp_min_cost=1)
    G, cap = lst.c.grid, g.n_local * 16 + 2 * job.max_grid * 8 + 64
    assert lst.c.trimmable and not lst.c.final_for_view and G >= 1
    before = columns(lst, G)
    # equal durations move nothing
    rc, same = trim(wl, set_, job, cap, lst, times_of(G, job.waves, [3000] * G))
    assert rc == 1 and columns(same, G) == before and same.c.grid == G
    assert same.c.trim_round == 1 and bool(same.c.final_for_view) == (rounds <= 1) and same.c.trimmable
    assert same.c.view_serial == lst.c.view_serial and bool(same.c.has_dp) == bool(lst.c.has_dp)
    # workgroup 0 took three times as long as the others: it hands entries over
    dur = [9000] + [3000] * (G - 1)
    rc, out = trim(wl, set_, job, cap, lst, times_of(G, job.waves, dur))
    assert rc == 1 and out.c.grid == G and len(out.entries) % G == 0
    after = columns(out, G)
    assert sorted(x for col in after for x in col) == sorted(x for col in before for x in col), "the multiset of (code, share) is preserved"
    for b in range(G):
        assert [s for _, s in after[b]] == sorted((s for _, s in after[b]), reverse=True), "a column is in order of decreasing share"
        assert {e for e, s in after[b] if s == 0} == {e for e, s in before[b] if s == 0}, "entries of share 0 stay in their column"
        n_b = len(after[b])
        assert (out.entries[b::G][n_b:] == NO_ITEM).all()
    if G > 1:
        assert sum(s for _, s in after[0]) < sum(s for _, s in before[0]) and set(after[0]) < set(before[0])
    # a second round on the result
    job2 = launch(job.waves, job.max_grid, grid=G)
    rc, out2 = trim(wl, set_, job2, cap, out, times_of(G, job.waves, [3000] * G))
    assert rc == 1 and out2.c.trim_round == 2 and bool(out2.c.final_for_view) == (rounds <= 2)
    # refusals: another grid, times that are not a frame's, a result above the capacity
    other = launch(job.waves, job.max_grid, grid=G + 1)
    assert trim(wl, set_, other, cap, lst, times_of(G, job.waves, dur))[0] == 0
    assert trim(wl, set_, job, cap, lst, times_of(G, job.waves, [2000001] * G))[0] == 0
    assert trim(wl, set_, job, len(out.entries) - 1, lst, times_of(G, job.waves, dur))[0] == 0
    assert wl.volym_wl_trim_list(C.byref(set_), C.byref(job), cap, None, p32(times_of(G, job.waves, dur)), C.byref(out.c)) == E_INVALID
