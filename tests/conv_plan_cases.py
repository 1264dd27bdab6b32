"""The split-fp16 convolution planner's three CU-count decisions, restated in plain Python from the comments and constants
of csrc/conv_f16x3.hip (plan_conv_f16x3, w4_pick_mt) and csrc/conv_lds_layout.h, for a 3x3 / pad 1 / dilation 1 layer over
a group of (1, h, w) units (or (b, h, w): a unit given as (h, w, b)):

  * 16-row or 8-row tiles for the dual-tile family (w4_pick_mt): rounds of `cus` blocks, an 8-row block at 0.56 of a
    16-row one; short K (Cin <= 128) always takes 8-row tiles;
  * the cover: all two-tile blocks, all single-tile blocks, or the hybrid -- a two-tile launch over pixel tiles [0, n2),
    then a single-tile launch with tile_base = n2 over [n2, tiles) -- by the block costs 1.0 / 1.82 (16 rows) and
    0.56 / 1.02 (8 rows) and whole rounds of cus / nct blocks; short K layers take single tiles (the slim form);
  * the persistent first pair: grid = min(tiles, cus), a block walks tile = block, block + grid, ...; its per-block tile
    table holds PC_TABN = 300 tiles and packs images < 256 and tile rows / columns < 1024.

`plan` returns what shf_debug_conv_plan_group reports (tests/test_conv_plans_host.py holds the two to each other on a sweep,
no GPU), and the decisions behind it: mt, the members' tiles, n2, the kind of cover and the three costs.  The knobs are
the environment's (SHF_F16X3_W4_MT, SHF_F16X3_W4D_NTILE, SHF_F16X3_W4_SLIM, SHF_F16X3_PC_TAB, SHF_F16X3_PC_PERSIST) as
{"w4_mt": .., "w4d_ntile": .., "w4_slim": .., "pc_tab": .., "pc_persist": ..}.
"""
import ctypes as C

TW = 16
MAX_GROUP = 16
PC_TABN = 300
COST = {4: (1.0, 1.82), 2: (0.56, 1.02)}     # mt -> cost of a one-tile / two-tile block (unit: a 16-row single-tile block)
# dynamic LDS per launch (conv_lds_layout.h pins these totals)
LDS_W4D = {(16, 2): 160768, (16, 1): 105216, (8, 2): 111616, (8, 1): 80640}
LDS_SLIM, LDS_PC, LDS_W8 = 48768, 161088, {128: 157248, 64: 101952}
FIELDS = ("grid", "lds", "rows", "ntile", "tile_base", "ntile_blocks", "slim", "persistent")
DEFAULT_KNOBS = dict(w4_mt=0, w4d_ntile=0, w4_slim=1, pc_tab=1, pc_persist=1)


def knobs_of(env):
    """The planner's knobs as an environment (a dict of strings) sets them."""
    names = dict(w4_mt="SHF_F16X3_W4_MT", w4d_ntile="SHF_F16X3_W4D_NTILE", w4_slim="SHF_F16X3_W4_SLIM", pc_tab="SHF_F16X3_PC_TAB",
                 pc_persist="SHF_F16X3_PC_PERSIST")
    return {k: int(env.get(v, DEFAULT_KNOBS[k])) for k, v in names.items()}


def _ceil(a, b):
    return (a + b - 1) // b


def _hwb(u):
    """A unit is (h, w) or (h, w, images)."""
    return (u[0], u[1], u[2] if len(u) > 2 else 1)


def member_tiles(units, rows):
    return [b * _ceil(w, TW) * _ceil(h, rows) for h, w, b in map(_hwb, units)]


def pick_mt(units, cin, nct, cus, knobs):
    if knobs["w4_mt"] in (2, 4):
        return knobs["w4_mt"]
    if cin <= 128:
        return 2
    t4, t2 = sum(member_tiles(units, 16)), sum(member_tiles(units, 8))
    c4, c2 = float(_ceil(t4 * nct, cus)), 0.56 * float(_ceil(t2 * nct, cus))
    return 2 if c2 < c4 else 4


def cover_costs(tiles, nct, cus, mt):
    """(per_round, {kind: cost}, n2 of the hybrid)."""
    per_round = max(1, cus // nct)
    pairs = (tiles + 1) // 2
    c1, c2 = COST[mt]
    full2 = pairs // per_round
    rest = max(0, tiles - 2 * full2 * per_round)
    costs = dict(all_single=c1 * _ceil(tiles, per_round), all_dual=c2 * _ceil(pairs, per_round),
                 hybrid=c2 * full2 + c1 * _ceil(rest, per_round))
    return per_round, costs, 2 * full2 * per_round


def _launch(**kw):
    return dict(dict.fromkeys(FIELDS, 0), **kw)


def plan(units, cin, cout, cus, first_pair=False, knobs=None):
    """The plan of a 3x3 / dilation 1 layer cin -> cout over `units` = [(h, w), ..] on `cus` compute units."""
    kn = dict(DEFAULT_KNOBS, **(knobs or {}))
    units = [tuple(u) for u in units]
    assert 1 <= len(units) <= MAX_GROUP and cin % 32 == 0 and cout % 64 == 0 and cus >= 1
    out = dict(cus=cus, pc_tab=0)
    if first_pair:
        assert cin == 64 and cout == 64
        per = member_tiles(units, 16)
        tiles = sum(per)
        out.update(mt=4, tiles=per, kind="first_pair")
        if not kn["pc_persist"]:
            out["launches"] = [_launch(grid=tiles, lds=LDS_PC, rows=16, ntile=1)]
            return out
        grid = min(tiles, cus)
        walk = _ceil(tiles, grid)
        packs = all(b <= 255 and _ceil(w, TW) <= 1023 and _ceil(h, 16) <= 1023 for h, w, b in map(_hwb, units))
        out.update(pc_tab=1 if kn["pc_tab"] and walk <= PC_TABN and packs else 0, tiles_per_block=walk)
        out["launches"] = [_launch(grid=grid, lds=LDS_PC, rows=16, ntile=1, ntile_blocks=tiles, persistent=1)]
        return out
    family = cin >= 64 and cout % 128 == 0
    if not family:     # the 8-wave kernel: 16-row tiles, one block per tile and cout tile
        bn = 64 if cout % 128 else 128
        per = member_tiles(units, 16)
        out.update(mt=4, tiles=per, kind="w8", launches=[_launch(grid=sum(per) * (cout // bn), lds=LDS_W8[bn], rows=16, ntile=1)])
        return out
    nct = cout // 128
    mt = pick_mt(units, cin, nct, cus, kn)
    rows = 4 * mt
    per = member_tiles(units, rows)
    tiles = sum(per)
    per_round, costs, n2_hyb = cover_costs(tiles, nct, cus, mt)
    n2 = 0
    if costs["all_dual"] <= costs["all_single"] and costs["all_dual"] <= costs["hybrid"]:
        n2 = tiles
    elif costs["hybrid"] < costs["all_single"]:
        n2 = n2_hyb
    if cin <= 128 and kn["w4_mt"] == 0:
        n2 = 0
    if kn["w4d_ntile"] == 1:
        n2 = 0
    if kn["w4d_ntile"] == 2:
        n2 = tiles
    slim = mt == 2 and n2 == 0 and kn["w4_slim"] != 0 and cin <= 128
    launches = []
    if n2 > 0:
        launches.append(_launch(grid=_ceil(n2, 2) * nct, lds=LDS_W4D[(rows, 2)], rows=rows, ntile=2, ntile_blocks=n2 * nct))
    if n2 < tiles:
        launches.append(_launch(grid=(tiles - n2) * nct, lds=LDS_SLIM if slim else LDS_W4D[(rows, 1)], rows=rows, ntile=1,
                                tile_base=n2, ntile_blocks=tiles * nct, slim=int(slim)))
    out.update(mt=mt, tiles=per, n2=n2, nct=nct, per_round=per_round, costs=costs, launches=launches,
               kind="all_single" if n2 == 0 else "all_dual" if n2 == tiles else "hybrid")
    return out


def member_of(plan_, tile):
    """The member pixel tile `tile` of the grouped launch belongs to."""
    start = 0
    for i, t in enumerate(plan_["tiles"]):
        start += t
        if tile < start:
            return i
    raise IndexError(tile)


def probe(lib, units, cin, cout, cus=0, in_split=0, pooled=0, first_pair=False):
    """shf_debug_conv_plan_group as {launches: [{field: value}], pc_tab}."""
    fn = lib.shf_debug_conv_plan_group
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.c_int] * 6 + [C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    n = len(units)
    hs, ws, bs = ((C.c_int * n)(*[_hwb(u)[k] for u in units]) for k in range(3))
    out, tab = (C.c_longlong * 16)(), C.c_int(-1)
    nl = fn(n, bs, hs, ws, cin, cout, int(in_split), int(pooled), int(first_pair), cus, out, C.byref(tab))
    assert 1 <= nl <= 2, (nl, lib.shf_last_error())
    return dict(launches=[dict(zip(FIELDS, (int(v) for v in out[8 * i:8 * i + 8]))) for i in range(nl)], pc_tab=int(tab.value))


def device_cus(lib):
    """The CU count the library plans by (SHF_CONV_CUS or the device's), read off a plan: the persistent first pair's
    grid is min(tiles, cus), here with 16 x 255 x 255 tiles."""
    return probe(lib, [(16 * 255, 16 * 255)] * 16, 64, 64, first_pair=True)["launches"][0]["grid"]


# the plans the bit-exact GPU cases (tests/test_gpu_conv_plans.py) run under, one by one: (units, cin, cout, cus, first pair,
# knobs) -> what the plan must be
GPU_PLANS = {
    "hybrid8": ([(23, 40)], 256, 256, 4, False, {}, dict(mt=2, tiles=[9], n2=8, kind="hybrid", grids=[8, 2])),
    "hybrid16": ([(23, 40)], 256, 256, 4, False, dict(w4_mt=4), dict(mt=4, tiles=[6], n2=4, kind="hybrid", grids=[4, 4])),
    "hybrid8_fp32_in": ([(23, 40)], 256, 128, 4, False, {}, dict(mt=2, tiles=[9], n2=8, kind="hybrid", grids=[4, 1])),
    "auto16_single": ([(9, 17)], 256, 256, 4, False, {}, dict(mt=4, tiles=[2], n2=0, kind="all_single", grids=[4])),
    "all_dual_odd": ([(33, 40)], 256, 256, 4, False, {}, dict(mt=2, tiles=[15], n2=15, kind="all_dual", grids=[16])),
    "straddle8": ([(23, 40), (9, 17)], 256, 256, 4, False, {}, dict(mt=2, tiles=[9, 4], n2=12, kind="hybrid", grids=[12, 2])),
    "straddle8_rev": ([(9, 17), (23, 40)], 256, 256, 4, False, {}, dict(mt=2, tiles=[4, 9], n2=12, kind="hybrid", grids=[12, 2])),
    "straddle16": ([(9, 40), (23, 40)], 256, 256, 4, False, dict(w4_mt=4), dict(mt=4, tiles=[3, 6], n2=8, kind="hybrid", grids=[8, 2])),
    "slim_128_256": ([(23, 40)], 128, 256, 4, False, {}, dict(mt=2, tiles=[9], n2=0, kind="all_single", grids=[18], slim=1)),
    "slim_128_128": ([(23, 40)], 128, 128, 4, False, {}, dict(mt=2, tiles=[9], n2=0, kind="all_single", grids=[9], slim=1)),
    "short_k_hybrid": ([(23, 40)], 128, 128, 4, False, dict(w4_mt=2), dict(mt=2, tiles=[9], n2=8, kind="hybrid", grids=[4, 1], slim=0)),
    "walk3": ([(18, 34)], 64, 64, 2, True, {}, dict(tiles=[6], grids=[2], tiles_per_block=3, pc_tab=1)),
    "walk6": ([(18, 34)], 64, 64, 1, True, {}, dict(tiles=[6], grids=[1], tiles_per_block=6, pc_tab=1)),
    "walk2_1": ([(18, 34)], 64, 64, 4, True, {}, dict(tiles=[6], grids=[4], tiles_per_block=2, pc_tab=1)),
    "walk_group": ([(18, 34), (34, 50)], 64, 64, 2, True, {}, dict(tiles=[6, 12], grids=[2], tiles_per_block=9, pc_tab=1)),
}
