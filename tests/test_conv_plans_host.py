"""The split-fp16 planner's CU-count decisions (16- or 8-row tiles, the dual-tile cover, the persistent first pair's grid)
against their plain-Python restatement (tests/conv_plan_cases.py), through shf_debug_conv_plan_group: no GPU, nothing is
launched.  The probe's `cus` argument sweeps CU counts in one process; the tile-row knob, read once per process, is swept in
child processes.  Also here: the plans tests/test_gpu_conv_plans.py runs bit-exact cases under, asserted one by one.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from smallhardface_amd import _lib
from tests import conv_plan_cases as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = ((64, 128), (128, 128), (128, 256), (256, 128), (256, 256), (512, 512))
HEIGHTS = (1, 8, 9, 16, 17, 23, 33, 64, 100, 384)
WIDTHS = (1, 16, 17, 40, 64, 200, 704)
CUS = (1, 2, 3, 4, 6, 32, 64, 128, 256, 304)
GROUPS = ([(23, 40), (9, 17)], [(9, 40), (23, 40)], [(18, 34), (34, 50)], [(9, 17), (23, 40), (33, 40)], [(100, 200), (8, 16), (17, 17)],
          [(384, 704), (64, 64)])


def _lib_or_skip():
    return _lib.load(require_gpu=False)


def check_plan(lib, units, cin, cout, cus, knobs, first_pair=False, probe_cus=None):
    """One plan: the probe equals the restatement, its launches partition [0, tiles), the cover is the cheapest."""
    want = PL.plan(units, cin, cout, cus, first_pair, knobs)
    got = PL.probe(lib, units, cin, cout, cus if probe_cus is None else probe_cus, first_pair=first_pair)
    what = (units, cin, cout, cus, first_pair)
    assert got["launches"] == want["launches"], (what, got, want)
    assert got["pc_tab"] == want["pc_tab"], (what, got, want)
    L = got["launches"]
    tiles = sum(PL.member_tiles(units, L[0]["rows"]))     # (counted from the tile rows the PROBE reports)
    if first_pair:
        assert len(L) == 1
        if knobs["pc_persist"]:
            assert L[0]["persistent"] == 1 and L[0]["grid"] == min(tiles, cus) and L[0]["ntile_blocks"] == tiles, (what, L)
            over = -(-tiles // L[0]["grid"]) > PL.PC_TABN or any(
                b > 255 or -(-w // 16) > 1023 or -(-h // 16) > 1023 for h, w, b in map(PL._hwb, units))
            assert got["pc_tab"] == (0 if over or not knobs["pc_tab"] else 1), (what, got)
        return want
    if want["kind"] == "w8":
        return want
    nct = cout // 128
    n2 = L[0]["ntile_blocks"] // nct if L[0]["ntile"] == 2 else 0
    if n2:     # the two-tile launch covers [0, n2)
        assert L[0]["tile_base"] == 0 and L[0]["grid"] == -(-n2 // 2) * nct and L[0]["ntile_blocks"] == n2 * nct, (what, L)
    if n2 < tiles:     # the single-tile launch covers [n2, tiles)
        S = L[-1]
        assert S["ntile"] == 1 and S["tile_base"] == n2 and S["grid"] == (tiles - n2) * nct and S["ntile_blocks"] == tiles * nct, (what, L)
    assert len(L) == (n2 > 0) + (n2 < tiles) and n2 == want["n2"], (what, L)
    if 0 < n2 < tiles:
        assert n2 % 2 == 0 and want["kind"] == "hybrid", (what, L)
    forced = knobs["w4d_ntile"] in (1, 2) or (cin <= 128 and knobs["w4_mt"] == 0)
    if not forced:
        assert want["costs"][want["kind"]] == min(want["costs"].values()), (what, want)
    return want


def sweep(lib, knobs, cus_list, groups=True):
    """Every plan of the sweep; returns (plans checked, kinds met)."""
    n, kinds = 0, set()
    for cin, cout in CHANNELS:
        for cus in cus_list:
            unit_lists = [[(h, w)] for h in HEIGHTS for w in WIDTHS]
            if groups:
                unit_lists += [g for u in GROUPS for g in (u, u[::-1])]
            for units in unit_lists:
                p = check_plan(lib, units, cin, cout, cus, knobs)
                kinds.add((p["kind"], p["mt"]))
                n += 1
    if knobs["w4_mt"] == 0:
        for cus in cus_list:
            for units in [[(h, w)] for h in HEIGHTS for w in WIDTHS] + [g for u in GROUPS for g in (u, u[::-1])]:
                check_plan(lib, units, 64, 64, cus, knobs, first_pair=True)
                n += 1
    return n, kinds


def _child(cus_list):
    """In a child process under a knob environment: the sweep, its result as one JSON line."""
    n, kinds = sweep(_lib_or_skip(), PL.knobs_of(os.environ), cus_list)
    print(json.dumps(dict(plans=n, kinds=sorted(kinds))))


def test_probe_equals_the_restatement_on_the_sweep():
    lib = _lib_or_skip()
    n, kinds = sweep(lib, PL.knobs_of(os.environ), CUS)
    print("plans", n, "kinds", sorted(kinds))
    assert n >= 6 * 10 * 7 * 10
    if PL.knobs_of(os.environ) == PL.DEFAULT_KNOBS:     # every branch of the cover at both tile heights is in the sweep
        assert {("all_single", 2), ("all_dual", 2), ("hybrid", 2), ("all_single", 4), ("all_dual", 4), ("hybrid", 4)} <= kinds, kinds


@pytest.mark.parametrize("mt", [2, 4])
def test_probe_equals_the_restatement_with_forced_tile_rows(mt):
    code = "from tests import test_conv_plans_host as M; M._child((2, 4, 6))"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, SHF_F16X3_W4_MT=str(mt)), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["plans"] >= 6 * 10 * 7 * 3 and {k[1] for k in res["kinds"]} == {mt}, res


def test_unset_knob_plans_for_the_device():
    """cus = 0: the knob's or the device's count (256 without a device), and the one-unit probe of before agrees launch by launch."""
    lib = _lib_or_skip()
    knobs = PL.knobs_of(os.environ)
    cus = PL.device_cus(lib)
    env = int(os.environ.get("SHF_CONV_CUS", "0") or 0)
    if env >= 1:
        assert cus == env
    elif lib.shf_device_count() <= 0:
        assert cus == 256
    else:
        assert cus >= 4
    old = lib.shf_debug_conv_plan
    old.restype = C.c_int
    old.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    for cin, cout in CHANNELS:
        for h in HEIGHTS:
            for w in WIDTHS:
                want = check_plan(lib, [(h, w)], cin, cout, cus, knobs, probe_cus=0)
                lds, grid, slim = (C.c_longlong * 2)(), (C.c_longlong * 2)(), (C.c_int * 2)()
                nl = old(cin, cout, h, w, 0, 0, lds, grid, slim)
                assert nl == len(want["launches"])
                assert [(grid[i], lds[i], slim[i]) for i in range(nl)] == [(L["grid"], L["lds"], L["slim"]) for L in want["launches"]]


def test_first_pair_table_flag_at_its_limits():
    """The per-block tile table is off exactly when a block would walk more than 300 tiles, or an image count, a tile
    row or a tile column does not pack (B <= 255, <= 1023 rows / columns)."""
    lib = _lib_or_skip()
    knobs = PL.knobs_of(os.environ)
    flags = {}
    for name, units, cus in (("walk300", [(16 * 30, 16 * 10)], 1), ("walk301", [(16 * 43, 16 * 7)], 1), ("walk301_of_2", [(16 * 43, 16 * 14)], 2),
                             ("b255", [(16, 16, 255)], 256), ("b256", [(16, 16, 256)], 256), ("b256_second", [(16, 16), (16, 16, 256)], 256),
                             ("cols1023", [(16, 16 * 1023)], 256), ("cols1024", [(16, 16 * 1023 + 1)], 256),
                             ("rows1023", [(16 * 1023, 16)], 256), ("rows1024", [(16 * 1023 + 1, 16)], 256)):
        flags[name] = check_plan(lib, units, 64, 64, cus, knobs, first_pair=True)["pc_tab"]
    if knobs["pc_tab"] and knobs["pc_persist"]:
        assert flags == dict(walk300=1, walk301=0, walk301_of_2=0, b255=1, b256=0, b256_second=0, cols1023=1, cols1024=0, rows1023=1,
                             rows1024=0), flags


TABLE = PL.GPU_PLANS


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_plans_of_the_gpu_cases(name):
    units, cin, cout, cus, first, knobs, want = TABLE[name]
    p = PL.plan(units, cin, cout, cus, first, knobs)
    got = dict(want, grids=[L["grid"] for L in p["launches"]])
    for k in want:
        if k == "slim":
            got[k] = p["launches"][-1]["slim"]
        elif k != "grids":
            got[k] = p[k]
    assert got == want, (name, p)
    if first:     # a block walks tile = block, block + grid, ...: more than one tile, and in a group from member to member
        grid = p["launches"][0]["grid"]
        assert want["tiles_per_block"] > 1
        if len(units) > 1:
            assert all({PL.member_of(p, t) for t in range(b, sum(p["tiles"]), grid)} == {0, 1} for b in range(grid))
    if name.startswith("straddle"):
        t = p["tiles"][0]
        assert t < p["n2"] and PL.member_of(p, p["n2"]) == 1     # the remainder launch works in the second member
        if name != "straddle8_rev":     # a pair of the two-tile launch holds one tile of each member
            assert t % 2 == 1 and PL.member_of(p, t - 1) == 0 and PL.member_of(p, t) == 1
        else:     # (4 + 9 tiles: the members meet between two pairs -- the same units with the exponents the other way round)
            assert t % 2 == 0
    if not knobs and PL.knobs_of(os.environ) == PL.DEFAULT_KNOBS:     # (knob-free rows: the real planner in this process too)
        assert PL.probe(_lib_or_skip(), units, cin, cout, cus, first_pair=first)["launches"] == p["launches"]
