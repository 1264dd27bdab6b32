"""The convolution plans the planner chooses by the CU count, held bit for bit to the operand models (``-m gpu``).

On the full card the bit-exact suite's maps are one round of single 8-row tiles and one tile per block of the first pair
(tests/test_gpu_conv_modes.py).  Under SHF_CONV_CUS -- the CU count the planner cuts work by; it changes launches, never a
result -- the same small maps reach the plans the real workload runs:
  (a) the hybrid cover of the dual-tile family -- a two-tile launch over pixel tiles [0, n2), then a single-tile launch with
      tile_base = n2 -- on 8- and 16-row tiles, split and fp32 input; 16-row tiles picked by w4_pick_mt itself; an all-dual
      cover by cost with an odd tile count (the last block's second tile is the dummy);
  (b) two-tile blocks whose tiles belong to DIFFERENT members of a grouped pass, the members' images a factor 2^6 apart in
      both orders: a tile lifted by its neighbour's activation exponent overflows fp16 on the larger unit or loses its low
      part on the smaller;
  (c) the persistent first pair's walk: 2, 3 and 6 tiles per block, with and without the per-block tile table, and in a
      grouped pass every block walking from the first member into the second;
  (d) the short-K layers: slim under the knob, and with 8-row tiles forced a hybrid of the two-tile and the two-per-CU form.
One child process per knob set (the knobs are read once per process), one after another, once per module; the child runs
the cases and reports the plans the library's probe gives in ITS process, the parent holds the plans to the table
(tests/conv_plan_cases.py GPU_PLANS; tests/test_conv_plans_host.py holds the table to the planner without a GPU) and the
bits to oracle/conv_modes.py, the profiler classes to K.expected_classes, range_fallbacks to 0.  No tolerance anywhere.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import conv_modes as CM
from tests import conv_mode_cases as K
from tests import conv_plan_cases as PL
from tests import helpers as H
from tests import test_gpu_conv_modes as M

pytestmark = pytest.mark.gpu
ROOT = M.ROOT
ALL, TWO = K.GRIDS, ("two",)
S = 2.0 ** -6     # the scale between the images of a group's units
GROUP_MODES = [("f16x3", 0), ("f16x3", 1), ("f16x3", 2), ("f16x2", 0), ("f16", 0), ("bf16", 0)]
PAIR_MODES = [("f16x3", 0), ("f16x2", 0), ("f16", 0), ("bf16", 0)]

# knob set -> (environment, cases (name, h, w, grids, row of PL.GPU_PLANS), grouped passes (case, units, modes, row of GPU_PLANS))
CUS4 = dict(SHF_CONV_CUS="4")
SETS = {
    "cus4": (CUS4,
             [("fam256", 23, 40, ALL, "hybrid8"), ("fam_256_128", 23, 40, ALL, "hybrid8_fp32_in"), ("fam256", 9, 17, ALL, "auto16_single"),
              ("fam256", 33, 40, ALL, "all_dual_odd"), ("slim_128_256", 23, 40, ALL, "slim_128_256"), ("slim_128_256", 9, 17, TWO, None),
              ("slim", 23, 40, ALL, "slim_128_128"), ("slim", 9, 17, TWO, None), ("first", 18, 34, ALL, "walk2_1")],
             [("fam256", [(23, 40, 1.0), (9, 17, S)], GROUP_MODES, "straddle8"), ("fam256", [(23, 40, S), (9, 17, 1.0)], GROUP_MODES, "straddle8"),
              ("fam256", [(9, 17, 1.0), (23, 40, S)], GROUP_MODES, "straddle8_rev"), ("fam256", [(9, 17, S), (23, 40, 1.0)], GROUP_MODES, "straddle8_rev")]),
    "cus4_rows16": (dict(CUS4, SHF_F16X3_W4_MT="4"),
                    [("fam256", 23, 40, ALL, "hybrid16")],
                    [("fam256", [(9, 40, 1.0), (23, 40, S)], GROUP_MODES, "straddle16"), ("fam256", [(9, 40, S), (23, 40, 1.0)], GROUP_MODES, "straddle16")]),
    "cus4_rows8": (dict(CUS4, SHF_F16X3_W4_MT="2"), [("slim", 23, 40, ALL, "short_k_hybrid")], []),
    "cus2": (dict(SHF_CONV_CUS="2"),
             [("first", 18, 34, ALL, "walk3")],
             [("first", [(18, 34, 1.0), (34, 50, S)], PAIR_MODES, "walk_group"), ("first", [(18, 34, S), (34, 50, 1.0)], PAIR_MODES, "walk_group")]),
    "cus1": (dict(SHF_CONV_CUS="1"), [("first", 18, 34, ALL, "walk6")], []),
    "cus4_no_table": (dict(CUS4, SHF_F16X3_PC_TAB="0"), [("first", 18, 34, ALL, "walk2_1")], []),
    "cus2_no_table": (dict(SHF_CONV_CUS="2", SHF_F16X3_PC_TAB="0"), [("first", 18, 34, ALL, "walk3")], []),
    "cus1_no_table": (dict(SHF_CONV_CUS="1", SHF_F16X3_PC_TAB="0"), [("first", 18, 34, ALL, "walk6")], []),
}
CASES = [(s, i) for s in sorted(SETS) for i in range(len(SETS[s][1]))]
GROUPS = [(s, i, m) for s in sorted(SETS) for i in range(len(SETS[s][2])) for m in range(len(SETS[s][2][i][2]))]


def _under(case):
    return [L for L in case["graph"] if L["name"] == case["under"][0]][0]


def _probe_under(case, units):
    """The plan the library gives the case's layer under test over `units` in THIS process (its knobs, its CU count)."""
    from smallhardface_amd import _lib
    L = _under(case)
    first = L["name"] == "c1" and L["cin"] == 64 and L["nout"] == 64 and case["fused"]
    return PL.probe(_lib.load(), [u[:2] for u in units], L["cin"], L["nout"], first_pair=first)


def _group_inputs(units):
    datas = [(K.image("two", h, w, seed=20 + k) * np.float32(s))[None] for k, (h, w, s) in enumerate(units)]
    return datas, [np.array([[h, w, 1]], np.float32) for h, w, _ in units]


def _products(case, mode, products):
    prod = dict(K.products_of(case, mode))
    if products:
        prod[case["under"][0]] = products
    return prod


def run_group(name, units, modes):
    """ONE grouped pass per 32 probed channels over the units (each on its own lane), then each unit as a single forward."""
    case = K.case_of(name)
    gnet, onet = K.make_nets(case, units[0][0], units[0][1], True)
    K.load_grid(case, "two", gnet, onet)
    lanes = [gnet] + [gnet.clone() for _ in units[1:]]
    datas, infos = _group_inputs(units)
    layers = sorted(set(case.get("keep3", [])) | {case["under"][0]})
    arrays, meta = {}, {}
    before = gnet.range_fallbacks
    for mode, products in modes:
        key = "%s/%d" % (mode, products)
        prod = _products(case, mode, products)
        gnet.set_conv_mode(mode)
        gnet.set_layer_products({n: prod.get(n, 0) for n in layers})
        gnet.prof_enable(True)
        gnet.prof_reset()
        grouped = M._read_group(gnet, lanes, onet, datas, infos, case)
        meta[key] = dict(prof=M._prof(gnet), forwards=H.readout_forwards(onet))
        gnet.prof_enable(False)
        for k, (d, i) in enumerate(zip(datas, infos)):
            arrays["%s/grouped/%d" % (key, k)] = grouped[k]
            arrays["%s/single/%d" % (key, k)] = H.read_fused_blob(gnet, onet, d, i, mode=mode)
    gnet.set_layer_products({n: 0 for n in layers})
    gnet.set_conv_mode("f16x3")
    meta["range_fallbacks"] = int(gnet.range_fallbacks - before)
    meta["plan"] = _probe_under(case, units)
    return arrays, meta


def _child(which, out):
    _, cases, groups = SETS[which]
    arrays, meta = {}, {}
    t0 = time.time()
    for i, (name, h, w, grids, _) in enumerate(cases):
        a, m = M.run_case(name, h, w, grids)
        m["plan"] = _probe_under(K.case_of(name), [(h, w)])
        arrays.update({"case%d/%s" % (i, k): v for k, v in a.items()})
        meta["case%d" % i] = m
    for i, (name, units, modes, _) in enumerate(groups):
        a, m = run_group(name, units, modes)
        arrays.update({"group%d/%s" % (i, k): v for k, v in a.items()})
        meta["group%d" % i] = m
    meta["seconds"] = time.time() - t0
    np.savez(out + ".npz", **arrays)
    json.dump(meta, open(out + ".json", "w"))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    res = {}
    for which, (env, _, _) in SETS.items():
        out = str(tmp_path_factory.mktemp(which) / "cases")
        code = "from tests import test_gpu_conv_plans as T; T._child(%r, %r)" % (which, out)
        t0 = time.time()
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (which, r.stderr[-3000:])
        res[which] = (dict(np.load(out + ".npz")), json.load(open(out + ".json")))
        print("child %s: %.1f s, of which cases %.1f s" % (which, time.time() - t0, res[which][1]["seconds"]))
    return res


def _mine(arrays, tag):
    return {k[len(tag) + 1:]: v for k, v in arrays.items() if k.startswith(tag + "/")}


def check_plan(which, row, got, units):
    """The plan the child's library reported is the table's row, launch by launch: what the case claims to run."""
    env = SETS[which][0]
    t_units, cin, cout, cus, first, knobs, want = PL.GPU_PLANS[row]
    assert [tuple(u) for u in t_units] == [tuple(u[:2]) for u in units] and cus == int(env["SHF_CONV_CUS"]), (row, units, env)
    assert knobs.get("w4_mt", 0) == int(env.get("SHF_F16X3_W4_MT", 0))
    p = PL.plan(t_units, cin, cout, cus, first, PL.knobs_of(env))
    assert got["launches"] == p["launches"] and got["pc_tab"] == p["pc_tab"], (row, got, p)
    L = got["launches"]
    assert [q["grid"] for q in L] == want["grids"], (row, L)
    if first:
        assert L[0]["persistent"] == 1 and -(-sum(p["tiles"]) // L[0]["grid"]) == want["tiles_per_block"] > 1, (row, L)
        assert got["pc_tab"] == (0 if env.get("SHF_F16X3_PC_TAB") == "0" else 1)
        return p
    assert (p["mt"], p["tiles"], p["n2"], p["kind"]) == (want["mt"], want["tiles"], want["n2"], want["kind"]), (row, p)
    if want["kind"] == "hybrid":     # two launches, the second from tile_base == n2 on
        assert len(L) == 2 and (L[0]["ntile"], L[0]["tile_base"]) == (2, 0) and (L[1]["ntile"], L[1]["tile_base"]) == (1, want["n2"]), (row, L)
        assert L[0]["rows"] == L[1]["rows"] == 4 * want["mt"]
    if want["kind"] == "all_dual":
        assert len(L) == 1 and L[0]["ntile"] == 2 and sum(p["tiles"]) % 2 == 1     # (an odd count: the last block's second tile is the dummy)
    if "slim" in want:
        assert L[-1]["slim"] == want["slim"], (row, L)
    if row.startswith("straddle") and row != "straddle8_rev":     # pair (t - 1, t) holds one tile of each member
        t = p["tiles"][0]
        assert t % 2 == 1 and t < p["n2"] and PL.member_of(p, t - 1) == 0 and PL.member_of(p, t) == 1
    if row.startswith("straddle"):
        assert PL.member_of(p, p["n2"]) == 1     # the remainder launch works in the second member
    return p


@pytest.mark.parametrize("which,i", CASES, ids=["%s-%s-%dx%d" % ((s,) + SETS[s][1][i][:3]) for s, i in CASES])
def test_plan_under_the_cu_knob_bits_in_every_mode(plans, which, i):
    arrays, meta = plans[which]
    name, h, w, grids, row = SETS[which][1][i]
    m = meta["case%d" % i]
    if row is not None:
        check_plan(which, row, m["plan"], [(h, w)])
    else:     # (the short-K layers at their second size: the slim form, whatever the CU count)
        assert [q["slim"] for q in m["plan"]["launches"]] == [1]
    knobs = dict(plan=dict(cus=int(SETS[which][0]["SHF_CONV_CUS"]), units=[(h, w)], env=SETS[which][0]))
    M.check_case(name, h, w, grids, _mine(arrays, "case%d" % i), m, knobs)


@pytest.mark.parametrize("which,i,mi", GROUPS, ids=["%s-%s-%s-%s-%d" % (s, SETS[s][2][i][0], "+".join("%dx%d@%g" % u for u in SETS[s][2][i][1]),
                                                                      SETS[s][2][i][2][mi][0], SETS[s][2][i][2][mi][1]) for s, i, mi in GROUPS])
def test_grouped_pass_under_the_cu_knob_each_member_equals_its_own_model(plans, which, i, mi):
    """ONE grouped pass over two units whose images are a factor 2^6 apart: every member's probed blob equals the model of
    ITS unit, and so does a single forward of it -- in a plan whose blocks hold tiles of both members (a two-tile block of
    the hybrid cover; a block of the persistent first pair walking from the first member into the second)."""
    arrays, meta = plans[which]
    name, units, modes, row = SETS[which][2][i]
    mode, products = modes[mi]
    case = K.case_of(name)
    m = meta["group%d" % i]
    env = SETS[which][0]
    p = check_plan(which, row, m["plan"], units)
    if PL.GPU_PLANS[row][4]:     # every block of the walk crosses from the first member into the second
        grid = m["plan"]["launches"][0]["grid"]
        assert all({PL.member_of(p, t) for t in range(b, sum(p["tiles"]), grid)} == {0, 1} for b in range(grid))
    assert m["range_fallbacks"] == 0
    key = "%s/%d" % (mode, products)
    mine = _mine(arrays, "group%d/%s" % (i, key))
    params = K.grid_params(case, "two")
    datas, _ = _group_inputs(units)
    prod = _products(case, mode, products)
    U, probe = _under(case), K.probes_of(case)[0]
    exps = []
    for k, ((h, w, _), d) in enumerate(zip(units, datas)):
        blobs = K.model(case, "two", h, w, mode, params=params, data=d[0], products=prod)
        # the scaled unit is as exact as the other: the same sums, six binades lower
        x, (wt, b) = blobs[U["bottom"]], params[U["name"]]
        r = CM.layer_rule(U, case["graph"], mode, True, prod)
        e = CM.act_exponent(np.abs(x).max()) if (r["arith"] == "fam" and not r["bf"]) else 0
        assert CM.exactness(CM.product_groups(x, wt, r["arith"], r["nprod"], r["bf"], e), b) < 24
        # the exponent the next family layer lifts this member's activations by (first pair: its pooled map's, read by the probe)
        exps.append(CM.act_exponent(np.abs(x if r["arith"] == "fam" else blobs[U["name"]]).max()))
        M.bits_equal(mine["grouped/%d" % k], blobs[probe], ("grouped", which, name, units, key, k))
        M.bits_equal(mine["single/%d" % k], blobs[probe], ("single", which, name, units, key, k))
    # the members' activation exponents differ: by the images' six binades, or by what the cap at 15 leaves of them -- four
    # on "fam256" (11 and 15: the larger unit's 6.0 lifted by 15 instead of 11 is 196 608, beyond fp16)
    assert abs(exps[0] - exps[1]) >= 4, exps
    expect = K.expected_classes(case, mode, dict(plan=dict(cus=int(env["SHF_CONV_CUS"]), units=[u[:2] for u in units], env=env)))
    n = m[key]["forwards"]
    prof = m[key]["prof"]
    assert {k: v for k, v in prof.items() if k != K.FIRST} == {k: n * v for k, v in expect.items() if k != K.FIRST}, (prof, expect)
