"""Every convolution kernel form in every conv mode against its bit-exact operand model (``-m gpu``).

The inputs lie on grids on which every product a mode forms and every partial sum is an fp32 number
(tests/conv_mode_cases.py; the conditions are checked on the CPU in tests/test_conv_mode_models.py), so a layer's output
in a mode is one number, computed in float64 from the mode's operand rule (oracle/conv_modes.py): the kernels must give
it BIT FOR BIT -- no tolerance, no measured band -- in "f16x3", "f16x2", "f16", "bf16" and, on the integer grid, "fp32".
The profile counters must show the kernel form the case is about (a profiler class is a form: the NP / BF instantiations
of a form share its class, and are told apart by the bits), and range_fallbacks stays 0.

Per-layer path: a graph without a tail; the input blob of the layer under test is read back and its bits go into the
model.  Fused path: a mini-detector read out through one-hot predictors (helpers.read_fused_blob), the model chained
through the whole stack.  Family and first-pair forms selected by a knob run in one child process per form (the knobs are read once per
process), one at a time, once per module.  set_layer_products: one layer of an f16x3 net at 1 and 2 products equals that
layer's f16 / f16x2 model, its neighbours stay at three, 0 clears it; also on the fused path and in a grouped pass.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import conv_modes as CM
from tests import conv_mode_cases as K
from tests import conv_plan_cases as PL
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_GRIDS = K.GRIDS


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        print(what, "first mismatch at", i, "got", repr(got[i]), "want", repr(want[i]), "of", int(bad.sum()), "in", bad.size)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(what))


def _prof(gnet):
    return K.conv_classes(gnet.prof_read())


def _plan_is_slim(cin, cout, h, w, in_split, pooled):
    from smallhardface_amd import _lib
    fn = _lib.load().shf_debug_conv_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lds, grid, slim = (C.c_longlong * 2)(), (C.c_longlong * 2)(), (C.c_int * 2)()
    assert fn(cin, cout, h, w, in_split, pooled, lds, grid, slim) == 1
    return int(slim[0])


# ------------------------------------------------------------------------------------------------------------
# the GPU side of a case: every grid x mode -> {key: array}, {key: {class: launches}} (in this process or in a child)
# ------------------------------------------------------------------------------------------------------------
def run_case(name, h, w, grids):
    case = K.case_of(name)
    gnet, onet = K.make_nets(case, h, w, True)
    info = np.array([[h, w, 1]], np.float32)
    arrays, meta = {}, {}
    before = gnet.range_fallbacks
    gnet.prof_enable(True)
    for grid in grids:
        K.load_grid(case, grid, gnet, onet)
        data = K.image(grid, h, w)[None]
        for mode in K.modes_of(grid, case["fused"]):
            key = "%s/%s" % (grid, mode)
            gnet.set_conv_mode(mode)
            gnet.set_layer_products({n: K.products_of(case, mode).get(n, 0) for n in case.get("keep3", [])})
            gnet.prof_reset()
            if case["fused"]:
                got = H.read_fused_blob(gnet, onet, data, info, mode=mode)
                meta[key] = dict(prof=_prof(gnet), forwards=H.readout_forwards(onet))
                for p, a in zip(K.probes_of(case), got if isinstance(got, list) else [got]):
                    arrays["%s/%s" % (key, p)] = a
            else:
                for b, shp in (("data", data.shape), ("im_info", (1, 3))):
                    gnet.blobs[b].reshape(*shp)
                gnet.forward(data=data, im_info=info)
                meta[key] = dict(prof=_prof(gnet), forwards=1)
                for p in ["c0"] + K.probes_of(case):
                    arrays["%s/%s" % (key, p)] = np.array(gnet.blobs[p].data[0])
    gnet.prof_enable(False)
    gnet.set_conv_mode("f16x3")
    meta["range_fallbacks"] = int(gnet.range_fallbacks - before)
    return arrays, meta


def plan_knobs(h, w, env=None, knobs=None):
    """`knobs` for K.expected_classes with the cover of the dilation-1 family layers from the planner's restatement, for
    the CU count this process's library plans by (256 on the full card, where nothing changes) under the knobs of `env`."""
    from smallhardface_amd import _lib
    return dict(knobs or {}, plan=dict(cus=PL.device_cus(_lib.load()), units=[(h, w)], env=dict(env or {})))


def check_case(name, h, w, grids, arrays, meta, knobs=None):
    case = K.case_of(name)
    assert meta["range_fallbacks"] == 0
    if "plan" not in (knobs or {}):
        knobs = plan_knobs(h, w, knobs=knobs)
    for grid in grids:
        params = K.grid_params(case, grid)
        for mode in K.modes_of(grid, case["fused"]):
            key = "%s/%s" % (grid, mode)
            inputs = None
            if not case["fused"]:
                # the first-layer kernel is fp32 FMAs in every mode: c0 is the image taps, exactly; its bits feed the model
                c0 = arrays[key + "/c0"]
                bits_equal(c0, K.model(case, grid, h, w, "fp32", params=params)["c0"], (name, key, "c0"))
                inputs = {"c0": c0}
            want = K.model(case, grid, h, w, mode, inputs=inputs, params=params)
            for p in K.probes_of(case):
                bits_equal(arrays["%s/%s" % (key, p)], want[p], (name, "%dx%d" % (h, w), key, p))
            prof, n = meta[key]["prof"], meta[key]["forwards"]
            expect = K.expected_classes(case, mode, knobs)
            if mode == "fp32":      # (which BN the exact kernels take is theirs: no split-fp16 form ran, one launch per layer)
                f32 = sum(v for k, v in prof.items() if k.startswith("conv_mfma_f32_kernel"))
                assert f32 == sum(v for k, v in expect.items() if k.startswith("conv_mfma_f32_kernel")), prof
                assert not any(k.startswith("conv_mfma_f16x3") for k in prof), prof
            else:
                assert prof == {k: v * n for k, v in expect.items()}, (name, key, prof, expect)


# ------------------------------------------------------------------------------------------------------------
# forms selected by shape, graph and mode, in this process
# ------------------------------------------------------------------------------------------------------------
LAYER = [(n, h, w) for n in K.LAYER_CASES for (h, w) in K.LAYER_CASES[n]["sizes"]]
FUSED = [(n, h, w, g) for n in K.FUSED_CASES for (h, w) in K.FUSED_CASES[n]["sizes"] for g in FUSED_GRIDS]


@pytest.mark.parametrize("name,h,w", LAYER, ids=["%s-%dx%d" % c for c in LAYER])
def test_per_layer_kernel_bits_in_every_mode(name, h, w):
    arrays, meta = run_case(name, h, w, K.GRIDS)
    check_case(name, h, w, K.GRIDS, arrays, meta)
    c = K.LAYER_CASES[name]["graph"][1]
    if name in K.FAMILY_DIL1:      # (the short-K layers' class is shared by the slim and the two-per-CU form: the planner says which)
        assert _plan_is_slim(c["cin"], c["nout"], h, w, 0, 0) == (1 if c["cin"] <= 128 else 0)


@pytest.mark.parametrize("name,h,w,grid", FUSED, ids=["%s-%dx%d-%s" % c for c in FUSED])
def test_fused_path_kernel_bits_in_every_mode(name, h, w, grid):
    arrays, meta = run_case(name, h, w, (grid,))
    check_case(name, h, w, (grid,), arrays, meta)


# ------------------------------------------------------------------------------------------------------------
# forms selected by a knob: one child process per form runs every family (first-pair) case in every mode
# ------------------------------------------------------------------------------------------------------------
FAMILY_CASES = [(n, h, w) for n in K.FAMILY_DIL1 + ("slim", "slim_main_pool", "slim_pool_only", "fam256")
                for (h, w) in K.case_of(n)["sizes"]]
PAIR_CASES = [("first", 18, 34)]
# form -> (environment, what expected_classes makes of it, cases)
FORMS = {
    "rows16_dual": (dict(SHF_F16X3_W4_MT="4", SHF_F16X3_W4D_NTILE="2"), dict(mt=4, nt=2), FAMILY_CASES),
    "rows16_single": (dict(SHF_F16X3_W4_MT="4", SHF_F16X3_W4D_NTILE="1"), dict(mt=4, nt=1), FAMILY_CASES),
    "rows8_dual": (dict(SHF_F16X3_W4_MT="2", SHF_F16X3_W4D_NTILE="2"), dict(mt=2, nt=2), FAMILY_CASES),
    "rows8_two_per_cu": (dict(SHF_F16X3_W4_SLIM="0"), dict(mt=2, nt=1), FAMILY_CASES),
    # the fused first pair with one tile per block, and the persistent walk without its tile table
    "pair_tile_per_block": (dict(SHF_F16X3_PC_PERSIST="0"), dict(pc=K.PC), PAIR_CASES),
    "pair_no_tile_table": (dict(SHF_F16X3_PC_TAB="0"), dict(), PAIR_CASES),
}
FORM_CASES = [(f, n, h, w) for f in sorted(FORMS) for (n, h, w) in FORMS[f][2]]


def _child(form, out):
    arrays, meta = {}, {}
    for name, h, w in FORMS[form][2]:
        a, m = run_case(name, h, w, FUSED_GRIDS)
        tag = "%s-%dx%d" % (name, h, w)
        arrays.update({"%s/%s" % (tag, k): v for k, v in a.items()})
        meta[tag] = m
    c = K.LAYER_CASES["slim_64_128"]["graph"][1]
    meta["slim"] = _plan_is_slim(c["cin"], c["nout"], 9, 17, 0, 0)
    np.savez(out + ".npz", **arrays)
    json.dump(meta, open(out + ".json", "w"))


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    res = {}
    for form, (env, _, _) in FORMS.items():
        out = str(tmp_path_factory.mktemp(form) / "cases")
        code = "from tests import test_gpu_conv_modes as M; M._child(%r, %r)" % (form, out)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env), cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (form, r.stderr[-3000:])
        res[form] = (dict(np.load(out + ".npz")), json.load(open(out + ".json")))
    return res


@pytest.mark.parametrize("form,name,h,w", FORM_CASES, ids=["%s-%s-%dx%d" % c for c in FORM_CASES])
def test_knob_selected_form_bits_in_every_mode(forms, form, name, h, w):
    arrays, meta = forms[form]
    tag = "%s-%dx%d" % (name, h, w)
    mine = {k[len(tag) + 1:]: v for k, v in arrays.items() if k.startswith(tag + "/")}
    check_case(name, h, w, FUSED_GRIDS, mine, meta[tag], plan_knobs(h, w, FORMS[form][0], FORMS[form][1]))
    if "pair" not in form:
        assert meta["slim"] == 0      # (none of the four family forms is the slim one, whose class the two-per-CU form shares)


# ------------------------------------------------------------------------------------------------------------
# set_layer_products
# ------------------------------------------------------------------------------------------------------------
OVERRIDE = K.OVERRIDE_CASE


def test_set_layer_products_on_the_per_layer_path():
    """c0 -> c1 (a copy, slim) -> c2 (under test, slim) -> c3 (a copy, 8-wave) in f16x3: c2 at 1 / 2 products equals its
    f16 / f16x2 model on its input's bits while c1 and c3 equal their three-product models (a copy with fewer products
    loses the low parts: it would show); 0 clears the override."""
    h, w = 23, 40
    gnet, onet = K.make_nets(OVERRIDE, h, w, True)
    params = K.load_grid(OVERRIDE, "two", gnet, onet)
    data, info = K.image("two", h, w)[None], np.array([[h, w, 1]], np.float32)
    gnet.set_conv_mode("f16x3")
    seen = {}
    for n in (1, 2, 3, 0):
        gnet.set_layer_products({"c2": n})
        for b, shp in (("data", data.shape), ("im_info", (1, 3))):
            gnet.blobs[b].reshape(*shp)
        gnet.forward(data=data, im_info=info)
        got = {b: np.array(gnet.blobs[b].data[0]) for b in ("c0", "c1", "c2", "c3")}
        for name, bottom in (("c1", "c0"), ("c2", "c1"), ("c3", "c2")):
            want = K.model(OVERRIDE, "two", h, w, "f16x3", inputs={bottom: got[bottom]}, params=params,
                           products={"c2": n} if n else {})[name]
            bits_equal(got[name], want, ("products", n, name))
        seen[n] = got["c2"]
    for a, b in ((1, 2), (2, 3)):
        assert np.mean(seen[a].view(np.uint32) != seen[b].view(np.uint32)) > 0.25
    bits_equal(seen[0], seen[3], "0 clears the override")
    assert gnet.range_fallbacks == 0


def _read_group(head, members, onet, datas, infos, case=None):
    """One grouped pass per 32 channels of the case's probed blob (a single-blob tail; default: the 128 channels of "slim")."""
    channels = 128 if case is None else [L for L in case["graph"] if L["name"] == case["probe"]][0]["nout"]
    outs = [None] * len(members)
    for m, d, i in zip(members, datas, infos):
        m.blobs['data'].reshape(*d.shape)
        m.blobs['im_info'].reshape(*i.shape)
    for c0 in range(0, channels, 32):
        H.readout_set_predictors(head, onet, c0)
        head.forward_group(members, [dict(data=d, im_info=i) for d, i in zip(datas, infos)])
        for k, m in enumerate(members):
            outs[k] = H.readout_take(m, onet, outs[k], c0)
    return [o[0] for o in outs]


@pytest.mark.parametrize("mode,products", [("f16x3", 0), ("f16x3", 1), ("f16x3", 2), ("f16x2", 0), ("f16", 0), ("bf16", 0)])
def test_grouped_pass_each_member_equals_its_own_model(mode, products):
    """ONE grouped pass over two units of different sizes (9x17, 23x40) and activation exponents (the second unit's image
    is scaled by 2^-3), slim kernel with split input: each member's blob equals the model of ITS unit, and so does a
    single forward of it; with set_layer_products on the layer under test the override reaches the fused path and the
    grouped pass."""
    case = K.FUSED_CASES["slim"]
    gnet, onet = K.make_nets(case, 9, 17, True)
    params = K.load_grid(case, "two", gnet, onet)
    lane = gnet.clone()
    units = [(9, 17, 1.0), (23, 40, 2.0 ** -3)]
    datas = [(K.image("two", h, w, seed=20 + k) * np.float32(s))[None] for k, (h, w, s) in enumerate(units)]
    infos = [np.array([[h, w, 1]], np.float32) for h, w, _ in units]
    prod = {"c2": products} if products else {}
    gnet.set_conv_mode(mode)
    gnet.set_layer_products({"c2": products})
    before = gnet.range_fallbacks
    gnet.prof_enable(True)
    gnet.prof_reset()
    grouped = _read_group(gnet, [gnet, lane], onet, datas, infos)
    prof = _prof(gnet)
    gnet.prof_enable(False)
    expect = K.expected_classes(case, mode)
    assert {k: v for k, v in prof.items() if k != K.FIRST} == {k: 4 * v for k, v in expect.items() if k != K.FIRST}, prof   # one grid per layer
    wants = []
    for (h, w, _), d, got in zip(units, datas, grouped):
        blobs = K.model(case, "two", h, w, mode, params=params, data=d[0], products=prod)
        # (the scaled unit is as exact as the first: the same sums, three binades lower)
        x, (wt, b) = blobs["c1"], params["c2"]
        r = CM.layer_rule(case["graph"][2], case["graph"], mode, True, prod)
        e = CM.act_exponent(np.abs(x).max()) if not r["bf"] else 0
        assert CM.exactness(CM.product_groups(x, wt, r["arith"], r["nprod"], r["bf"], e), b) < 24
        bits_equal(got, blobs["c2"], ("grouped", mode, products, h, w))
        wants.append(blobs["c2"])
    assert CM.act_exponent(np.abs(datas[0]).max()) != CM.act_exponent(np.abs(datas[1]).max())
    for (h, w, _), d, i, want in zip(units, datas, infos, wants):
        single = H.read_fused_blob(gnet, onet, d, i, mode=mode)
        bits_equal(single, want, ("single", mode, products, h, w))
    gnet.set_layer_products({"c2": 0})
    gnet.set_conv_mode("f16x3")
    assert gnet.range_fallbacks == before
