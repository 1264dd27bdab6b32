"""The conv-mode models and grids on the CPU (oracle/conv_modes.py, tests/conv_mode_cases.py): what the bit-exact GPU
comparison of tests/test_gpu_conv_modes.py rests on.

  * every case's inputs are EXACT: per accumulator, sum |a| |w| over the products a mode forms is below 2^24 quanta, so
    every partial sum in any order is an fp32 number (and a float32 accumulation of the terms in random orders gives the
    model's value);
  * the models are told apart by the case's own data: neighbouring models -- 3 / 2 products, 2 / 1, fp16 / bf16, nearest
    even / truncation, both lanes of a packed conversion / the odd one replaced by the even one -- differ in at least a
    quarter of the probed elements;
  * a deliberately wrong model (a product too few or too many, truncation, the odd bf16 lane lost, one tap shifted in the
    last column) never equals the right one: the comparison would fail;
  * the vectorised model equals a plain loop over taps and channels on tiny layers;
  * the read-out of the fused-path graphs through one-hot predictors is an exact copy (the oracle net forwarded).
"""
import numpy as np
import pytest

from oracle import conv_modes as CM
from tests import conv_mode_cases as K
from tests import helpers as H

ALL = [(n, h, w) for n in list(K.LAYER_CASES) + list(K.FUSED_CASES) for (h, w) in K.case_of(n)["sizes"]]
IDS = ["%s-%dx%d" % c for c in ALL]
_MODELS = {}


def _model(name, grid, h, w, mode, wrong=None, products=None):
    key = (name, grid, h, w, mode, wrong, None if products is None else tuple(sorted(products.items())))
    if key not in _MODELS:
        case = K.case_of(name)
        layer = case["under"][0] if wrong else None
        if wrong in ("trunc", "odd_lane") and grid == "around":
            layer = K.conversion_layer(case, mode)
        _MODELS[key] = K.model(case, grid, h, w, mode, wrong=wrong, wrong_layer=layer, products=products)
        if wrong and layer == case["under"][0] and len(case["under"]) > 1:      # (the shared-weight heads: the same wrong model in all three)
            blobs = dict(_MODELS[key])
            for u in case["under"][1:]:
                blobs[u] = K.model(case, grid, h, w, mode, wrong=wrong, wrong_layer=u, products=products)[u]
            _MODELS[key] = blobs
    return _MODELS[key]


def _differ(name, h, w, a, b):
    """Fraction of the probed elements in which two models' blobs differ (the smallest over the probes)."""
    return min(float(np.mean(a[p].view(np.uint32) != b[p].view(np.uint32))) for p in K.probes_of(K.case_of(name)))


@pytest.mark.parametrize("name,h,w", ALL, ids=IDS)
def test_case_inputs_are_exact_in_every_mode(name, h, w):
    case = K.case_of(name)
    rng = np.random.default_rng(1)
    for grid in K.GRIDS:
        params = K.grid_params(case, grid)
        for mode in K.modes_of(grid, case["fused"]):
            prod = K.products_of(case, mode)
            blobs = K.model(case, grid, h, w, mode, params=params)
            for L in case["graph"]:
                if L["op"] != "conv" or L["bottom"] == "data":
                    continue
                r = CM.layer_rule(L, case["graph"], mode, case["fused"] and mode != "fp32", prod)
                x = blobs[L["bottom"]]
                wt, b = params[L.get("shared_as", L["name"])]
                e = CM.act_exponent(np.abs(x).max()) if r["arith"] == "fam" and not r["bf"] else 0
                groups = CM.product_groups(x, wt, r["arith"], r["nprod"], r["bf"], e)
                bits = CM.exactness(groups, b, L["dil"])      # (asserts that every accumulator and the output are fp32 numbers)
                if L["name"] not in case["under"]:
                    # a one-hot copy: one non-zero term per product, nothing to reorder but hi + lo, an fp32 number (above)
                    assert all(np.count_nonzero(wt[co]) == 1 for co in range(L["nout"]))
                    continue
                assert bits < 24, (grid, mode, L["name"], bits)
                # the activation exponent is a lift by an exact power of two: the value does not depend on it
                if r["arith"] == "fam" and not r["bf"]:
                    for e2 in ((0,) if grid == "two" else ()):
                        again = CM.conv_model(x, wt, b, "fam", r["nprod"], False, L["dil"], L["relu"], e2)
                        np.testing.assert_array_equal(again, blobs[L["name"]])
                # a float32 accumulation of the terms, in random orders, gives the model's value
                for _ in range(3):
                    co, y, xx = int(rng.integers(L["nout"])), int(rng.integers(x.shape[1])), int(rng.integers(x.shape[2]))
                    v, terms = CM.conv_scalar(x, wt, b, r["arith"], r["nprod"], r["bf"], L["dil"], L["relu"], e, co, y, xx, groups)
                    assert v == blobs[L["name"]][co, y, xx]
                    for _ in range(2):
                        tot = np.float32(0)
                        for scale, ts in terms:
                            acc = np.float32(0)
                            for t in rng.permutation(np.asarray(ts, np.float32)):
                                acc = np.float32(acc + t)
                            tot = np.float32(tot + np.float32(acc * np.float32(scale)))
                        tot = np.float32(tot + b[co])
                        assert (max(tot, np.float32(0)) if L["relu"] else tot) == v, (grid, mode, L["name"])


@pytest.mark.parametrize("name,h,w", ALL, ids=IDS)
def test_neighbouring_models_differ_in_a_quarter_of_the_elements(name, h, w):
    frac = {}
    m = lambda *a, **k: _model(name, *a, **k)
    frac["3 vs 2 products"] = _differ(name, h, w, m("two", h, w, "f16x3"), m("two", h, w, "f16x3", "fewer"))
    frac["2 vs 1 products"] = _differ(name, h, w, m("two", h, w, "f16x2"), m("two", h, w, "f16x2", "fewer"))
    frac["fp16 vs bf16"] = _differ(name, h, w, m("around", h, w, "f16"), m("around", h, w, "bf16"))
    frac["fp16 vs bf16 weights"] = _differ(name, h, w, m("wround", h, w, "f16"), m("wround", h, w, "bf16"))
    for grid in ("around", "wround"):
        for mode in ("f16", "bf16"):
            frac["%s %s nearest even vs truncation" % (grid, mode)] = _differ(name, h, w, m(grid, h, w, mode), m(grid, h, w, mode, "trunc"))
    frac["bf16 both lanes vs odd from even"] = _differ(name, h, w, m("around", h, w, "bf16"), m("around", h, w, "bf16", "odd_lane"))
    print(name, h, w, {k: round(v, 3) for k, v in frac.items()})
    for k, v in frac.items():
        assert v >= 0.25, (k, v)


WRONG = [("two", "f16x3", "fewer"), ("two", "f16x2", "fewer"), ("two", "f16x2", "more"), ("two", "f16", "more"),
         ("around", "f16", "trunc"), ("around", "f16x2", "trunc"), ("around", "bf16", "trunc"), ("wround", "f16", "trunc"),
         ("wround", "bf16", "trunc"), ("around", "bf16", "odd_lane"), ("two", "f16x3", "edge"), ("two", "f16", "edge"),
         ("int", "f16x2", "edge"), ("int", "bf16", "edge")]


@pytest.mark.parametrize("name,h,w", ALL, ids=IDS)
def test_a_wrong_model_would_fail_the_comparison(name, h, w):
    case = K.case_of(name)
    for grid, mode, wrong in WRONG + [("int", "fp32", "edge")]:
        if mode == "fp32" and case["fused"]:
            continue
        right, bad = _model(name, grid, h, w, mode), _model(name, grid, h, w, mode, wrong)
        assert any(not np.array_equal(right[p].view(np.uint32), bad[p].view(np.uint32)) for p in K.probes_of(case)), (grid, mode, wrong)


def test_layer_products_override_case():
    """The set_layer_products case: exact at 1, 2 and 3 products of the layer under test, the three told apart in a
    quarter of its elements, and visible behind the copy that follows it."""
    case, (h, w) = K.OVERRIDE_CASE, K.OVERRIDE_CASE["sizes"][0]
    params = K.grid_params(case, "two")
    out = {}
    for n in (1, 2, 3):
        blobs = K.model(case, "two", h, w, "f16x3", params=params, products={"c2": n})
        x, (wt, b) = blobs["c1"], params["c2"]
        np.testing.assert_array_equal(x, blobs["c0"][np.arange(128) % 64])          # the copy kept the low parts
        groups = CM.product_groups(x, wt, "fam", n, False, CM.act_exponent(np.abs(x).max()))
        assert CM.exactness(groups, b) < 24
        out[n] = blobs
    for a, b in ((1, 2), (2, 3)):
        for name in ("c2", "c3"):
            assert np.mean(out[a][name].view(np.uint32) != out[b][name].view(np.uint32)) >= 0.25
    fewer = K.model(case, "two", h, w, "f16x3", params=params, products={"c1": 2})
    assert not np.array_equal(fewer["c1"], out[3]["c1"])


@pytest.mark.parametrize("arith,nprod,bf", [("fp32", 0, False), ("w8", 3, False), ("w8", 2, False), ("w8", 1, False), ("w8", 1, True),
                                            ("fam", 3, False), ("fam", 2, False), ("fam", 1, False), ("fam", 1, True)])
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 2), (1, 1)])
def test_model_equals_a_plain_loop_on_tiny_layers(arith, nprod, bf, k, dil):
    rng = np.random.default_rng(k * 10 + dil)
    for grid in ("two", "around"):
        a = np.maximum(K._two_part(rng, (8, 5, 6)) if grid == "two" else K._around(rng, (8, 5, 6)), 0)
        wt, b = K.test_weights(grid, 6, 8, k, 3)
        e = CM.act_exponent(np.abs(a).max()) if arith == "fam" and not bf else 0
        for relu in (True, False):
            full = CM.conv_model(a, wt, b, arith, nprod, bf, dil, relu, e)
            for co in range(6):
                for y in range(5):
                    for x in range(6):
                        assert CM.conv_scalar(a, wt, b, arith, nprod, bf, dil, relu, e, co, y, x)[0] == full[co, y, x]


def test_conversions():
    x = np.float32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, -(1 + 2.0 ** -11), 65520.0, 2.0 ** -25])
    np.testing.assert_array_equal(CM.f16(x), [1, 1 + 2.0 ** -9, 1 + 2.0 ** -10, -1, np.inf, 0])        # ties to even
    np.testing.assert_array_equal(CM.f16(x, trunc=True)[:4], [1, 1 + 2.0 ** -10, 1, -1])
    y = np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 3.0e38])
    np.testing.assert_array_equal(CM.bf16(y)[:3], [1, 1 + 2.0 ** -6, 1 + 2.0 ** -7])
    np.testing.assert_array_equal(CM.bf16(y, trunc=True)[:3], [1, 1 + 2.0 ** -7, 1])
    assert np.isfinite(CM.bf16(y)[3])
    hi, lo = CM.split_hi_lo(np.float32([6 + 3 * 2.0 ** -12, 0.1]))
    assert hi[0] == 6 and lo[0] == 1.5 and abs(hi[1] + lo[1] / 2048 - np.float32(0.1)) < 2.0 ** -24
    assert CM.act_exponent(6.0) == 11 and CM.act_exponent(0.0) == 0 and CM.act_exponent(2.0 ** -20) == 15 and CM.act_exponent(3e4) == 0
    assert CM.weight_lift_exponent(np.float32([6.0])) == 0 and CM.weight_lift_exponent(np.float32([0.3])) == 4
    pooled = CM.max_pool_2x2(np.arange(15, dtype=np.float64).reshape(1, 3, 5))
    np.testing.assert_array_equal(pooled[0], [[6, 8, 9], [11, 13, 14]])


@pytest.mark.parametrize("name", sorted(K.FUSED_CASES))
def test_fused_graph_readout_is_an_exact_copy(name):
    """The oracle net of every fused-path graph, forwarded through the one-hot predictors (helpers.read_fused_blob without a
    GPU net): the read-out returns the probed blobs bit for bit; and the oracle's fp32 convolutions, exact on the integer
    grid, agree with the fp32 model."""
    case = K.FUSED_CASES[name]
    h, w = case["sizes"][0]
    _, onet = K.make_nets(case, h, w, False)
    K.load_grid(case, "int", None, onet)
    data, info = K.image("int", h, w)[None], np.array([[h, w, 1]], np.float32)
    got = H.read_fused_blob(None, onet, data, info)
    got = got if isinstance(got, list) else [got]
    want = K.model(dict(case, fused=False), "int", h, w, "fp32")
    for p, g in zip(K.probes_of(case), got):
        np.testing.assert_array_equal(g, onet.blobs[p].data[0])
        np.testing.assert_array_equal(g, want[p])


def test_expected_kernel_forms():
    """The table of forms the GPU tests look for in the profile counters, at a few known points."""
    e = K.expected_classes
    assert e(K.LAYER_CASES["slim_64_128"], "f16") == {K.FIRST: 1, K.W4(False, 2, 1): 1}
    assert e(K.LAYER_CASES["k1_256_256"], "bf16") == {K.FIRST: 1, K.W8(128, 1, 1): 1}
    assert e(K.LAYER_CASES["heads"], "f16x2") == {K.FIRST: 1, K.HEADS3: 1}
    assert e(K.LAYER_CASES["heads"], "bf16") == {K.FIRST: 1, K.W4(False, 2, 1): 1, K.W4(True, dil=2): 1, K.W4(True, dil=4): 1}
    assert e(K.FUSED_CASES["first"], "f16") == {K.PCP: 1, K.W4(True, 2, 1): 1}
    assert e(K.FUSED_CASES["first"], "bf16") == {K.PCP: 1, K.W4(False, 2, 1): 1}
    assert e(K.FUSED_CASES["slim_main_pool"], "f16x3") == {K.FUSE1: 1, K.W4(True, 2, 1): 2}
    assert e(K.FUSED_CASES["k1"], "bf16") == {K.FIRST: 1, K.W4(False, 2, 1): 1, K.W8(128, 1, 1): 1}
    assert e(K.FUSED_CASES["slim"], "f16", dict(mt=4, nt=2)) == {K.FUSE1: 1, K.W4(True, 4, 2): 1}
