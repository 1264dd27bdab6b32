"""Inputs on exact grids and the case table of the conv-mode tests (test_conv_mode_models.py on the CPU,
test_gpu_conv_modes.py on the GPU; the models themselves: oracle/conv_modes.py).

A case is a small graph -- per-layer path: data -> c0 (the first-layer kernel) -> the layer(s) under test, no proposal
tail; fused path: a mini-detector of tests/test_gpu_fused_forms.py's builders -- with parameters from one of four GRIDS on
which every product a mode forms and every partial sum is an fp32 number, so the layer's output in a mode is one number:
  "two"     activations and weights x = x_h + x_l: x_h = +-4 or +-6 (or the whole value 0),
            x_l in {-3..3} 2^-12, so fp16(x) = x_h and the low part is x_l exactly; 64 non-zero weights per output channel
            at seeded positions: sum |a w| < 2^12, 24 bits with the 2^-12 quantum.  Feeds the lo paths.
  "around"  activations +-2^k (1 + j 2^-13), k in {0, 1}, j just below / at / just above a rounding tie of fp16 (j = 8n +
            3, 4, 5) or of bf16 (j = 64n + 31, 32, 33), n even and odd, different in neighbouring channels and pixels;
            weights in {0, +-1, +-2}.  Holds the activation conversions.
  "wround"  the same values in the weights, activations in {0, 1, 2}: holds the host-side weight packs.
  "int"     small integers in both operands: exact in every mode, fp32 included.
The activations reach the layer under test through layers that are exact on the grid: c0 copies one image tap per
channel (one-hot weights +-1, ReLU; taps outside the image are zeros), and on the fused path the convolutions in front of
and behind the layer under test are one-hot centre-tap copies; the model (conv_modes.net_model) is chained through all of
them with each layer's own rule, so what they do to the low parts in a reduced mode is part of the expectation.
"""
import numpy as np

from oracle import conv_modes as CM
from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import conv_plan_cases as PL
from tests import helpers as H
from tests.test_gpu_fused_forms import conv as conv_txt, pool as pool_txt

GRIDS = ("two", "around", "wround", "int")
SPLIT_MODES = ("f16x3", "f16x2", "f16", "bf16")
NNZ = 64


def modes_of(grid, fused=False):
    return SPLIT_MODES if (fused or grid != "int") else CM.MODES


# ------------------------------------------------------------------------------------------------------------
# profiler classes (net_forward.cpp kProfNames: a class is a kernel FORM -- the reduced modes' NP / BF instantiations of a
# form are booked under the form's headline name)
# ------------------------------------------------------------------------------------------------------------
def W8(bn, dil=1, ks=3, fuse1=False):
    return "conv_mfma_f16x3_kernel<%d, %s, %d, %d, 3, false>" % (bn, "true" if fuse1 else "false", dil, ks)


def W4(split, mt=2, nt=1, dil=1):
    if dil != 1:     # (one class per dilation, whatever the input format)
        return "conv_mfma_f16x3_w4d_kernel<true, 4, 1, 3, false, %d>" % dil
    return "conv_mfma_f16x3_w4d_kernel<%s, %d, %d, 3, false, 1>" % ("true" if split else "false", mt, nt)


FUSE1, PCP, PC = W8(64, 1, 3, True), "conv_mfma_f16x3_pc_kernel<3, false, true>", "conv_mfma_f16x3_pc_kernel<3, false, false>"
K1, HEADS3 = "conv_mfma_f16x3_k1_kernel<true, 3>", "conv_mfma_f16x3_heads3_kernel<true, 3>"
FIRST, POOLK, DIRECT = "conv_first_kernel", "maxpool_kernel", "conv_direct_kernel"


def F32(ks, dil, bn):
    return "conv_mfma_f32_kernel<%d, %d, %d, %d, 16>" % (ks, dil if ks == 3 else 0, bn, 8 if bn == 128 else 16)


def conv_classes(prof):
    """{class: launches} of the convolution and pool classes that ran."""
    return {k: int(v["launches"]) for k, v in prof.items()
            if int(v["launches"]) and (k.startswith("conv_") or k == POOLK)}


# ------------------------------------------------------------------------------------------------------------
# graphs
# ------------------------------------------------------------------------------------------------------------
def Lc(name, bottom, cin, nout, k=3, dil=1, relu=True, **kw):
    return dict(op="conv", name=name, bottom=bottom, cin=cin, nout=nout, k=k, dil=dil, relu=relu, **kw)


def Lp(name, bottom):
    return dict(op="pool", name=name, bottom=bottom)


def graph_text(graph):
    s = ""
    for L in graph:
        if L["op"] == "conv":
            s += conv_txt(L["name"], L["bottom"], L["nout"], L["k"], L["dil"], L["relu"], "shared_as" in L)
        elif L["op"] == "pool":
            s += pool_txt(L["name"], L["bottom"])
        else:
            s += L["text"]
    return s


def _layer_case(cin, cout, k=3, dil=1, relu=True, sizes=((9, 17), (23, 40))):
    return dict(graph=[Lc("c0", "data", 3, cin), Lc("ct", "c0", cin, cout, k, dil, relu)], under=["ct"], sizes=sizes, fused=False)


_HEADS = [Lc("h1", None, 128, 128, 3, 1, shared_as="h1"), Lc("h2", None, 128, 128, 3, 2, shared_as="h1"),
          Lc("h4", None, 128, 128, 3, 4, shared_as="h1")]


def _heads(bottom):
    return [dict(L, bottom=bottom) for L in _HEADS]


LAYER_CASES = {
    # 8-wave kernel
    "w8_128_3x3": _layer_case(32, 128, relu=False),
    "w8_128_1x1": _layer_case(64, 128, 1),
    "w8_64_3x3": _layer_case(64, 64),
    "w8_64_d2": _layer_case(32, 64, 3, 2),
    "w8_64_d4": _layer_case(32, 64, 3, 4, relu=False, sizes=((9, 17), (23, 40), (5, 6))),
    "w8_64_1x1": _layer_case(64, 64, 1),
    # a convolution into a Concat slice that starts at channel 66: value-by-value stores (conv_store_tile)
    "w8_unaligned": dict(graph=[Lc("c0", "data", 3, 64), dict(op="raw", name="ca", bottom="c0", text=conv_txt("ca", "c0", 66)),
                                Lc("cb", "c0", 64, 64, aligned=False),
                                dict(op="raw", name="cat", bottom=None,
                                     text='layer { name: "cat" type: "Concat" bottom: "ca" bottom: "cb" top: "cat" }\n')],
                         under=["cb"], sizes=((9, 17), (23, 40)), fused=False),
    # dual-tile family: slim (short K), two per CU (Cin 256), dilated
    "slim_64_128": _layer_case(64, 128),
    "slim_128_256": _layer_case(128, 256, relu=False),
    "fam_256_128": _layer_case(256, 128),
    "fam_d2": _layer_case(128, 128, 3, 2),
    "fam_d4": _layer_case(128, 128, 3, 4, relu=False, sizes=((9, 17), (23, 40), (5, 6))),
    # 1x1 GEMM kernel (bf16: the 8-wave kernel's 1x1 form)
    "k1_96_256": _layer_case(96, 256, 1, relu=False),
    "k1_256_256": _layer_case(256, 256, 1, sizes=((9, 17), (23, 40), (23, 29))),
    # the three shared-weight heads: one launch in the fp16 modes, three in bf16
    "heads": dict(graph=[Lc("c0", "data", 3, 128)] + _heads("c0"), under=["h1", "h2", "h4"], sizes=((9, 17), (23, 40)), fused=False),
}
FAMILY_DIL1 = ("slim_64_128", "slim_128_256", "fam_256_128")

_C0, _C1 = Lc("c0", "data", 3, 64), Lc("c1", "c0", 64, 128)
FUSED_CASES = {
    # the fused first pair (18x34 in: the pooled 9x17 map is read by a family convolution, here a copy)
    "first": dict(graph=[_C0, Lc("c1", "c0", 64, 64), Lp("p", "c1"), Lc("c2", "p", 64, 128)], under=["c1"], probe="c2",
                  sizes=((18, 34),), keep3=["c2"]),
    # slim with split input: plain, pool + main, pool only
    "slim": dict(graph=[_C0, _C1, Lc("c2", "c1", 128, 128)], under=["c2"], probe="c2", sizes=((9, 17), (23, 40))),
    "slim_main_pool": dict(graph=[_C0, _C1, Lc("c2", "c1", 128, 128), Lp("p", "c2"), Lc("c3", "c2", 128, 128), Lp("p3", "c3")],
                           under=["c2"], probe=["p", "p3"], sizes=((9, 17), (23, 40)), keep3=["c3"]),
    "slim_pool_only": dict(graph=[_C0, _C1, Lc("c2", "c1", 128, 128), Lp("p", "c2")], under=["c2"], probe="p",
                           sizes=((9, 17), (23, 40))),
    "fam256": dict(graph=[_C0, Lc("c1", "c0", 64, 256), Lc("c2", "c1", 256, 256)], under=["c2"], probe="c2", sizes=((9, 17), (23, 40))),
    "dil2": dict(graph=[_C0, _C1, Lc("c2", "c1", 128, 128, 3, 2)], under=["c2"], probe="c2", sizes=((9, 17), (23, 40))),
    "dil4": dict(graph=[_C0, _C1, Lc("c2", "c1", 128, 128, 3, 4, relu=False)], under=["c2"], probe="c2", sizes=((9, 17), (23, 40))),
    "k1": dict(graph=[_C0, Lc("c1", "c0", 64, 256), Lc("c2", "c1", 256, 256, 1)], under=["c2"], probe="c2", sizes=((9, 17), (23, 40))),
    "heads3": dict(graph=[_C0, _C1] + _heads("c1"), under=["h1", "h2", "h4"], probe=["h1", "h2", "h4"], sizes=((9, 17), (23, 40))),
}
for _c in FUSED_CASES.values():
    _c["fused"] = True


# set_layer_products on the per-layer path: c1 and c3 are copies (slim, 8-wave) around the layer under test
OVERRIDE_CASE = dict(graph=[Lc("c0", "data", 3, 64), Lc("c1", "c0", 64, 128), Lc("c2", "c1", 128, 128, relu=False),
                            Lc("c3", "c2", 128, 64)], under=["c2"], sizes=((23, 40),), fused=False)


def case_of(name):
    return LAYER_CASES[name] if name in LAYER_CASES else FUSED_CASES[name]


def probes_of(case):
    if not case["fused"]:
        return list(case["under"])
    return [case["probe"]] if isinstance(case["probe"], str) else list(case["probe"])


def products_of(case, mode):
    """The per-layer override the case's read-out convolutions need: a copy behind the layer under test keeps three
    products in the fp16 modes (bf16 has no products to choose)."""
    return {n: 3 for n in case.get("keep3", [])} if mode in ("f16x2", "f16") else {}


def conversion_layer(case, mode):
    """The layer whose kernel converts fp32 activations that still carry low bits.  Per-layer path: the layer under test.
    Fused path: the layer under test in the fp16 modes (the copy in front of it keeps three products); in bf16 every
    layer rounds, so behind the first one a layer only sees bf16 numbers -- the conversion that meets the grid's low bits is
    the first pair's conv1_1 (the image) or the copy in front of the layer under test.  (bf16 has no split-input forms: the
    fused path runs the per-layer path's instantiations, whose conversions the per-layer cases feed directly.)"""
    if not case["fused"] or mode != "bf16":
        return case["under"][0]
    return "c0" if case["under"][0] == "c1" else "c1"


def net_text(case, h, w):
    g = graph_text(case["graph"])
    if case["fused"]:
        return H.mini_detector(g, case["probe"], 2, 3, h, w)
    return H.single_layer_net(g, 3, h, w)


# ------------------------------------------------------------------------------------------------------------
# grids
# ------------------------------------------------------------------------------------------------------------
def _two_part(rng, shape):
    # (x_h = +-4 or +-6, not +-2: just below a power of two fp16's spacing halves, and 2 - 3 2^-12 would not round to 2)
    x = rng.choice([-1.0, 1.0], shape) * 2.0 * rng.integers(2, 4, shape) + rng.integers(-3, 4, shape) * 2.0 ** -12
    assert np.array_equal(x.astype(np.float16).astype(np.float64), np.round(x))
    return x.astype(np.float32)


def _around(rng, shape):
    n16, n8 = rng.integers(0, 1024, shape), rng.integers(0, 128, shape)
    j = np.where(rng.integers(0, 2, shape) == 0, 8 * n16 + rng.integers(3, 6, shape), 64 * n8 + rng.integers(31, 34, shape))
    x = rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.integers(0, 2, shape) * (1.0 + j * 2.0 ** -13)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return x.astype(np.float32)


def _ints(rng, shape, top, signed=True):
    x = rng.integers(1, top + 1, shape).astype(np.float64)
    return (x * rng.choice([-1.0, 1.0], shape) if signed else x).astype(np.float32)


def image(grid, h, w, seed=7):
    rng = np.random.default_rng(seed)
    if grid == "two":
        return _two_part(rng, (3, h, w))
    if grid == "around":
        return _around(rng, (3, h, w))
    return _ints(rng, (3, h, w), 2 if grid == "wround" else 4)


def first_weights(nout):
    """c0: channel co copies image channel co % 3 at tap (co // 3) % 9 with weight +1 / -1, no bias (ReLU follows)."""
    w = np.zeros((nout, 3, 3, 3), np.float32)
    for co in range(nout):
        t = (co // 3) % 9
        w[co, co % 3, t // 3, t % 3] = 1.0 if (co // 27) % 2 == 0 else -1.0
    return w, np.zeros(nout, np.float32)


def copy_weights(nout, cin, k):
    """A centre-tap copy: output channel co = input channel co % cin."""
    w = np.zeros((nout, cin, k, k), np.float32)
    w[np.arange(nout), np.arange(nout) % cin, k // 2, k // 2] = 1.0
    return w, np.zeros(nout, np.float32)


def test_weights(grid, nout, cin, k, seed):
    """The layer under test: NNZ non-zero weights per output channel at seeded positions, and a bias, on the grid."""
    rng = np.random.default_rng(seed)
    n = cin * k * k
    nnz = min(NNZ, n)
    w = np.zeros((nout, n), np.float32)
    for co in range(nout):
        pos = rng.choice(n, nnz, replace=False)
        if grid == "two":
            w[co, pos] = _two_part(rng, nnz)
        elif grid == "wround":
            w[co, pos] = _around(rng, nnz)
        else:
            w[co, pos] = _ints(rng, nnz, 2 if grid == "around" else 3)
    b = rng.integers(-4, 5, nout).astype(np.float64)
    if grid == "two":
        b = b + rng.integers(-3, 4, nout) * 2.0 ** -12
    return w.reshape(nout, cin, k, k), b.astype(np.float32)


def grid_params(case, grid, seed=11):
    """{layer: (w, b)} of the case's modelled convolutions."""
    out = {}
    for i, L in enumerate(case["graph"]):
        if L["op"] != "conv" or L.get("shared_as", L["name"]) != L["name"]:
            continue
        if L["bottom"] == "data":
            out[L["name"]] = first_weights(L["nout"])
        elif L["name"] in case["under"]:
            out[L["name"]] = test_weights(grid, L["nout"], L["cin"], L["k"], seed + i)
        else:
            out[L["name"]] = copy_weights(L["nout"], L["cin"], L["k"])
    return out


def make_nets(case, h, w, with_gpu):
    """(gpu net or None, oracle net) of the case at input size h x w, seeded parameters everywhere (the grids come in
    through `load_grid`), zero predictors."""
    msg = P.parse(net_text(case, h, w))
    params = O.synth_params(msg, seed=5)
    for name, blobs in params.items():
        if name.startswith("cls_score") or name.startswith("bbox_pred"):
            for b in blobs:
                b[...] = 0
    onet = O.OracleNet(msg, params=params)
    gnet = None
    if with_gpu:
        from smallhardface_amd import caffe
        gnet = caffe.Net(None, prototxt_text=P.dumps(msg))
    return gnet, onet


def load_grid(case, grid, gnet, onet):
    params = grid_params(case, grid)
    for L in case["graph"]:
        if L["op"] == "conv":
            w, b = params[L.get("shared_as", L["name"])]
            onet.params[L["name"]][0][...] = w
            onet.params[L["name"]][1][...] = b
    if gnet is not None:
        H.load_params(gnet, onet.params)
    return params


def model(case, grid, h, w, mode, inputs=None, wrong=None, wrong_layer=None, products=None, params=None, data=None):
    """{blob: float32 (C, H, W)}: the case's model in `mode`."""
    params = grid_params(case, grid) if params is None else params
    data = image(grid, h, w) if data is None else data
    prod = products_of(case, mode) if products is None else products
    return CM.net_model(case["graph"], params, data, mode, case["fused"], prod, wrong, wrong_layer, inputs)


# ------------------------------------------------------------------------------------------------------------
# which kernel form must run.  Without a "plan" entry in `knobs`: the planner on 256 compute units, where maps this small are
# one round of single 8-row tiles ("mt" / "nt": a form forced by knob).  knobs["plan"] = dict(cus=, units=[(h, w), ..] of the
# net's input, env={the planner's knobs as environment variables}): tile rows and cover of every dilation-1 family layer come
# from the planner's restatement (tests/conv_plan_cases.py) for that CU count -- a hybrid cover is one launch of the two-tile
# class AND one of the single-tile class.
# ------------------------------------------------------------------------------------------------------------
def _conv_class(L, mode, split_in, knobs=None, units=None):
    cin, cout, k, dil = L["cin"], L["nout"], L["k"], L["dil"]
    bf = mode == "bf16"
    if mode == "fp32" or not CM.eligible(cin, cout, k, dil):
        if not CM.eligible(cin, cout, k, dil):
            return DIRECT
        return F32(k, dil, 128 if cout % 128 == 0 else 64)
    if CM.family_shape(cin, cout, k, bf, L.get("aligned", True)):
        if k == 1:
            return K1
        if dil != 1:
            return W4(True, dil=dil)
        pl = (knobs or {}).get("plan")
        if pl:
            p = PL.plan(units, cin, cout, pl["cus"], knobs=PL.knobs_of(pl.get("env", {})))
            return [W4(split_in and not bf, p["mt"], q["ntile"]) for q in p["launches"]]
        mt, nt = (knobs or {}).get("mt", 2), (knobs or {}).get("nt", 1)
        return W4(split_in and not bf, mt, nt)
    bn = 64 if (cout % 128 or (k == 3 and dil != 1)) else 128
    return W8(bn, dil if k == 3 else 1, k)


def expected_classes(case, mode, knobs=None):
    """{class: launches per forward} of the case's graph in `mode`."""
    out = {}
    graph = case["graph"]
    fused = case["fused"] and mode != "fp32"
    add = lambda c: out.__setitem__(c, out.get(c, 0) + 1)
    split_blob = {}
    heads_done = False
    sizes = {"data": [tuple(u) for u in (knobs or {}).get("plan", {}).get("units", [])]}      # blob -> the units' map sizes
    for L in graph:
        if L.get("bottom") in sizes:
            sizes[L["name"]] = [((h + 1) // 2, (w + 1) // 2) for h, w in sizes[L["bottom"]]] if L["op"] == "pool" else sizes[L["bottom"]]
        if L["op"] == "pool":
            prod = [M for M in graph if M["name"] == L["bottom"]][0]
            if not (fused and prod["op"] == "conv" and CM.eligible(prod["cin"], prod["nout"], prod["k"], prod["dil"])):
                add(POOLK)
            continue
        if L["op"] != "conv":
            if L["name"] == "ca":
                add(DIRECT)
            continue
        r = CM.layer_rule(L, graph, mode, fused)
        if r["arith"] == "absorbed":
            continue
        if L["bottom"] == "data":
            add(FIRST)
            continue
        if r["first"]:
            add((knobs or {}).get("pc", PCP) if r["first"] == "pc" else FUSE1)
            continue
        if "shared_as" in L and mode not in ("fp32", "bf16"):
            if not heads_done:
                add(HEADS3)
            heads_done = True
            continue
        # split-format input: every reader of the bottom blob is a family-shaped convolution of an fp16 mode on the fused path
        rd = [M for M in graph if M.get("bottom") == L["bottom"] and M["op"] == "conv"]
        split_in = fused and mode != "bf16" and all(CM.family_shape(M["cin"], M["nout"], M["k"], False) for M in rd)
        cls = _conv_class(L, mode, split_in, knobs, sizes.get(L["bottom"]))
        for c in (cls if isinstance(cls, list) else [cls]):
            add(c)
    return out
