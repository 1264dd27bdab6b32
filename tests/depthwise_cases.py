"""Cases, graphs and references for the depthwise convolution (csrc/conv_dw.hip): ``Convolution`` with ``group`` equal to the
bottom's channels and ``num_output = m * channels`` (tests/test_depthwise_host.py, tests/test_gpu_depthwise.py).  Everything
here runs without a GPU.

A layer case is ``(Cin, m, k, stride, pad, dil, H, W)``, each the smallest that exposes one failure mode.  The layer under
test is ``g``, behind ``pre`` / ``sel`` of tests/general_conv_cases.py (1x1 layers that hand the grid on unchanged in every
conv mode).  Three references that must agree (the host file checks it): ``O.convolution(..., group=Cin)``; the same layer
written densely, ``O.convolution`` with the block-diagonal weights of ``dense_weights``; ``naive_depthwise``, a binary64 loop
over the taps that also gives the ``sum |a w|`` of the f64 mode's error bound.

``mbnet_mini(h, w)``: a MobileNet-v1-shaped detector.  ``conv1`` 3x3 stride 2 on the image (3 -> 32), then depthwise 3x3 /
pointwise 1x1 pairs ``dw2`` / ``pw2`` (32 -> 64), ``dw3`` (stride 2) / ``pw3`` (-> 128), ``dw4`` / ``pw4`` (-> 128), ``dw5`` (stride
2) / ``pw5`` (top ``f8``), ``dw6`` (stride 2) / ``pw6`` (top ``f16``); every convolution without a bias and with in-place BatchNorm,
Scale and ReLU behind it; one ProposalLayer (tests/modules_cases.module_tail) on ``f8`` and one on ``f16``.
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC
from tests import norm_cases as N

F32 = np.float32
F64 = np.float64

LAYER_CASES = [
    (32, 1, 3, 1, 1, 1, 9, 11),       # MobileNet's stride-1 layer
    (32, 1, 3, 2, 1, 1, 9, 11),       # its stride-2 layer, odd size
    (32, 1, 3, 2, 1, 1, 8, 10),       # ... even size: the last window falls off
    (16, 1, 3, 1, 1, 1, 1, 1),        # a 1x1 map: eight of nine taps outside
    (8, 1, 3, 1, 1, 1, 2, 3),         # a map shorter than one row strip
    (5, 1, 3, 1, 1, 1, 7, 9),         # ragged C: scalar form, `sel` in front
    (6, 1, 3, 2, 1, 1, 7, 9),         # C % 4 == 2
    (16, 2, 3, 1, 1, 1, 5, 6),        # channel multiplier 2
    (4, 3, 3, 2, 1, 1, 7, 7),         # multiplier 3, strided
    (16, 1, 5, 1, 2, 1, 6, 19),       # 5x5; W crosses a block's column span
    (16, 1, 7, 2, 3, 1, 17, 21),      # 7x7 stride 2
    (8, 1, 3, 1, 2, 2, 7, 7),         # dilation 2, "same"
    (8, 1, 3, 1, 1, 2, 7, 7),         # pad != dilation: the output shrinks
    (16, 1, 3, 1, 0, 1, 5, 6),        # valid
    (8, 1, 3, 1, 0, 1, 3, 3),         # a 1x1 output
    (8, 1, 2, 2, 0, 1, 6, 7),         # even kernel, a dropped column
    (8, 1, 3, 3, 0, 1, 10, 10),       # stride above the strip's reuse; a dropped row
    (16, 1, 1, 1, 0, 1, 4, 5),        # k = 1: a per-channel scale
    (260, 1, 3, 1, 1, 1, 5, 5),       # more channel quads than one wave, with a remainder
    (64, 1, 3, 2, 1, 1, 33, 67),      # several blocks in both directions
]
VARIANTS = G.VARIANTS                 # (bias, in-place ReLU)


def case_id(case):
    return "c%dm%d_k%ds%dp%dd%d_%dx%d" % tuple(case)


def cout(case):
    return case[0] * case[1]


def out_size(case):
    cin, m, k, s, p, d, h, w = case
    return O.conv_out_size(h, k, p, s, d), O.conv_out_size(w, k, p, s, d)


def dense_is_general(case):
    """The layer written densely (group 1) runs the general-geometry kernel: stride != 1, or neither 3x3 pad == dilation nor
    1x1 pad 0."""
    cin, m, k, s, p, d, h, w = case
    return s != 1 or not ((k == 3 and p == d) or (k == 1 and p == 0))


DENSE_TWIN_CASES = [c for c in LAYER_CASES if dense_is_general(c) and c[0] <= 64]


# ---- the layers in front ------------------------------------------------------------------------------------------------------
# `pre` runs the first-layer kernel, whose LDS tile of 64 pixels x (Cout + 4) floats fits the default 64 KiB up to 240 outputs
# (in steps of 16).  A wider case keeps `data` and `pre` at 16 channels and lets `sel` fan them out: row i of its 0/1 matrix
# picks data channel perm[i], perm = a scrambled (0 .. Cin - 1) % 16 -- exact in every mode like the narrow selection.
WIDE = 240


def data_channels(cin):
    return G.data_channels(cin, False) if cin <= WIDE else 16


def feeder_txt(cin):
    """(layer text, the blob `g` reads) of the layers in front of the layer under test."""
    if cin <= WIDE:
        return G.feeder_txt(cin, False)
    return G.conv_txt("pre", "data", 16, 1) + G.conv_txt("sel", "pre", cin, 1), "sel"


def feeder_params(cin):
    """Parameters of `pre` / `sel`, and the channels of `data` that `g` reads (in g's channel order)."""
    if cin <= WIDE:
        return G.feeder_params(cin, False)
    perm = np.random.default_rng(5 + cin).permutation(cin) % 16
    w = np.zeros((cin, 16, 1, 1), F32)
    w[np.arange(cin), perm] = 1.0
    return {"pre": G.feeder_params(16, False)[0]["pre"], "sel": [w, np.zeros(cin, F32)]}, perm


# ---- layer text -------------------------------------------------------------------------------------------------------------
def dw_txt(name, bottom, cin, m, k, stride=1, pad=0, dil=1, relu=False, bias=True, top=None):
    return G.conv_txt(name, bottom, cin * m, k, stride, pad, dil, relu, bias, group=cin, top=top)


def layer_net_text(case, bias=True, relu=False, dense_twin=False):
    """`pre` (/ `sel`) -> `g`; ``dense_twin``: and `g_dense` on the same bottom, the same geometry with group 1."""
    cin, m, k, s, p, d, h, w = case
    txt, bottom = feeder_txt(cin)
    txt += dw_txt("g", bottom, cin, m, k, s, p, d, relu, bias)
    if dense_twin:
        txt += G.conv_txt("g_dense", bottom, cin * m, k, s, p, d, relu, bias)
    return H.single_layer_net(txt, data_channels(cin), h, w)


def concat_net_text(C, h=7, w=9):
    """Two depthwise layers of C channels each (3x3 pad 1 with a ReLU, 5x5 pad 2) on `sel` (16 -> C) write one Concat: `g1` is
    the view at coff C of cstride 2 C (C = 12: the vector form on an offset view; C = 6: the scalar form)."""
    return H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("sel", "pre", C, 1) +
                              dw_txt("g0", "sel", C, 1, 3, 1, 1, 1, relu=True) + dw_txt("g1", "sel", C, 1, 5, 1, 2, 1) +
                              F.concat_layer("cat", ["g0", "g1"]), 16, h, w)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def int_inputs(case, bias, seed=0):
    """Integers: inputs in [-4, 4], weights in [-2, 2], biases in [-8, 8]: the largest |sum| is 49 * 8 + 8, so fp32, the
    split-fp16 and bf16 operands of the layers in front and binary64 all compute the exact integer."""
    cin, m, k, s, p, d, h, w = case
    rng = np.random.default_rng(1000 * cin + 10 * m + k + s + seed)
    data = rng.integers(-4, 5, (1, data_channels(cin), h, w)).astype(F32)
    wt = rng.integers(-2, 3, (cin * m, 1, k, k)).astype(F32)
    bs = rng.integers(-8, 9, (cin * m,)).astype(F32) if bias else None
    return data, wt, bs


def random_inputs(case, bias, seed=0):
    """He-normal weights as `O.synth_params` gives a grouped layer (std sqrt(2 / (k k))), normal inputs, a normal bias."""
    cin, m, k, s, p, d, h, w = case
    params = O.synth_params(P.parse(layer_net_text(case, bias)), seed=77 + seed)
    rng = np.random.default_rng(31 * cin + m + k + seed)
    data = rng.normal(0, 1.0, (1, data_channels(cin), h, w)).astype(F32)
    wt = params["g"][0]
    assert wt.shape == (cin * m, 1, k, k)
    bs = rng.normal(0, 0.5, (cin * m,)).astype(F32) if bias else None
    return data, wt, bs


def g_params(case, wt, bs, dense_twin=False):
    """Parameters of `pre` / `sel` / `g` (/ `g_dense`), and the channels of `data` that `g` reads (in g's channel order)."""
    params, perm = feeder_params(case[0])
    params["g"] = [wt] + ([bs] if bs is not None else [])
    if dense_twin:
        params["g_dense"] = [dense_weights(wt, case[0], case[1])] + ([bs] if bs is not None else [])
    return params, perm


def dense_weights(wt, cin, m):
    """(Cin m, 1, k, k) -> the block-diagonal (Cin m, Cin, k, k): output channel o reads input channel o // m."""
    co, _, k, _ = wt.shape
    assert co == cin * m
    dense = np.zeros((co, cin, k, k), F32)
    dense[np.arange(co), np.arange(co) // m] = wt[:, 0]
    return dense


# ---- references -------------------------------------------------------------------------------------------------------------
def oracle_layer(case, x, wt, bs, relu):
    """`O.convolution(..., group=Cin)` on g's input x (1, Cin, H, W), as float64."""
    cin, m, k, s, p, d, h, w = case
    y = O.convolution(x, wt, bs, pad=p, stride=s, dil=d, group=cin).astype(F64)
    return np.maximum(y, 0) if relu else y


def naive_depthwise(x, w, b, stride, pad, dil, m):
    """One binary64 loop over the taps: x (C, H, W), w (C m, 1, k, k) -> (sum a w + b, sum |a w|), each (C m, Ho, Wo)."""
    C, Hh, Ww = x.shape
    Co, _, k, _ = w.shape
    assert Co == C * m
    Ho, Wo = O.conv_out_size(Hh, k, pad, stride, dil), O.conv_out_size(Ww, k, pad, stride, dil)
    assert Ho >= 1 and Wo >= 1
    xd = np.repeat(x.astype(F64), m, axis=0)            # output channel o reads input channel o // m
    wd = w.astype(F64)[:, 0]
    out, mag = np.zeros((Co, Ho, Wo), F64), np.zeros((Co, Ho, Wo), F64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(k):
                iy = oy * stride - pad + ky * dil
                if not 0 <= iy < Hh:
                    continue
                for kx in range(k):
                    ix = ox * stride - pad + kx * dil
                    if not 0 <= ix < Ww:
                        continue
                    out[:, oy, ox] += wd[:, ky, kx] * xd[:, iy, ix]
                    mag[:, oy, ox] += np.abs(wd[:, ky, kx] * xd[:, iy, ix])
    if b is not None:
        out += b.astype(F64)[:, None, None]
    return out, mag


# ---- the fold's nets ----------------------------------------------------------------------------------------------------------
FOLD_HW = (9, 13)


def fold_text(C, bias, relu, bare=False, hw=FOLD_HW):
    """Net A: `pre` (/ `sel`) -> depthwise 3x3 `g` -> BatchNorm `g_bn` -> Scale `g_sc` (-> ReLU), in place.  ``bare``: net B, the
    same layer with a bias blob (-> ReLU) alone."""
    txt, bottom = G.feeder_txt(C, False)
    txt += dw_txt("g", bottom, C, 1, 3, 1, 1, 1, bias=bias or bare)
    if not bare:
        txt += N.bn_layer("g_bn", "g") + N.scale_layer("g_sc", "g")
    if relu:
        txt += F.relu_layer("g_relu", "g")
    return H.single_layer_net(txt, G.data_channels(C, False), *hw)


def fold_pair(C, bias, relu, hw=FOLD_HW):
    """(message A, parameters A, message B, parameters B, data): B's layer holds ``norm_cases.fold`` of A's blobs."""
    data = np.random.default_rng(200 + C).normal(0, 1, (1, G.data_channels(C, False)) + tuple(hw)).astype(F32)
    msg_a, msg_b = P.parse(fold_text(C, bias, relu, hw=hw)), P.parse(fold_text(C, bias, relu, True, hw=hw))
    pa = N.synth_norm_params(msg_a, data, seed=60 + C + 2 * bias + relu)
    w_eff, b_eff = N.fold(pa["g"][0], pa["g"][1] if bias else None, pa["g_bn"], pa["g_sc"])
    pb = {k: v for k, v in pa.items() if k in ("pre", "sel")}
    pb["g"] = [w_eff, b_eff]
    return msg_a, pa, msg_b, pb, data


# ---- graphs -----------------------------------------------------------------------------------------------------------------
NEIGHBOUR_BLOBS = ("c1", "dw", "pw", "c3")


def neighbours_text(h, w):
    """Split-fp16 neighbours: a family convolution `c1` (3 -> 64, 3x3), the depthwise 3x3 `dw`, the 1x1 `pw` (64 -> 128: the
    split-fp16 GEMM kernel, which reads dw's activation exponent), a family convolution `c3`, `H.mini_detector`'s tail."""
    txt = (G.conv_txt("c1", "data", 64, 3, 1, 1, 1, relu=True) + dw_txt("dw", "c1", 64, 1, 3, 1, 1, 1, relu=True) +
           G.conv_txt("pw", "dw", 128, 1, relu=True) + G.conv_txt("c3", "pw", 128, 3, 1, 1, 1, relu=True))
    return H.mini_detector(txt, "c3", 2, 3, h, w)


MB_MODULES = {
    "8": (["f8"], 2, "{'feat_stride': [8,8],'scales': [1,2], 'ratios':[1,]}"),
    "16": (["f16"], 2, "{'feat_stride': [16,16],'scales': [2,4], 'ratios':[1,]}"),
}
MB_DW_LAYERS = ("dw2", "dw3", "dw4", "dw5", "dw6")
MB_CONVS = ("conv1", "dw2", "pw2", "dw3", "pw3", "dw4", "pw4", "dw5", "pw5", "dw6", "pw6")
MB_BLOBS = ("conv1", "dw2", "pw2", "dw3", "pw3", "dw4", "pw4", "dw5", "f8", "dw6", "f16")
MB_SIZE = (64, 96)
MB_GROUP_SIZES = [(64, 96), (49, 80), (57, 71)]
MB_SEED, MB_THRESH, MB_MIN_SIZE = 32, 0.5, 3.0


def _unit(name, bottom, nout, k, stride=1, pad=0, group=None, top=None, bare=False):
    """Convolution without a bias -> BatchNorm -> Scale -> ReLU in place; ``bare``: with a bias -> ReLU."""
    top = top or name
    txt = G.conv_txt(name, bottom, nout, k, stride, pad, 1, False, bare, group=group, top=top)
    if not bare:
        txt += N.bn_layer("bn_" + name, top) + N.scale_layer("scale_" + name, top)
    return txt + F.relu_layer(name + "_relu", top)


def mbnet_text(h, w, bare=False):
    def pair(i, cin, nout, stride, top=None):
        return (_unit("dw%d" % i, "pw%d" % (i - 1) if i > 2 else "conv1", cin, 3, stride, 1, group=cin, bare=bare) +
                _unit("pw%d" % i, "dw%d" % i, nout, 1, top=top, bare=bare))
    txt = _unit("conv1", "data", 32, 3, 2, 1, bare=bare) + pair(2, 32, 64, 1) + pair(3, 64, 128, 2) + pair(4, 128, 128, 1)
    txt += pair(5, 128, 128, 2, top="f8")
    txt += (_unit("dw6", "f8", 128, 3, 2, 1, group=128, bare=bare) + _unit("pw6", "dw6", 128, 1, top="f16", bare=bare))
    tails = "".join(MC.module_tail(m, *MB_MODULES[m]) for m in MB_MODULES)
    return H.single_layer_net(txt + tails, 3, h, w)


def mbnet_mini(h=MB_SIZE[0], w=MB_SIZE[1], bare=False):
    return P.parse(mbnet_text(h, w, bare))


def mbnet_unit(h, w, seed=4):
    """(data, im_info) of one unit: a synthetic image and an im_info a few pixels inside it."""
    return H.synth_image_blob(h, w, seed=seed + h), np.array([[h - 3, w - 3, 0.75]], F32)


_MB_PARAMS = {}


def mbnet_params():
    """Seeded parameters; the BatchNorm / Scale blobs are trained-like statistics of the oracle's own activations on the first
    unit (`norm_cases.synth_norm_params`).  Computed once."""
    if "p" not in _MB_PARAMS:
        data, info = mbnet_unit(*MB_SIZE)
        _MB_PARAMS["p"] = N.synth_norm_params(mbnet_mini(), data, info, seed=MB_SEED)
    return _MB_PARAMS["p"]


def mbnet_folded_params():
    """The parameters of ``mbnet_mini(bare=True)``: every convolution with `norm_cases.fold` of its BatchNorm and Scale."""
    p = mbnet_params()
    out = {k: v for k, v in p.items() if k.startswith(("cls_score", "bbox_pred"))}
    for name in MB_CONVS:
        out[name] = list(N.fold(p[name][0], None, p["bn_" + name], p["scale_" + name]))
    return out


def mbnet_map_sizes(h, w):
    s = lambda n: O.conv_out_size(n, 3, 1, 2, 1)   # noqa: E731
    h2, w2 = s(h), s(w)
    h4, w4 = s(h2), s(w2)
    h8, w8 = s(h4), s(w4)
    return {"conv1": (h2, w2), "pw2": (h2, w2), "dw3": (h4, w4), "pw4": (h4, w4), "f8": (h8, w8), "f16": (s(h8), s(w8))}


def mbnet_oracle(h=MB_SIZE[0], w=MB_SIZE[1], bare=False):
    return N.NormOracleNet(mbnet_mini(h, w, bare), params=mbnet_folded_params() if bare else mbnet_params(),
                           proposal_cfg=O.ProposalParams(pre_nms_topN=10000, score_thresh=MB_THRESH, min_size=MB_MIN_SIZE))


def forwarded(onet, data, info):
    onet.blobs["data"].reshape(*data.shape)
    onet.blobs["im_info"].reshape(*info.shape)
    onet.forward(data=data, im_info=info)
    return onet
