"""Cases, graphs and references for the general-geometry convolution (csrc/conv_gen.h): any square kernel, stride, pad and
dilation, on the NHWC activations or on the NCHW net input (tests/test_general_conv_host.py, tests/test_gpu_general_conv.py).
Everything here runs without a GPU.

A layer case is ``(Cin, Cout, k, stride, pad, dil, H, W)``, each the smallest that exposes one failure mode.  The layer under
test is ``g``.  A layer on the activations sits behind 1x1 layers that hand the grid on unchanged in every conv mode: ``pre``
on ``data`` (an identity matrix; the first-layer kernel takes output counts that are multiples of 16, so ``data`` carries
Cin rounded up to one) and, where Cin is no multiple of 16, ``sel`` (a 0/1 selection matrix that picks Cin of those channels
in a scrambled order).  Both carry zero biases: x * 1 + 0 * ... is x in fp32, in the split-fp16 modes (integers and fp16 values
are their own high halves), in bf16 (integers up to 256) and in binary64.

``s3fd_mini(h, w)``: an S3FD-shaped graph.  Trunk: a 7x7 stride-2 pad-3 stem on the image (3 -> 64), a 3x3 layer, a 2x2 pool and
two 3x3 layers giving ``f8`` (128 channels); extra 1: 1x1 64 and 3x3 stride 2 128 giving ``f16``; extra 2 the same giving
``f32``; one ProposalLayer (tests/modules_cases.module_tail) on each with feat_stride 8, 16 and 32.  (The maps are at 1/4, 1/8
and 1/16 of the input; the anchors' strides are the detector family's.)
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H
from tests import modules_cases as MC
from tests.fusion_cases import FusionOracleNet  # noqa: F401  (the oracle net of the graph cases)

F32 = np.float32

LAYER_CASES = [
    (32, 64, 3, 2, 1, 1, 9, 11),      # the S3FD extra
    (32, 64, 3, 2, 1, 1, 8, 10),      # ... at an even size: the last window falls off
    (5, 7, 3, 2, 1, 1, 7, 9),         # ragged Cin, Cout and K
    (32, 64, 1, 2, 0, 1, 7, 8),       # a shortcut
    (16, 32, 3, 1, 0, 1, 5, 6),       # valid
    (16, 16, 3, 1, 2, 1, 4, 5),       # the output grows
    (8, 8, 2, 2, 0, 1, 6, 7),         # even kernels; a dropped column
    (8, 8, 4, 2, 1, 1, 6, 7),
    (32, 32, 3, 2, 2, 2, 9, 9),       # stride with dilation
    (8, 8, 3, 1, 1, 2, 7, 7),         # pad != dilation
    (40, 72, 5, 1, 2, 1, 6, 19),      # K = 1000 is no chunk multiple; Cout crosses the 64 tile; W crosses the 16-pixel tile
    (8, 8, 3, 1, 0, 1, 3, 3),         # a 1x1 output
    (8, 8, 3, 3, 0, 1, 10, 10),       # stride 3; a dropped row
    (64, 128, 3, 2, 1, 1, 33, 67),    # several tiles in both directions, two cout tiles
]
IMAGE_CASES = [                       # on the image: NCHW input, Cin 3
    (3, 64, 7, 2, 3, 1, 17, 21),
    (3, 24, 7, 4, 3, 1, 19, 23),
]
ALL_CASES = [(c, False) for c in LAYER_CASES] + [(c, True) for c in IMAGE_CASES]
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]   # (bias, in-place ReLU)


def case_id(case_first):
    case, first = case_first
    return "%s%dto%d_k%ds%dp%dd%d_%dx%d" % (("img_" if first else "",) + tuple(case))


def out_size(case):
    cin, cout, k, s, p, d, h, w = case
    return O.conv_out_size(h, k, p, s, d), O.conv_out_size(w, k, p, s, d)


# ---- layer text -------------------------------------------------------------------------------------------------------------
def conv_txt(name, bottom, nout, k, stride=1, pad=0, dil=1, relu=False, bias=True, group=None, top=None):
    top = top or name
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d kernel_size: %d '
         'stride: %d pad: %d dilation: %d%s%s } }\n'
         % (name, bottom, top, nout, k, stride, pad, dil, "" if bias else " bias_term: false",
            "" if group is None else " group: %d" % group))
    if relu:
        s += 'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, top, top)
    return s


def data_channels(cin, first):
    return cin if first else -(-cin // 16) * 16


def feeder_txt(cin, first):
    """(layer text, the blob `g` reads) of the layers in front of the layer under test."""
    if first:
        return "", "data"
    cd = data_channels(cin, False)
    txt = conv_txt("pre", "data", cd, 1)
    if cd == cin:
        return txt, "pre"
    return txt + conv_txt("sel", "pre", cin, 1), "sel"


def layer_net_text(case, first, bias=True, relu=False):
    cin, cout, k, s, p, d, h, w = case
    txt, bottom = feeder_txt(cin, first)
    return H.single_layer_net(txt + conv_txt("g", bottom, cout, k, s, p, d, relu, bias), data_channels(cin, first), h, w)


def concat_net_text(h=9, w=11):
    """Two 12-channel general convolutions (3x3 stride 2 pad 1 and 5x5 stride 2 pad 2 of `pre`) written into one Concat: `g1`
    is an unaligned view with coff 12 and cstride 24."""
    return H.single_layer_net(conv_txt("pre", "data", 16, 1) + conv_txt("g0", "pre", 12, 3, 2, 1, 1, relu=True) +
                              conv_txt("g1", "pre", 12, 5, 2, 2, 1) +
                              'layer { name: "cat" type: "Concat" bottom: "g0" bottom: "g1" top: "cat" concat_param { axis: 1 } }\n',
                              16, h, w)


def selection(cin, cd, seed=5):
    """The `sel` weights: row i picks data channel perm[i] (a 0/1 matrix), and the picked channels."""
    perm = np.random.default_rng(seed + cin).permutation(cd)[:cin]
    w = np.zeros((cin, cd, 1, 1), F32)
    w[np.arange(cin), perm] = 1.0
    return w, perm


def feeder_params(cin, first):
    """Parameters of `pre` / `sel`, and the channels of `data` that `g` reads (in g's channel order)."""
    if first:
        return {}, np.arange(cin)
    cd = data_channels(cin, False)
    params = {"pre": [np.eye(cd, dtype=F32).reshape(cd, cd, 1, 1), np.zeros(cd, F32)]}
    if cd == cin:
        return params, np.arange(cin)
    w, perm = selection(cin, cd)
    params["sel"] = [w, np.zeros(cin, F32)]
    return params, perm


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def int_inputs(case, first, bias, seed=0):
    """Integers: inputs in [-4, 4], weights in [-2, 2], biases in [-8, 8] -- every partial sum stays below 2^24 in magnitude
    (the largest: K = 1000 of case (40, 72, 5): 1000 * 8 + 8), so fp32, the split-fp16 and bf16 operands and binary64 all
    compute the exact integer."""
    cin, cout, k, s, p, d, h, w = case
    rng = np.random.default_rng(1000 * cin + 10 * cout + k + s + seed)
    data = rng.integers(-4, 5, (1, data_channels(cin, first), h, w)).astype(F32)
    wt = rng.integers(-2, 3, (cout, cin, k, k)).astype(F32)
    bs = rng.integers(-8, 9, (cout,)).astype(F32) if bias else None
    return data, wt, bs


def random_inputs(case, first, bias, seed=0):
    """He-normal weights as `O.synth_params` gives them (a layer on `data` scaled by 1/64), normal inputs (on `data`: of the
    image's magnitude), a normal bias."""
    cin, cout, k, s, p, d, h, w = case
    params = O.synth_params(P.parse(layer_net_text(case, first, bias)), seed=77 + seed)
    rng = np.random.default_rng(31 * cin + cout + k + seed)
    data = rng.normal(0, 64.0 if first else 1.0, (1, data_channels(cin, first), h, w)).astype(F32)
    wt = params["g"][0]
    bs = rng.normal(0, 0.5, (cout,)).astype(F32) if bias else None
    return data, wt, bs


def g_params(case, first, wt, bs):
    params, perm = feeder_params(case[0], first)
    params["g"] = [wt] + ([bs] if bs is not None else [])
    return params, perm


# ---- references -------------------------------------------------------------------------------------------------------------
def naive_conv(x, w, b, stride, pad, dil, dtype=np.float64):
    """Caffe's convolution as one loop over the taps in `dtype`: x (C, H, W), w (Co, C, k, k) -> (sum a w + b, sum |a w|),
    each (Co, Ho, Wo).  Output pixel (oy, ox) reads input (oy * stride - pad + ky * dil, ox * stride - pad + kx * dil)."""
    C, Hh, Ww = x.shape
    Co, _, k, _ = w.shape
    Ho, Wo = O.conv_out_size(Hh, k, pad, stride, dil), O.conv_out_size(Ww, k, pad, stride, dil)
    assert Ho >= 1 and Wo >= 1
    xd, wd = x.astype(dtype), w.astype(dtype)
    out = np.zeros((Co, Ho, Wo), dtype)
    mag = np.zeros((Co, Ho, Wo), dtype)
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
                    out[:, oy, ox] += wd[:, :, ky, kx] @ xd[:, iy, ix]
                    mag[:, oy, ox] += np.abs(wd[:, :, ky, kx]) @ np.abs(xd[:, iy, ix])
    if b is not None:
        out += b.astype(dtype)[:, None, None]
    return out, mag


def oracle_layer(case, x, wt, bs, relu):
    """`O.convolution` on g's input x (1, Cin, H, W) with the case's geometry, as float64."""
    cin, cout, k, s, p, d, h, w = case
    y = O.convolution(x, wt, bs, pad=p, stride=s, dil=d).astype(np.float64)
    return np.maximum(y, 0) if relu else y


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def neighbours_text(h, w):
    """Split-format neighbours: family convolutions (3 -> 64 -> 64, 3x3), a general 3x3 stride 2 (64 -> 128), a family
    convolution (128 -> 128), `H.mini_detector`'s tail on the last one."""
    txt = (conv_txt("c1", "data", 64, 3, 1, 1, 1, relu=True) + conv_txt("c2", "c1", 64, 3, 1, 1, 1, relu=True) +
           conv_txt("g", "c2", 128, 3, 2, 1, 1, relu=True) + conv_txt("c3", "g", 128, 3, 1, 1, 1, relu=True))
    return H.mini_detector(txt, "c3", 2, 3, h, w)


S3FD_MODULES = {
    "8": (["f8"], 2, "{'feat_stride': [8,8],'scales': [1,2], 'ratios':[1,]}"),
    "16": (["f16"], 2, "{'feat_stride': [16,16],'scales': [2,4], 'ratios':[1,]}"),
    "32": (["f32"], 2, "{'feat_stride': [32,32],'scales': [4,8], 'ratios':[1,]}"),
}
S3FD_GENERAL_LAYERS = ("stem", "e1b", "e2b")
S3FD_SIZE = (64, 96)
S3FD_GROUP_SIZES = [(64, 96), (49, 80), (57, 71)]
S3FD_SEED, S3FD_THRESH, S3FD_MIN_SIZE = 21, 0.3, 0.0   # (no min-size cut: the row sets hinge on the score threshold alone)


def s3fd_text(h, w):
    trunk = (conv_txt("stem", "data", 64, 7, 2, 3, 1, relu=True) + conv_txt("c2", "stem", 64, 3, 1, 1, 1, relu=True) +
             MC._pool("p2", "c2") + conv_txt("c3", "p2", 128, 3, 1, 1, 1, relu=True) + conv_txt("f8", "c3", 128, 3, 1, 1, 1, relu=True))
    extra = (conv_txt("e1a", "f8", 64, 1, relu=True) + conv_txt("e1b", "e1a", 128, 3, 2, 1, 1, relu=True, top="f16") +
             conv_txt("e2a", "f16", 64, 1, relu=True) + conv_txt("e2b", "e2a", 128, 3, 2, 1, 1, relu=True, top="f32"))
    tails = "".join(MC.module_tail(m, *S3FD_MODULES[m]) for m in S3FD_MODULES)
    return H.single_layer_net(trunk + extra + tails, 3, h, w)


def s3fd_mini(h=S3FD_SIZE[0], w=S3FD_SIZE[1]):
    return P.parse(s3fd_text(h, w))


def s3fd_params():
    return O.synth_params(s3fd_mini(), seed=S3FD_SEED, cls_bias=1.0)


def s3fd_unit(h, w, seed=4):
    """(data, im_info) of one unit: a synthetic image and an im_info a few pixels inside it."""
    return H.synth_image_blob(h, w, seed=seed + h), np.array([[h - 3, w - 3, 0.75]], F32)


def s3fd_map_sizes(h, w):
    h2, w2 = O.conv_out_size(h, 7, 3, 2, 1), O.conv_out_size(w, 7, 3, 2, 1)
    h4, w4 = -(-h2 // 2), -(-w2 // 2)
    h8, w8 = O.conv_out_size(h4, 3, 1, 2, 1), O.conv_out_size(w4, 3, 1, 2, 1)
    return {"stem": (h2, w2), "f8": (h4, w4), "f16": (h8, w8), "f32": (O.conv_out_size(h8, 3, 1, 2, 1), O.conv_out_size(w8, 3, 1, 2, 1))}


def s3fd_oracle(h=S3FD_SIZE[0], w=S3FD_SIZE[1]):
    return FusionOracleNet(s3fd_mini(h, w), params=s3fd_params(), proposal_cfg=O.ProposalParams(
        pre_nms_topN=10000, score_thresh=S3FD_THRESH, min_size=S3FD_MIN_SIZE))
