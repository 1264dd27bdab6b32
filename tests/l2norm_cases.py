"""Cases, graphs and references for the Normalize layer (csrc/l2norm.hip: channel_l2norm), the per-pixel L2 norm over channels
with a learned scale of the SSD / S3FD lineage (tests/test_l2norm_host.py, tests/test_gpu_l2norm.py).  Everything here runs
without a GPU.

The layer (normalize_layer.cpp:85-134 of the reference's Caffe, ``across_spatial: false``), for every pixel of a 4-D blob:
``S = sum_c x_c^2``, ``norm = sqrt(S + eps)``, ``top_c = (x_c / norm) * scale_c``; with ``channel_shared`` the blob has no
axes and one value.  Two references:

``normalize``     binary64 from the fp32 values (eps: its fp32 value), unrounded -- the yardstick, and rounded once what conv
                  mode "f64" computes.
``normalize32``   the kernel's fixed operation order in fp32: per lane ``s = fmaf(x, x, s)`` over its channel quads (or
                  channels, in the scalar form) in ascending order, an xor-butterfly over the pixel's lanes with masks 1, 2,
                  4, ..., then ``+ eps``, ``sqrt``, ``/`` and ``*`` with one rounding each.  The fmaf is stated as
                  ``fp32(fp64(x) * fp64(x) + fp64(s))``: the product is exact in binary64, the sum is rounded to binary64 and
                  then to fp32 -- equal to the fused operation except where that double rounding meets a tie, which integer
                  grids (every value exact) never do.  ``form(C, vec)`` is the launcher's choice of lanes per pixel and items
                  per lane (``l2norm_form``).

A layer case is ``(C, H, W)``.  The layer under test is ``n``, behind ``pre`` / ``sel`` of tests/general_conv_cases.py (1x1
layers that hand an integer or fp16-exact grid on unchanged in every conv mode; in fp32 and f64 mode any grid); above 240
channels the 16-channel fan-out of tests/depthwise_cases.py.  ``L2NormOracleNet`` is ``norm_cases.NormOracleNet`` plus the
layer (``normalize32``).
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import depthwise_cases as D
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC
from tests import norm_cases as N

F32 = np.float32
F64 = np.float64
EPS = 1e-10                      # NormalizeParameter.eps

LAYER_CASES = [
    (512, 3, 5),                 # VGG's conv4_3: 32 lanes of 4 quads
    (256, 2, 3),                 # conv3_3: 16 lanes of 4 quads, four pixels per wave
    (4, 1, 1),                   # one quad, one pixel
    (1, 3, 3),                   # one channel: the scalar form with one lane per pixel
    (5, 7, 9),                   # scalar form, lanes past the pixel's channels
    (6, 7, 9),                   # C % 4 == 2
    (260, 5, 5),                 # 65 quads on 32 lanes: unequal quad counts, 8 register slots for 3
    (1028, 2, 3),                # 257 quads on 64 lanes: past 4 quads per lane, still read once
    (64, 33, 67),                # several blocks, a ragged last pixel group
    (4100, 1, 2),                # 1025 quads: past 64 lanes x 16, the re-reading form
    (1030, 1, 2),                # the scalar form past 64 lanes x 16 channels: it re-reads too
]
MAX_NPL = 16


def case_id(case):
    return "c%d_%dx%d" % tuple(case)


# ---- references ---------------------------------------------------------------------------------------------------------------
def _scale_vec(scale, C, shared):
    s = np.asarray(scale, F32).reshape(-1)
    assert s.size == (1 if shared else C), (s.size, C, shared)
    return np.full(C, s[0], F32) if shared else s


def normalize(x, scale, eps=EPS, shared=False):
    """The layer in binary64 from the fp32 values, unrounded: x (N, C, H, W)."""
    x64 = np.asarray(x, F32).astype(F64)
    S = (x64 * x64).sum(axis=1, keepdims=True)
    norm = np.sqrt(S + F64(F32(eps)))
    return (x64 / norm) * _scale_vec(scale, x64.shape[1], shared).astype(F64).reshape(1, -1, 1, 1)


def form(C, vec=None):
    """(vec, lanes per pixel, items per lane) as the launcher picks them; items per lane 0: the re-reading form (the same
    order over as many items as the pixel has)."""
    vec = C % 4 == 0 if vec is None else vec
    items = C // 4 if vec else C

    def pow2ceil(v):
        r = 1
        while r < v:
            r <<= 1
        return r
    lanes = min(max(pow2ceil((items + 3) // 4), min(pow2ceil(items), 8)), 64)
    need = -(-items // lanes)
    return vec, lanes, (0 if need > MAX_NPL else pow2ceil(need))


def sum_squares32(x, vec=None):
    """The kernel's sum of squares per pixel in its order: x (N, C, H, W) fp32 -> (N, 1, H, W) fp32."""
    x = np.asarray(x, F32)
    n, C, h, w = x.shape
    vec, lanes, _ = form(C, vec)
    V = 4 if vec else 1
    px = x.transpose(0, 2, 3, 1).reshape(-1, C)
    s = np.zeros((px.shape[0], lanes), F32)
    for l in range(lanes):
        acc = np.zeros(px.shape[0], F32)
        for it in range(l, C // V, lanes):
            for e in range(V):
                v = px[:, it * V + e].astype(F64)
                acc = (v * v + acc.astype(F64)).astype(F32)
        s[:, l] = acc
    m = 1
    idx = np.arange(lanes)
    while m < lanes:
        s = (s + s[:, idx ^ m]).astype(F32)
        m <<= 1
    assert (s == s[:, :1]).all() or np.isnan(s).any()        # every lane of the group ends with the same bits
    return s[:, 0].reshape(n, h, w)[:, None]


def normalize32(x, scale, eps=EPS, shared=False, vec=None):
    """The layer in the kernel's fp32 operation order (module docstring)."""
    x = np.asarray(x, F32)
    se = (sum_squares32(x, vec) + F32(eps)).astype(F32)
    norm = np.sqrt(se).astype(F32)
    q = (x / norm).astype(F32)
    return (q * _scale_vec(scale, x.shape[1], shared).reshape(1, -1, 1, 1)).astype(F32)


def bound(ref, C):
    """|got - ref| <= (C / 2 + 4) 2^-24 |ref| + 2^-126 per element: C roundings of the sum, halved by the square root; one
    rounding each for + eps, sqrt, / and *; the last term for subnormal results."""
    return (C / 2.0 + 4.0) * 2.0 ** -24 * np.abs(ref) + 2.0 ** -126


# ---- layer text -------------------------------------------------------------------------------------------------------------
def norm_layer(name, bottom, top=None, shared=False, fill=None, eps=None, across=False, filler=None, pnames=None, extra=""):
    """``across``: False / True as written, None: the field is absent (the proto's default, true).  ``fill``: the value of a
    constant scale_filler; ``filler``: a filler message's text instead.  ``top`` None: in place."""
    f = ""
    if across is not None:
        f += " across_spatial: %s" % ("true" if across else "false")
    f += " channel_shared: %s" % ("true" if shared else "false")
    if filler is not None:
        f += " scale_filler { %s }" % filler
    elif fill is not None:
        f += ' scale_filler { type: "constant" value: %s }' % repr(float(fill))
    if eps is not None:
        f += " eps: %s" % (eps if isinstance(eps, str) else repr(float(eps)))
    par = "".join(' param { name: "%s" }' % p for p in (pnames or []))
    return 'layer { name: "%s" type: "Normalize" bottom: "%s" top: "%s"%s norm_param {%s%s } }\n' % (name, bottom, top or bottom, par, f, extra)


def feeder_txt(C):
    return D.feeder_txt(C)


def layer_net_text(case, shared=False, eps=None, in_place=False, fill=None):
    """`pre` (/ `sel`) -> Normalize `n`, on a top of its own (`n`) or in place on the feeder's blob."""
    C, h, w = case
    txt, bottom = D.feeder_txt(C)
    return H.single_layer_net(txt + norm_layer("n", bottom, None if in_place else "n", shared, fill, eps), D.data_channels(C), h, w)


def out_blob(case, in_place):
    return D.feeder_txt(case[0])[1] if in_place else "n"


def concat_net_text(C, h=7, w=9):
    """`pre` -> `s0`, `s1` (selections of C channels each) -> Concat `cin`; Normalize `n0` on `s0` -> `a`, `n1` on `s1` -> `b`;
    Concat `cat` of `a` and `b`.  `n1` reads the view at channel C of `cin`'s 2 C and writes the view at channel C of `cat`'s
    (C = 12: the vector form on offset views; C = 6: the scalar form)."""
    return H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("s0", "pre", C, 1) + G.conv_txt("s1", "pre", C, 1) +
                              F.concat_layer("cin", ["s0", "s1"]) + norm_layer("n0", "s0", "a") + norm_layer("n1", "s1", "b", eps=0.001) +
                              F.concat_layer("cat", ["a", "b"]), 16, h, w)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def int_inputs(case, shared=False, seed=0):
    """Integers: inputs in [-4, 4], scales in [-3, 3] with a zero among them, pixel (0, 0) all zeros (on a map of more than
    one pixel; the single pixel of a 1 x 1 map gets a nonzero first channel instead).  The sum of squares is at most
    16 C <= 2^17: exact in fp32 in any order."""
    C, h, w = case
    rng = np.random.default_rng(100 * C + 10 * h + w + seed)
    data = rng.integers(-4, 5, (1, D.data_channels(C), h, w)).astype(F32)
    if h * w > 1:
        data[:, :, 0, 0] = 0
    else:
        data[:, :, 0, 0] = np.where(data[:, :, 0, 0] == 0, 3, data[:, :, 0, 0])
    sc = rng.integers(-3, 4, (1 if shared else C,)).astype(F32)
    sc[sc == 0] = 2
    if not shared and C > 1:
        sc[rng.integers(0, C)] = 0
    elif sc[0] == 0:
        sc[0] = -3
    return data, (sc.reshape(()) if shared else sc)


def random_inputs(case, shared=False, seed=0):
    """Normal inputs whose deviation differs per channel by up to 30x (trained-like: a few channels dominate the norm), scales
    around 10 of both signs."""
    C, h, w = case
    rng = np.random.default_rng(7 * C + 3 * h + w + seed)
    cd = D.data_channels(C)
    data = (rng.normal(0, 1, (1, cd, h, w)) * np.exp(rng.uniform(-1.7, 1.7, (1, cd, 1, 1)))).astype(F32)
    sc = (rng.uniform(5, 15, (1 if shared else C,)) * np.where(rng.uniform(0, 1, 1 if shared else C) < 0.2, -1.0, 1.0)).astype(F32)
    return data, (sc.reshape(()) if shared else sc)


def n_params(case, scale):
    """Parameters of `pre` / `sel` / `n`, and the channels of `data` that `n` reads (in n's channel order)."""
    params, perm = D.feeder_params(case[0])
    params["n"] = [np.asarray(scale, F32)]
    return params, perm


# ---- the oracle net -------------------------------------------------------------------------------------------------------------
def norm_spec(L):
    """(shared, eps, filler value) of a Normalize layer message."""
    np_ = L.get("norm_param")
    shared = np_ is None or str(np_.get("channel_shared", "true")) == "true"
    eps = float(np_.get("eps", EPS)) if np_ is not None else EPS
    fill = 1.0
    sf = np_.get("scale_filler") if np_ is not None else None
    if sf is not None and str(sf.get("type", "constant")) == "constant":
        fill = float(sf.get("value", 0.0))
    return shared, eps, fill


def filler_params(msg):
    """{layer name: [scale blob]} of every Normalize layer of ``msg`` as its filler creates it: (C,), or no axes when shared."""
    ch = O.infer_channels(msg)
    out = {}
    for L in msg.getall("layer"):
        if str(L.get("type")) != "Normalize":
            continue
        shared, _, fill = norm_spec(L)
        out[str(L.get("name"))] = [np.full(() if shared else (ch[str(L.get("bottom"))],), fill, F32)]
    return out


class L2NormOracleNet(N.NormOracleNet):
    """``NormOracleNet`` plus Normalize (``normalize32``; an in-place layer replaces its blob)."""

    def forward(self, **kwargs):
        if kwargs:
            assert set(kwargs.keys()) == set(self.inputs)
            for in_, blob in kwargs.items():
                self.blobs[in_].data[...] = blob
        every, snaps = self.layers, {}
        try:
            for L in every:
                t, name = str(L.get("type")), str(L.get("name"))
                if t != "Normalize":
                    self.layers = [L]
                    N.NormOracleNet.forward(self)
                    snaps.update(self.snapshots)
                    continue
                shared, eps, _ = norm_spec(L)
                top = str(L.get("top"))
                out = normalize32(self.blobs[str(L.get("bottom"))].data, self.params[name][0], eps, shared)
                self.blobs[top].data = np.ascontiguousarray(out, dtype=F32)
                snaps[(name, top)] = self.blobs[top].data
        finally:
            self.layers = every
        self.snapshots = snaps
        return {o: self.blobs[o].data for o in self.outputs}


def forwarded(onet, data, info):
    onet.blobs["data"].reshape(*data.shape)
    onet.blobs["im_info"].reshape(*info.shape)
    onet.forward(data=data, im_info=info)
    return onet


# ---- graphs -----------------------------------------------------------------------------------------------------------------
NB_BLOBS = ["c1", "n", "c2", "c2b"]


def neighbours_text(h, w, fill=10.0):
    """Split-fp16 neighbours on the fused path: `c0` (3 -> 64) and `c1` (64 -> 128), 3x3 with ReLU; Normalize `n` of `c1`
    (scale `fill`); `c2`, a 3x3 128-channel family convolution of `n`; `c2b`, another of `c1` itself -- alone it would make
    `c1` a split-format blob, next to the Normalize it reads plain fp32; `H.mini_detector`'s per-blob tail on the two."""
    txt = (G.conv_txt("c0", "data", 64, 3, 1, 1, 1, relu=True) + G.conv_txt("c1", "c0", 128, 3, 1, 1, 1, relu=True) +
           norm_layer("n", "c1", "n", fill=fill) + G.conv_txt("c2", "n", 128, 3, 1, 1, 1, relu=True) +
           G.conv_txt("c2b", "c1", 128, 3, 1, 1, 1, relu=True))
    return H.mini_detector(txt, ["c2", "c2b"], 2, 3, h, w)


def head_text(h, w, fill=10.0):
    """The Normalize top as the head blob of a ProposalLayer: `H.mini_detector`'s 1x1 predictors directly on `n`."""
    txt = (G.conv_txt("c0", "data", 64, 3, 1, 1, 1, relu=True) + G.conv_txt("c1", "c0", 128, 3, 1, 1, 1, relu=True) +
           norm_layer("n", "c1", "n", fill=fill))
    return H.mini_detector(txt, "n", 2, 3, h, w)


def graph_params(msg, seed=5, cls_bias=1.0):
    """``O.synth_params`` plus every Normalize layer's blob from its filler."""
    params = O.synth_params(msg, seed=seed, cls_bias=cls_bias)
    params.update(filler_params(msg))
    return params


S3FD_NORMS = {"f8_norm": ("f8", 10.0), "f16_norm": ("f16", 8.0)}      # layer (= its top) -> (bottom, constant filler)
S3FD_MODULES = dict(G.S3FD_MODULES, **{"8": (["f8_norm"],) + G.S3FD_MODULES["8"][1:], "16": (["f16_norm"],) + G.S3FD_MODULES["16"][1:]})


def s3fd_norm_text(h, w):
    """``general_conv_cases.s3fd_text`` with Normalize on `f8` (constant filler 10) and `f16` (8) in front of their modules;
    the extras go on reading the maps themselves, as S3FD's do."""
    trunk = (G.conv_txt("stem", "data", 64, 7, 2, 3, 1, relu=True) + G.conv_txt("c2", "stem", 64, 3, 1, 1, 1, relu=True) +
             MC._pool("p2", "c2") + G.conv_txt("c3", "p2", 128, 3, 1, 1, 1, relu=True) + G.conv_txt("f8", "c3", 128, 3, 1, 1, 1, relu=True))
    extra = (G.conv_txt("e1a", "f8", 64, 1, relu=True) + G.conv_txt("e1b", "e1a", 128, 3, 2, 1, 1, relu=True, top="f16") +
             G.conv_txt("e2a", "f16", 64, 1, relu=True) + G.conv_txt("e2b", "e2a", 128, 3, 2, 1, 1, relu=True, top="f32"))
    norms = "".join(norm_layer(name, bottom, name, fill=fill) for name, (bottom, fill) in S3FD_NORMS.items())
    tails = "".join(MC.module_tail(m, *S3FD_MODULES[m]) for m in S3FD_MODULES)
    return H.single_layer_net(trunk + extra + norms + tails, 3, h, w)


def s3fd_norm_params():
    return graph_params(P.parse(s3fd_norm_text(*G.S3FD_SIZE)), seed=G.S3FD_SEED, cls_bias=1.0)


def s3fd_norm_oracle(h=G.S3FD_SIZE[0], w=G.S3FD_SIZE[1]):
    return L2NormOracleNet(P.parse(s3fd_norm_text(h, w)), params=s3fd_norm_params(), proposal_cfg=O.ProposalParams(
        pre_nms_topN=10000, score_thresh=G.S3FD_THRESH, min_size=G.S3FD_MIN_SIZE))
