"""Cases, graphs and references for the Pooling layer beyond MAX on channel quads (csrc/pool.hip: pool_kernel): AVE, global
pooling, rectangular windows, any channel count (tests/test_pooling_host.py, tests/test_gpu_pooling.py).  Everything here runs
without a GPU.

The layer, per channel of a 4-D blob and per output position (oy, ox), along h (the same along w):

    start = oy * stride_h - pad_h
    MAX   end = min(start + kernel_h, H); start = max(start, 0); from -FLT_MAX, ``x > m ? x : m`` in (y, x) order
    AVE   end = min(start + kernel_h, H + pad_h); size = (end_h - start_h) * (end_w - start_w) taken BEFORE the clip to the image
          -- the padding counts in the divisor, what a ceil-sized last window has beyond H + pad does not --; then
          start = max(start, 0), end = min(end, H); an fp32 sum from 0 in (y, x) order; ONE fp32 division by fp32(size)

    output rows = ceil((H + 2 pad_h - kernel_h) / stride_h) + 1, and with a pad on EITHER axis one less on each axis whose last
    window would start at or beyond H + pad (the drop rule).  Global pooling: the window is the whole map, the top (B, C, 1, 1).

``pool_ref`` states that in numpy (``f64``: the AVE sum and the division in binary64, rounded once) and returns the sum of |x|
over each window beside it.  A global layer on more than ``GLOBAL_T`` pixels runs the kernel's tree form, whose additions are
ordered differently (pool.hip): 64 pixel lanes walk the pixels lane, lane + 64, ... with one add chain each, an xor-butterfly
over 16 lanes (4 levels) and a two-level tree over the 4 waves join them.  ``tree_chain(H, W)`` is the longest chain of
additions an input passes through: ceil(H W / 64) + 4 + 2.

A case is ``(C, method, kh, kw, sh, sw, ph, pw, H, W, global)``, each the smallest that exposes one failure mode; ``BATCH``
names the cases that run on two images.  The layer under test is ``p``, behind ``pre`` / ``sel`` of
tests/general_conv_cases.py (1x1 layers that hand an integer or fp16-exact grid on unchanged in every conv mode); above 240
channels the 16-channel fan-out of tests/depthwise_cases.py.

``pool_mini(h, w)``: a detector with every new form on its path.  `stem` 3x3 stride 2 on the image (3 -> 32); `p1` MAX 3x3/2
pad 1 (maxpool_kernel's); a two-layer dense block -- `d1` (3x3, 16) on `p1`, `d2` (3x3, 32) on `cat1` = Concat(`p1`, `d1`) --;
a transition `tr` (1x1, 64) + `tr_pool` AVE 2x2/2; a ResNet-D unit -- `r_main` 3x3 stride 2 against the shortcut `r_avg` AVE
2x2/2 -> `r_sc` 1x1, Eltwise SUM `r_sum`, ReLU --; an Inception pair -- `i_a` 1x1 and `i_avg` AVE 3x3/1 pad 1 -> `i_b` 1x1 --
into Concat `i_cat`; `f16` (3x3, 128) and one ProposalLayer (tests/modules_cases.module_tail) on it.
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import depthwise_cases as D
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC

F32 = np.float32
F64 = np.float64
GLOBAL_T = 16            # pixels up to which a global layer walks its window in Caffe's order (pool.hip kPoolGlobalT)
TREE_LANES = 64          # pixel lanes of the tree form
TREE_LEVELS = 4 + 2      # butterfly levels within a wave (masks 4, 8, 16, 32), then (w0 + w1) + (w2 + w3)

WINDOW_CASES = [
    (16, "AVE", 2, 2, 2, 2, 0, 0, 8, 10, False),
    (16, "AVE", 2, 2, 2, 2, 0, 0, 7, 9, False),        # ceil-sized last window: divisors 2 and 1
    (16, "AVE", 3, 3, 2, 2, 1, 1, 7, 9, False),        # a corner: divisor 9 over 4 values
    (16, "AVE", 3, 3, 2, 2, 1, 1, 8, 10, False),       # the last window reaches one pad row, not two
    (16, "AVE", 2, 2, 2, 2, 1, 1, 3, 5, False),        # the drop rule fires on both axes: 3 x 4 -> 2 x 3
    (16, "AVE", 3, 3, 1, 1, 1, 1, 5, 6, False),        # Inception's
    (16, "AVE", 3, 3, 1, 1, 1, 1, 1, 1, False),        # one value over 9
    (5, "AVE", 3, 3, 2, 2, 0, 0, 7, 9, False),         # the scalar form
    (6, "AVE", 3, 3, 2, 2, 0, 0, 7, 9, False),         # C % 4 == 2
    (6, "MAX", 3, 3, 2, 2, 0, 0, 7, 9, False),         # MAX off the quad grid
    (5, "MAX", 3, 3, 2, 2, 1, 1, 7, 9, False),
    (16, "AVE", 1, 3, 1, 2, 0, 1, 4, 7, False),        # rectangular: 1 x 3, stride 1 x 2, pad 0 x 1
    (16, "MAX", 1, 3, 1, 2, 0, 1, 4, 7, False),
    (16, "AVE", 3, 1, 1, 1, 0, 0, 5, 4, False),        # 3 x 1
    (16, "MAX", 3, 1, 1, 1, 0, 0, 5, 4, False),
    (16, "AVE", 5, 5, 3, 3, 0, 0, 10, 10, False),      # a remainder beyond the last window
    (8, "AVE", 3, 3, 2, 2, 1, 1, 6, 7, False),         # two images (BATCH)
    (64, "AVE", 3, 3, 2, 2, 0, 0, 33, 67, False),      # several blocks both ways
    (260, "AVE", 2, 2, 2, 2, 0, 0, 5, 5, False),       # more quads than a wave, with a remainder
    (260, "MAX", 3, 2, 1, 1, 1, 0, 5, 5, False),       # (rectangular: a square MAX on 260 channels is maxpool_kernel's)
]
BATCH = {(8, "AVE", 3, 3, 2, 2, 1, 1, 6, 7, False): 2, (6, "AVE", 0, 0, 1, 1, 0, 0, 3, 5, True): 2, (16, "AVE", 0, 0, 1, 1, 0, 0, 33, 67, True): 2}
GLOBAL_SIZES = [(1, 1), (3, 5), (4, 4), (3, 6), (7, 7), (33, 67)]     # 4 x 4 = T, 3 x 6 = T + 2; 7 x 7: one pixel per lane; 33 x 67: 35
GLOBAL_CASES = [(C, m, 0, 0, 1, 1, 0, 0, h, w, True) for m in ("AVE", "MAX") for C in (16, 6, 260) for h, w in GLOBAL_SIZES]
ALL_CASES = WINDOW_CASES + GLOBAL_CASES


def case_id(case):
    C, m, kh, kw, sh, sw, ph, pw, h, w, gl = case
    return "c%d_%s_%s_%dx%d" % (C, m, "global" if gl else "k%dx%ds%dx%dp%dx%d" % (kh, kw, sh, sw, ph, pw), h, w)


def batch(case):
    return BATCH.get(tuple(case), 1)


def above_t(case):
    return bool(case[10]) and case[8] * case[9] > GLOBAL_T


def tree_chain(h, w):
    """The longest chain of additions of the tree form on an h x w map: a lane's pixels, then the levels."""
    return -(-(h * w) // TREE_LANES) + TREE_LEVELS


# ---- references ---------------------------------------------------------------------------------------------------------------
def out_size(h, w, kh, kw, sh, sw, ph, pw):
    ho = int(np.ceil((h + 2 * ph - kh) / float(sh))) + 1
    wo = int(np.ceil((w + 2 * pw - kw) / float(sw))) + 1
    if ph or pw:
        if (ho - 1) * sh >= h + ph:
            ho -= 1
        if (wo - 1) * sw >= w + pw:
            wo -= 1
    return ho, wo


def case_out_size(case):
    C, m, kh, kw, sh, sw, ph, pw, h, w, gl = case
    return (1, 1) if gl else out_size(h, w, kh, kw, sh, sw, ph, pw)


def pool_ref(x, method, kh, kw, sh, sw, ph, pw, global_pool, f64=False):
    """(top, sum of |x| over each window) of x (N, C, H, W): the module docstring's formulas, fp32 (``f64``: AVE in binary64,
    rounded once); the second in binary64."""
    x = np.asarray(x, F32)
    n, c, h, w = x.shape
    if global_pool:
        kh, kw, sh, sw, ph, pw = h, w, 1, 1, 0, 0
    ho, wo = out_size(h, w, kh, kw, sh, sw, ph, pw)
    assert ho >= 1 and wo >= 1 and (not global_pool or (ho, wo) == (1, 1))
    ave = method == "AVE"
    assert ave or method == "MAX"
    acc_t = F64 if (ave and f64) else F32
    top = np.zeros((n, c, ho, wo), F32)
    mag = np.zeros((n, c, ho, wo), F64)
    for oy in range(ho):
        for ox in range(wo):
            hs, ws = oy * sh - ph, ox * sw - pw
            if ave:
                he, we = min(hs + kh, h + ph), min(ws + kw, w + pw)
                size = (he - hs) * (we - ws)
                he, we = min(he, h), min(we, w)
            else:
                he, we = min(hs + kh, h), min(ws + kw, w)
            hs, ws = max(hs, 0), max(ws, 0)
            acc = np.zeros((n, c), acc_t) if ave else np.full((n, c), -np.finfo(F32).max, F32)
            for y in range(hs, he):
                for xx in range(ws, we):
                    v = x[:, :, y, xx]
                    if ave:
                        acc = (acc + v.astype(acc_t)).astype(acc_t)
                    else:
                        acc = np.where(v > acc, v, acc)
                    mag[:, :, oy, ox] += np.abs(v.astype(F64))
            if ave:
                assert size >= 1
                acc = (acc / acc_t(size)).astype(acc_t)
            top[:, :, oy, ox] = acc.astype(F32)
    return top, mag


def case_ref(case, x, f64=False):
    C, m, kh, kw, sh, sw, ph, pw, h, w, gl = case
    return pool_ref(x, m, kh, kw, sh, sw, ph, pw, gl, f64)


# ---- layer text -------------------------------------------------------------------------------------------------------------
def pool_txt(name, bottom, method="AVE", k=None, stride=None, pad=None, kh=None, kw=None, sh=None, sw=None, ph=None, pw=None,
             global_pool=False, top=None, extra=""):
    """Only the fields given are written (``k`` / ``stride`` / ``pad``: the square ones)."""
    f = "" if method is None else " pool: %s" % method
    for key, v in (("kernel_size", k), ("stride", stride), ("pad", pad), ("kernel_h", kh), ("kernel_w", kw), ("stride_h", sh),
                   ("stride_w", sw), ("pad_h", ph), ("pad_w", pw)):
        if v is not None:
            f += " %s: %d" % (key, v)
    if global_pool:
        f += " global_pooling: true"
    return 'layer { name: "%s" type: "Pooling" bottom: "%s" top: "%s" pooling_param {%s%s } }\n' % (name, bottom, top or name, f, extra)


def case_pool_txt(case, name, bottom, top=None):
    """The case's layer: the square fields where the geometry is square, the _h / _w fields where it is not."""
    C, m, kh, kw, sh, sw, ph, pw, h, w, gl = case
    if gl:
        return pool_txt(name, bottom, m, global_pool=True, top=top)
    if kh == kw and sh == sw and ph == pw:
        return pool_txt(name, bottom, m, k=kh, stride=sh, pad=ph, top=top)
    return pool_txt(name, bottom, m, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph, pw=pw, top=top)


def layer_net_text(case):
    """`pre` (/ `sel`) -> Pooling `p`."""
    C, h, w = case[0], case[8], case[9]
    txt, bottom = D.feeder_txt(C)
    return H.single_layer_net(txt + case_pool_txt(case, "p", bottom), D.data_channels(C), h, w)


def layer_params(case):
    """Parameters of `pre` / `sel`, and the channels of `data` that `p` reads (in p's channel order)."""
    return D.feeder_params(case[0])


def concat_net_text(C, h=7, w=9):
    """`pre` -> `s0`, `s1` (selections of C channels each) -> Concat `cin`; MAX 3x3/2 pad 1 `m0` on `s0` -> `a`, AVE 3x3/2 pad 1
    `p1` on `s1` -> `b`; Concat `cat` of `a` and `b`.  `p1` reads the view at channel C of `cin`'s 2 C and writes the view at
    channel C of `cat`'s (C = 12: the vector form on offset views; C = 6: the scalar form); `a`, its neighbour in `cat`, has its
    own producer."""
    return H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("s0", "pre", C, 1) + G.conv_txt("s1", "pre", C, 1) +
                              F.concat_layer("cin", ["s0", "s1"]) + pool_txt("m0", "s0", "MAX", k=3, stride=2, pad=1, top="a") +
                              pool_txt("p1", "s1", "AVE", k=3, stride=2, pad=1, top="b") + F.concat_layer("cat", ["a", "b"]), 16, h, w)


def fold_net_text(method, h=9, w=12):
    """`c0` (3 -> 64) and `c1` (64 -> 64), 3x3 with in-place ReLUs -> 2x2/2 pool `p` of `method` -> `c2` (3x3, 128) with
    `H.mini_detector`'s tail, so that a split-fp16 forward takes the fused path: the MAX pool is folded into `c1`'s epilogue
    there (the template's conv1_2 / pool1), the AVE one must not be."""
    txt = (G.conv_txt("c0", "data", 64, 3, 1, 1, 1, relu=True) + G.conv_txt("c1", "c0", 64, 3, 1, 1, 1, relu=True) +
           pool_txt("p", "c1", method, k=2, stride=2) + G.conv_txt("c2", "p", 128, 3, 1, 1, 1, relu=True))
    return H.mini_detector(txt, "c2", 2, 3, h, w)


def exponent_net_text(h=9, w=11, C=64):
    """`pre` -> AVE 3x3/2 pad 1 `p` -> 3x3 "same" convolution `c` (C -> 128), with `H.mini_detector`'s tail on `c`: in f16x3 `c`
    scales its input by the activation exponent that `p`'s launch published."""
    txt = G.conv_txt("pre", "data", C, 1) + pool_txt("p", "pre", "AVE", k=3, stride=2, pad=1) + G.conv_txt("c", "p", 128, 3, 1, 1, 1)
    return H.mini_detector(txt, "c", 2, C, h, w)


def global_net_text(h, w, C=16, method="AVE"):
    """`pre` -> global pooling `p`: a (1, C, 1, 1) net output."""
    return H.single_layer_net(G.conv_txt("pre", "data", C, 1) + pool_txt("p", "pre", method, global_pool=True), C, h, w)


def group_net_text(h, w, C=16):
    """`pre` -> `a1` AVE 2x2/2 -> `a2` AVE 3x3/1 pad 1, and `g` global AVE of `pre`: two windowed layers and a global one."""
    return H.single_layer_net(G.conv_txt("pre", "data", C, 1) + pool_txt("a1", "pre", "AVE", k=2, stride=2) +
                              pool_txt("a2", "a1", "AVE", k=3, stride=1, pad=1) + pool_txt("g", "pre", "AVE", global_pool=True), C, h, w)


GROUP_SIZES = [(3, 5), (12, 5), (9, 13)]      # 15, 60 and 117 pixels: the first lane's global layer walks its window, the others take the tree form


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def int_grid(shape, seed=0):
    """Integers in [-4, 4]: every sum of them is exact in fp32 in any order (at most 4 * 64 * 80 < 2^24)."""
    return np.random.default_rng(seed).integers(-4, 5, shape).astype(F32)


def random_grid(shape, seed=0):
    """Normal values whose deviation differs per channel by up to 30x, as tests/l2norm_cases.py builds them, rounded to fp16
    values (their own high halves: the split-fp16 feeders hand them on unchanged) and flushed to zero below 2^-8."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, shape) * np.exp(rng.uniform(-1.7, 1.7, (shape[0], shape[1], 1, 1)))
    x = x.astype(np.float16).astype(F32)
    x[np.abs(x) < 2.0 ** -8] = 0
    return x


def case_inputs(case, kind, seed=0):
    C, h, w = case[0], case[8], case[9]
    shape = (batch(case), D.data_channels(C), h, w)
    s = 1000 * C + 10 * h + w + seed
    return int_grid(shape, s) if kind == "int" else random_grid(shape, s)


# ---- the oracle net -------------------------------------------------------------------------------------------------------------
def pool_spec(L):
    """(method, kh, kw, sh, sw, ph, pw, global) of a Pooling layer message."""
    q = L.get("pooling_param")
    gi = lambda key, d: int(q.get(key, d))      # noqa: E731
    gl = str(q.get("global_pooling", "false")) == "true"
    if gl:
        return str(q.get("pool", "MAX")), 0, 0, 1, 1, 0, 0, True
    if q.get("kernel_size") is not None:
        kh = kw = gi("kernel_size", 0)
    else:
        kh, kw = gi("kernel_h", 0), gi("kernel_w", 0)
    sh, sw = (gi("stride_h", 1), gi("stride_w", 1)) if q.get("stride") is None else (gi("stride", 1),) * 2
    ph, pw = (gi("pad_h", 0), gi("pad_w", 0)) if q.get("pad") is None else (gi("pad", 0),) * 2
    return str(q.get("pool", "MAX")), kh, kw, sh, sw, ph, pw, False


class PoolOracleNet(F.FusionOracleNet):
    """``FusionOracleNet`` with every Pooling layer computed by ``pool_ref`` (``f64``: its binary64 form)."""

    f64 = False

    def forward(self, **kwargs):
        if kwargs:
            assert set(kwargs.keys()) == set(self.inputs)
            for in_, blob in kwargs.items():
                self.blobs[in_].data[...] = blob
        every, snaps = self.layers, {}
        try:
            for L in every:
                t, name = str(L.get("type")), str(L.get("name"))
                if t != "Pooling":
                    self.layers = [L]
                    F.FusionOracleNet.forward(self)
                    snaps.update(self.snapshots)
                    continue
                top = str(L.get("top"))
                out, _ = pool_ref(self.blobs[str(L.get("bottom"))].data, *pool_spec(L), f64=self.f64)
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


# ---- the detector -------------------------------------------------------------------------------------------------------------
PM_MODULES = {"16": (["f16"], 2, "{'feat_stride': [16,16],'scales': [1,2], 'ratios':[1,]}")}
PM_NEW_POOLS = ("tr_pool", "r_avg", "i_avg")          # pool_kernel's; `p1` stays maxpool_kernel's
PM_BLOBS = ("stem", "p1", "d1", "cat1", "d2", "tr", "tr_pool", "r_main", "r_avg", "r_sc", "r_sum", "i_a", "i_avg", "i_b", "i_cat", "f16")
PM_SIZE = (64, 96)
PM_GROUP_SIZES = [(64, 96), (49, 80), (57, 71)]
PM_SEED, PM_THRESH, PM_MIN_SIZE = 11, 0.5, 0.0


def pool_mini_text(h=PM_SIZE[0], w=PM_SIZE[1]):
    txt = (G.conv_txt("stem", "data", 32, 3, 2, 1, 1, relu=True) + pool_txt("p1", "stem", "MAX", k=3, stride=2, pad=1) +
           G.conv_txt("d1", "p1", 16, 3, 1, 1, 1, relu=True) + F.concat_layer("cat1", ["p1", "d1"]) +
           G.conv_txt("d2", "cat1", 32, 3, 1, 1, 1, relu=True) +
           G.conv_txt("tr", "d2", 64, 1, relu=True) + pool_txt("tr_pool", "tr", "AVE", k=2, stride=2) +
           G.conv_txt("r_main", "tr_pool", 128, 3, 2, 1, 1) + pool_txt("r_avg", "tr_pool", "AVE", k=2, stride=2) +
           G.conv_txt("r_sc", "r_avg", 128, 1) + F.eltwise_layer("r_sum", ["r_main", "r_sc"]) + F.relu_layer("r_sum_relu", "r_sum") +
           G.conv_txt("i_a", "r_sum", 64, 1, relu=True) + pool_txt("i_avg", "r_sum", "AVE", k=3, stride=1, pad=1) +
           G.conv_txt("i_b", "i_avg", 64, 1, relu=True) + F.concat_layer("i_cat", ["i_a", "i_b"]) +
           G.conv_txt("f16", "i_cat", 128, 3, 1, 1, 1, relu=True))
    return H.single_layer_net(txt + "".join(MC.module_tail(m, *PM_MODULES[m]) for m in PM_MODULES), 3, h, w)


def pool_mini(h=PM_SIZE[0], w=PM_SIZE[1]):
    return P.parse(pool_mini_text(h, w))


def pool_mini_params():
    return O.synth_params(pool_mini(), seed=PM_SEED, cls_bias=1.0)


def pool_mini_unit(h, w, seed=4):
    """(data, im_info) of one unit: a synthetic image and an im_info a few pixels inside it."""
    return H.synth_image_blob(h, w, seed=seed + h), np.array([[h - 3, w - 3, 0.75]], F32)


def pool_mini_map_sizes(h, w):
    c = lambda n: -(-n // 2)      # noqa: E731  (a 3x3 stride 2 pad 1 convolution and AVE 2x2/2 both give ceil(n / 2))
    h2, w2 = c(h), c(w)
    h4, w4 = out_size(h2, w2, 3, 3, 2, 2, 1, 1)          # (MAX 3x3/2 pad 1 under ceil sizing: n / 2 + 1 on an even n)
    h8, w8 = c(h4), c(w4)
    return {"stem": (h2, w2), "p1": (h4, w4), "d2": (h4, w4), "tr_pool": (h8, w8), "r_avg": (c(h8), c(w8)), "i_avg": (c(h8), c(w8)),
            "f16": (c(h8), c(w8))}


def pool_mini_oracle(h=PM_SIZE[0], w=PM_SIZE[1], f64=False):
    onet = PoolOracleNet(pool_mini(h, w), params=pool_mini_params(), proposal_cfg=O.ProposalParams(
        pre_nms_topN=10000, score_thresh=PM_THRESH, min_size=PM_MIN_SIZE))
    onet.f64 = f64
    return onet
