"""Cases of tests/test_gpu_buffer_history.py (GPU) and tests/test_buffer_history_host.py (CPU): one long-lived net per graph
walks sizes A, B, A, C, B and must give at every visit, bit for bit, what a newly constructed net gives at that size.

Every device buffer of the runtime is grow-only (DevBuf, csrc/net_internal.h): a new level shape re-plans sizes and pointers
inside whatever the buffer holds and almost nothing is cleared, so a kernel is right only if it reads no byte that this pass
did not write.  The sequence makes every buffer shrink (A -> B), hold a larger extent than the pass uses (B, then A again),
be reallocated (C: at least 1.3x A's area -- DevBuf allocates 1/8 of slack) and shrink again from the new allocation (C -> B).

Nothing here is a new graph: every key takes its graph, parameters, units and oracle from the family's own case module (or,
where the recipe lives in the family's GPU test module, from there; those modules import without a GPU).

    key             graph                                          A          B          C
    template_dd     helpers.detector_msg(True), seed 7             64 x 96    48 x 64    384 x 704
    template_plain  helpers.detector_msg(False), seed 7            64 x 96    48 x 64    80 x 112
    fam16           test_gpu_fused_forms GRAPHS["fam16"]           128 x 128  37 x 53    128 x 256   (*)
    first           ... ["first"]                                  64 x 64    37 x 53    77 x 75
    heads3          ... ["heads3"]                                 37 x 53    5 x 6      64 x 48     (*)
    dil2            ... ["dil2"]                                   32 x 32    5 x 6      37 x 53
    main_pool       ... ["main_pool"]                              32 x 32    5 x 6      37 x 53
    slim            test_gpu_conv_slim split_128_128_main_pool     9 x 17     8 x 16     23 x 40
    s3fd            general_conv_cases.s3fd_mini                   49 x 80    41 x 63    64 x 96
    mbnet           depthwise_cases.mbnet_mini (folded BN/Scale)   49 x 80    41 x 63    64 x 96
    resblock        norm_cases.resblock                            51 x 79    37 x 53    64 x 96
    s3fd_norm       l2norm_cases.s3fd_norm_text                    49 x 80    41 x 63    64 x 96
    pool_mini       pooling_cases.pool_mini                        49 x 80    41 x 63    64 x 96
    pool_group      pooling_cases.group_net_text                   12 x 5     3 x 5      9 x 13      (*)
    m1              fusion_cases.m1_shaped                         51 x 79    37 x 53    64 x 96
    chain           fusion_cases.chain_text                        51 x 79    37 x 53    64 x 96

The template's Concat layers need sizes that are multiples of 16 (the pyramid pads its levels to them), so its ragged size is
48 x 64: a 6 x 8 map at stride 8, less than one 8 x 16 tile.  Its large size, 384 x 704, is the smallest at which the planner's
cost model moves conv3_2 / conv3_3 (96 x 176 maps, 66 sixteen-row tiles x 2 cout tiles on 256 compute units) from 8-row to
16-row tiles (w4_pick_mt, csrc/conv_f16x3.hip); it stays below the 1008 x 1008 of tests/test_gpu_parity.py.  The four
detector minis share the group sizes (64, 96), (49, 80), (57, 71), none of which is smaller than another in both directions:
A and C are two of them, B = 41 x 63 is new (odd in both directions), and 57 x 71 runs in the grouped passes.  resblock, m1 and
chain have 64 x 96 as the largest size of their own tests, so it is their C; 51 x 79 and 37 x 53 are the two ragged ones.

(*) The sizes these rows must use cannot be ordered strictly in both directions (128 x 128 / 128 x 256; 37 x 53 / 64 x 48;
12 x 5 / 3 x 5 / 9 x 13).  For them B is no larger than A in either direction and smaller in area, and C holds the area rule
alone -- the rule that forces the reallocation (LOOSE).
"""
import numpy as np

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import helpers as H

F32 = np.float32
ACT_TOL = 2e-5
MODES = ("fp32", "f16x3")
EXTRA_MODES = ("bf16", "f64")                       # on EXTRA_KEYS only, and only at A, B, A
EXTRA_KEYS = ("template_dd", "s3fd", "mbnet", "pool_mini")
MODE_WALK = ("fp32", "f16x3", "bf16", "f64", "f16x3", "fp32")       # one net of each EXTRA_KEYS graph at size A
GROUP_KEYS = ("s3fd", "mbnet", "pool_group", "pool_mini")
FORM_KEYS = ("fam16", "slim", "pool_group", "template_dd")          # the sizes must cross a kernel form
LOOSE = ("fam16", "heads3", "pool_group")
MIN_GROWTH = 1.3
DEFAULT_CFG = (0.002, 0.0, 10000)                   # cfg.TEST.SCORE_THRESH, ANCHOR_MIN_SIZE, N_DETS_PER_MODULE


def sequence(sizes):
    a, b, c = sizes
    return [a, b, a, c, b]


def _copy(params):
    return {k: [np.array(v) for v in blobs] for k, blobs in params.items()}


_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


class Case(object):
    """One graph.  `setup(h, w)` -> (prototxt text at that size, a new oracle net holding the parameters, data, im_info)."""

    def __init__(self, key, sizes, blobs, last, cfg=DEFAULT_CFG, fused=False, largest=None, group_sizes=None):
        self.key, self.sizes, self.blobs, self.last, self.cfg, self.fused = key, tuple(sizes), tuple(blobs), tuple(last), cfg, fused
        self.largest = largest or sizes[2]          # (height, width) no size of the graph's own test file exceeds
        self.group_sizes = group_sizes
        self.modes = MODES + (EXTRA_MODES if key in EXTRA_KEYS else ())

    def setup(self, h, w):
        raise NotImplementedError

    def sequence(self, mode):
        s = sequence(self.sizes)
        return s[:3] if mode in EXTRA_MODES else s

    def distinct_sizes(self, mode):
        out = list(dict.fromkeys(self.sequence(mode)))
        if self.group_sizes and mode in MODES:
            out += [s for s in self.group_sizes if s not in out]
        return out

    def oracle(self, h, w):
        """The family's oracle, forwarded on the unit of this size."""
        _, onet, data, info = self.setup(h, w)
        onet.blobs["data"].reshape(*data.shape)
        onet.blobs["im_info"].reshape(*info.shape)
        onet.forward(data=data, im_info=info)
        return onet


def _unit(h, w, seed=4):
    return H.synth_image_blob(h, w, seed=seed + h), np.array([[h - 3, w - 3, 0.75]], F32)


def _pp(cfg):
    return O.ProposalParams(pre_nms_topN=cfg[2], score_thresh=cfg[0], min_size=cfg[1])


class Template(Case):
    def __init__(self, key, dd, sizes):
        Case.__init__(self, key, sizes, ("conv3_3", "conv4_3", "conv5_3", "conv4_fuse_final", "cls_prob_reshape_output", "bbox_pred_output"),
                      ("conv4_fuse_final",), largest=(1008, 1008))
        self.dd = dd

    def setup(self, h, w):
        msg = H.detector_msg(self.dd)
        msg.set_nth("input_shape", 0, P.Msg([("dim", 1), ("dim", 3), ("dim", h), ("dim", w)]))
        params = _once(self.key, lambda: O.synth_params(H.detector_msg(self.dd), seed=7, cls_bias=1.0))
        return (P.dumps(msg), O.OracleNet(msg, params=_copy(params)),) + _unit(h, w)


class FusedForm(Case):
    """A mini-detector of tests/test_gpu_fused_forms.py: random biases, zero predictors, read out through one-hot predictors."""

    def __init__(self, key, sizes, largest):
        from tests import test_gpu_fused_forms as FF
        layers, stack, probe = FF.GRAPHS[key]
        probes = FF._probes(key)
        Case.__init__(self, key, sizes, tuple(stack) + tuple(p for p in probes if p not in stack), probes, fused=True, largest=largest)

    def setup(self, h, w):
        from tests import test_gpu_fused_forms as FF
        layers, stack, probe = FF.GRAPHS[self.key]
        _, onet, data, info = FF._setup(self.key, h, w, 1.0, False)
        return H.mini_detector(layers, probe, 2, 3, h, w), onet, data, info


class Slim(Case):
    NAME = "split_128_128_main_pool_%dx%d"

    def __init__(self, sizes):
        from tests import test_gpu_conv_slim as CS
        _, _, _, _, stack, probes = CS._setup(self.NAME % sizes[0], False)
        Case.__init__(self, "slim", sizes, tuple(stack) + tuple(probes), probes, fused=True, largest=(23, 40))

    def setup(self, h, w):
        from tests import test_gpu_conv_slim as CS
        name = self.NAME % (h, w)
        _, onet, data, info, _, _ = CS._setup(name, False)
        return CS._graph(*CS.CASES[name][:6])[0], onet, data, info


class Mini(Case):
    """A detector mini of a family case module: text(h, w), params(), unit(h, w), oracle net class."""

    def __init__(self, key, sizes, blobs, last, cfg, text, params, unit, net, **kw):
        Case.__init__(self, key, sizes, blobs, last, cfg, **kw)
        self._text, self._params, self._unit, self._net = text, params, unit, net

    def setup(self, h, w):
        text = self._text(h, w)
        params = _once(self.key, self._params)
        onet = self._net(P.parse(text), params=_copy(params), proposal_cfg=_pp(self.cfg))
        return (text, onet) + tuple(self._unit(h, w))


def _cases():
    from tests import depthwise_cases as D
    from tests import fusion_cases as F
    from tests import general_conv_cases as G
    from tests import l2norm_cases as L
    from tests import norm_cases as N
    from tests import pooling_cases as K
    det = [(49, 80), (41, 63), (64, 96)]
    rag = [(51, 79), (37, 53), (64, 96)]
    s3fd_blobs = ("stem", "c2", "p2", "c3", "f8", "e1a", "f16", "e2a", "f32")

    def res_params():
        data, info = H.synth_image_blob(64, 96, seed=4), np.array([[61, 93, 0.75]], F32)
        return N.synth_norm_params(N.resblock(64, 96), data, info, seed=22)

    def chain_params():
        params = O.synth_params(P.parse(F.chain_text(64, 96)), seed=31, cls_bias=1.0)
        params["up"][0][...] = np.random.default_rng(31).normal(0, 0.5, params["up"][0].shape)
        return params

    cs = [
        Template("template_dd", True, [(64, 96), (48, 64), (384, 704)]),
        Template("template_plain", False, [(64, 96), (48, 64), (80, 112)]),
        FusedForm("fam16", [(128, 128), (37, 53), (128, 256)], (128, 256)),
        FusedForm("first", [(64, 64), (37, 53), (77, 75)], (272, 270)),
        FusedForm("heads3", [(37, 53), (5, 6), (64, 48)], (64, 53)),
        FusedForm("dil2", [(32, 32), (5, 6), (37, 53)], (37, 53)),
        FusedForm("main_pool", [(32, 32), (5, 6), (37, 53)], (37, 53)),
        Slim([(9, 17), (8, 16), (23, 40)]),
        Mini("s3fd", det, s3fd_blobs, ("f32",), (G.S3FD_THRESH, G.S3FD_MIN_SIZE, 10000), G.s3fd_text, G.s3fd_params, G.s3fd_unit,
             F.FusionOracleNet, group_sizes=G.S3FD_GROUP_SIZES),
        Mini("mbnet", det, D.MB_BLOBS, ("f16",), (D.MB_THRESH, D.MB_MIN_SIZE, 10000), D.mbnet_text, D.mbnet_params, D.mbnet_unit,
             N.NormOracleNet, group_sizes=D.MB_GROUP_SIZES),
        Mini("resblock", rag, N.RES_BLOBS, (N.RES_PROBE,), (0.5, 3.0, 10000), N.resblock_text, res_params,
             lambda h, w: (H.synth_image_blob(h, w, seed=4), np.array([[h - 3, w - 3, 0.75]], F32)), N.NormOracleNet),
        Mini("s3fd_norm", det, s3fd_blobs + tuple(L.S3FD_NORMS), ("f32",), (G.S3FD_THRESH, G.S3FD_MIN_SIZE, 10000), L.s3fd_norm_text,
             L.s3fd_norm_params, G.s3fd_unit, L.L2NormOracleNet),
        Mini("pool_mini", det, K.PM_BLOBS, ("f16",), (K.PM_THRESH, K.PM_MIN_SIZE, 10000), K.pool_mini_text, K.pool_mini_params,
             K.pool_mini_unit, K.PoolOracleNet, group_sizes=K.PM_GROUP_SIZES),
        Mini("pool_group", [(12, 5), (3, 5), (9, 13)], ("pre", "a1", "a2", "g"), ("a2", "g"), DEFAULT_CFG,
             lambda h, w: K.group_net_text(h, w, C=16), lambda: {"pre": G.feeder_params(16, False)[0]["pre"]},
             lambda h, w: (K.random_grid((1, 16, h, w), seed=h), np.array([[h, w, 1]], F32)), K.PoolOracleNet,
             group_sizes=K.GROUP_SIZES, largest=(12, 13)),
        Mini("m1", rag, ("conv5_128_up", "conv5_128_crop", "conv4_fuse", "m1_3x3", "m1_5x5", "m1_7x7", "m1_out"), ("m1_out",),
             (0.05, 3.0, 10000), lambda h, w: P.dumps(F.m1_shaped(h, w)),
             lambda: O.synth_params(F.m1_shaped(64, 96), seed=22, cls_bias=1.0),
             lambda h, w: (H.synth_image_blob(h, w, seed=4), np.array([[h - 3, w - 3, 0.75]], F32)), F.FusionOracleNet),
        Mini("chain", rag, ("up", "up_crop", "sum", "fuse"), ("fuse",), DEFAULT_CFG, F.chain_text, chain_params,
             lambda h, w: (H.synth_image_blob(h, w, seed=5), np.array([[h, w, 1]], F32)), F.FusionOracleNet, fused=True),
    ]
    return {c.key: c for c in cs}


CASES = _cases()
KEYS = list(CASES)


def slim_plan(h, w):
    """What the planner gives `slim`'s layer under test (128 -> 128, split-format input, fused pool) on an h x w map: its one
    launch's blocks and whether it is the slim form (C ABI shf_debug_conv_plan: nothing is launched, no GPU is needed)."""
    import ctypes as C
    from smallhardface_amd import _lib
    fn = _lib.load(require_gpu=False).shf_debug_conv_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lds, grid, slim = (C.c_longlong * 2)(), (C.c_longlong * 2)(), (C.c_int * 2)()
    assert fn(128, 128, h, w, 1, 1, lds, grid, slim) == 1, _lib.last_error()
    return dict(grid=int(grid[0]), slim=int(slim[0]))


# ---- the other scenarios (tests/test_gpu_buffer_history.py) ---------------------------------------------------------------------
DETECTOR_ORDERS = ("012", "210", "0", "1", "2", "012012")
DETECTOR_SCALES = [100, 300]


def detector_images():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, (80 + 12 * i, 150 - 9 * i, 3)).astype(np.uint8) for i in range(3)]


MULTICLASS_SIZES = [(9, 13), (7, 9)]                 # tests/test_gpu_multiclass_tail.py's own
MULTICLASS_ORDERS = ("01", "10", "0", "1")
MULTICLASS_CFG = dict(pre_nms_topN=40, score_thresh=0.3)
MULTICLASS_THRESH = 0.4
NMS_N = (20000, 30000)                               # tests/test_gpu_parity.py test_nms_vote_large's smallest n; the larger first call


def nms_dets(n):
    """The deterministic boxes of tests/test_gpu_parity.py::test_nms_vote_large."""
    rng = np.random.default_rng(n)
    c = rng.uniform(0, 3000, (n, 2))
    s = rng.uniform(8, 80, (n, 2))
    return np.hstack([c, c + s, rng.uniform(0.05, 1, (n, 1))]).astype(F32)
