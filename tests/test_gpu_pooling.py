"""The Pooling layer beyond MAX on channel quads (csrc/pool.hip: pool_kernel) through caffe.Net, Net.forward and
Net.forward_group (run on an MI355X: ``pytest -m gpu``).  Cases, graphs and references: tests/pooling_cases.py; the references
on their own: tests/test_pooling_host.py.

Without the kernel every test here fails at ``caffe.Net(...)`` ("only MAX pooling is supported", a layer run as 2x2 stride 1) or
at ``forward()`` ("maxpool: channel count / views must be multiples of 4"), the refusals for want of their texts.

1. Windowed cases, fp32 and f16x3, integer and random grids: the top equals ``pool_ref`` bit for bit.  Per-layer path: every
   case as a net without a tail.  Fast path: every geometry at C = 128 with `H.mini_detector`'s tail on the pool's top, read out
   exactly by `H.read_fused_blob` (the read-out needs C % 128 == 0: the ragged channel counts are per-layer only; both paths
   are the same dispatch in `run_pass`).  The scalar form inside a fused pass: a 6-channel pool between 1x1 layers, observed
   through the 128-channel layer behind it (within ACT_TOL of the oracle) and through Blob.data (bit for bit).
2. f64 mode, windowed: bit-equal to ``pool_ref(..., f64=True)``.
3. Global cases: integer grids bit-equal in every form and mode; random grids at or below T bit-equal; above T within
   (L + 2) 2^-24 sum|x| / n of the binary64 mean, L = ``tree_chain(H, W)``; f64 above T within one fp32 ulp of fp32(mean64).
4. The fold: conv + ReLU -> AVE 2x2/2 in f16x3 on the fast path is the average and one `pool_kernel` launch; the MAX twin is
   folded into the convolution as before (no pool launch at all).
5. Views: AVE from a member of one Concat into a member of another, C = 12 (vector form at an offset) and 6 (scalar form); the
   neighbouring member, written by its own producer, is untouched.
6. Grouped pass: three lanes of different sizes, two AVE layers and a global one (windowed on one lane, tree form on two):
   one launch per layer and pass, every member's blobs bit-equal to its own forward.
7. Activation exponent: AVE -> 3x3 convolution in f16x3 with inputs scaled by 2^-20 and 2^10 within ACT_TOL, no fp32 redo.
8. Reshape of a global layer: 7x9, 12x5, 7x9 again; the third forward allocates nothing.
9. `pool_mini` in fp32, f16x3 and f64 against its oracle; forward, forward_group and clone() agree bit for bit.
10. Refusals by layer name; the process stays usable.
11. MAX 2x2/2 with C = 64 and MAX 3x3/2 with C = 8 still run `maxpool_kernel`, one launch per layer and lane.
12. 65 540 output rows (more than one grid's 65 535): the launch goes out as two row ranges, exact on an integer grid.
"""
import numpy as np
import pytest

from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC
from tests import pooling_cases as K

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
ACT_TOL = 2e-5          # tests/test_gpu_parity.py, tests/test_gpu_depthwise.py
SCORE_TOL = 1e-4
BOX_TOL = 1e-3
KERNEL = "pool_kernel"
OLD_KERNEL = "maxpool_kernel"


def _net(text, params):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=text)
    H.load_params(net, params)
    return net


def _info(data):
    return np.array([[data.shape[2], data.shape[3], 1]], F32)


def _forward(net, data, info=None):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {k: np.array(v) for k, v in net.forward(data=data, im_info=_info(data) if info is None else info).items()}


def _blob(net, name):
    return np.array(net.blobs[name].data)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(what))


def _profiled(head, fn):
    head.prof_enable(True)
    head.prof_reset()
    try:
        out = fn()
        prof = {k: int(v["launches"]) for k, v in head.prof_read().items()}
    finally:
        head.prof_enable(False)
        head.prof_reset()
    return out, prof


def _feeder(case):
    from tests import depthwise_cases as D
    return D.feeder_txt(case[0])[1]


# ---- 1. / 2. windowed cases, per-layer path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "random"])
@pytest.mark.parametrize("case", K.WINDOW_CASES, ids=K.case_id)
def test_windowed_cases_per_layer_are_bit_exact(case, kind):
    data = K.case_inputs(case, kind)
    params, perm = K.layer_params(case)
    net = _net(K.layer_net_text(case), params)
    x = data[:, perm]
    want32, _ = K.case_ref(case, x)
    want64, _ = K.case_ref(case, x, f64=True)
    assert np.abs(want32).max() > 0.01
    for mode, want in (("fp32", want32), ("f16x3", want32), ("f64", want64)):
        net.set_conv_mode(mode)
        _, prof = _profiled(net, lambda: _forward(net, data))
        assert prof[KERNEL] == 1 and prof[OLD_KERNEL] == 0, (mode, prof[KERNEL], prof[OLD_KERNEL])
        _same(_blob(net, _feeder(case)), x, (mode, "the feeder"))
        assert tuple(net.blobs["p"].shape) == (K.batch(case), case[0]) + K.case_out_size(case), mode
        _same(_blob(net, "p"), want, (mode, kind, K.case_id(case)))


# ---- 1. the fast path: every geometry at C = 128 behind a proposal tail ----------------------------------------------------------
FAST_CASES = sorted(set((128,) + c[1:] for c in K.WINDOW_CASES + K.GLOBAL_CASES if c[0] == 16))


def _fast_text(case):
    h, w = case[8], case[9]
    return H.mini_detector(G.conv_txt("pre", "data", 128, 1) + K.case_pool_txt(case, "p", "pre"), "p", 2, 128, h, w)


@pytest.mark.parametrize("case", FAST_CASES, ids=K.case_id)
def test_fast_path_is_bit_exact(case):
    from oracle import oracle as O
    text = _fast_text(case)
    msg = P.parse(text)
    params = O.synth_params(msg, seed=3)
    params["pre"] = G.feeder_params(128, False)[0]["pre"]
    onet = K.PoolOracleNet(msg, params={k: [np.array(v) for v in b] for k, b in params.items()})
    net = _net(text, params)
    kinds = ["int"] if K.above_t(case) else ["int", "random"]          # (above T a random grid is held to the bound: test 3)
    for kind in kinds:
        data = K.case_inputs(case, kind)[:1]
        want, _ = K.case_ref(case, data)
        net.set_conv_mode("f16x3")
        redos = net.range_fallbacks
        _, prof = _profiled(net, lambda: _forward(net, data))
        assert prof[KERNEL] == 1 and prof[OLD_KERNEL] == 0 and prof["detect_tail"] >= 1, prof
        got = H.read_fused_blob(net, onet, data, _info(data), mode="f16x3")          # what the FUSED pass left in `p`
        assert net.range_fallbacks == redos
        _same(got[None], want, ("fast", kind, K.case_id(case)))
        _same(_blob(net, "p"), want, ("read back layer by layer", kind))


# ---- 3. global pooling ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.GLOBAL_CASES, ids=K.case_id)
def test_global_cases(case):
    C, method, h, w = case[0], case[1], case[8], case[9]
    params, perm = K.layer_params(case)
    net = _net(K.layer_net_text(case), params)
    n = h * w
    for kind in ("int", "random"):
        data = K.case_inputs(case, kind)
        x = data[:, perm]
        want32, mag = K.case_ref(case, x)
        want64, _ = K.case_ref(case, x, f64=True)
        mean64 = x.astype(F64).sum(axis=(2, 3), keepdims=True) / n
        for mode, want in (("fp32", want32), ("f16x3", want32), ("f64", want64)):
            net.set_conv_mode(mode)
            out, prof = _profiled(net, lambda: _forward(net, data))
            assert prof[KERNEL] == 1 and prof[OLD_KERNEL] == 0, (mode, prof)
            _same(_blob(net, _feeder(case)), x, (mode, "the feeder"))
            got = out["p"]                                               # a (B, C, 1, 1) net output
            assert got.shape == (K.batch(case), C, 1, 1) == tuple(net.blobs["p"].shape)
            what = (mode, kind, K.case_id(case))
            if kind == "int" or method == "MAX" or not K.above_t(case):
                _same(got, want, what)
                continue
            # AVE on a random grid above T: the tree's order is not Caffe's
            if mode == "f64":
                ref = mean64.astype(F32)
                assert (np.abs(got.astype(F64) - ref.astype(F64)) <= np.spacing(np.abs(ref)).astype(F64)).all(), what
                continue
            bound = (K.tree_chain(h, w) + 2) * 2.0 ** -24 * mag / n
            err = np.abs(got.astype(F64) - mean64)
            print("%s %s: max err / bound %.3g, %d of %d differ from the serial order" % (
                K.case_id(case), mode, float((err / np.maximum(bound, 1e-300)).max()), int((got != want32).sum()), got.size))
            assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err - bound).max()))


# ---- 4. the fold ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["AVE", "MAX"])
def test_only_a_max_pool_is_folded_into_the_convolution(method):
    from oracle import oracle as O
    h, w = 9, 12
    text = K.fold_net_text(method, h, w)
    msg = P.parse(text)
    params = O.synth_params(msg, seed=8)
    onet = K.PoolOracleNet(msg, params={k: [np.array(v) for v in b] for k, b in params.items()})
    net = _net(text, params)
    data, info = H.synth_image_blob(h, w, seed=5), np.array([[h, w, 1.0]], F32)
    K.forwarded(onet, data, info)
    want = {k: onet.blobs[k].data.copy() for k in ("c1", "p", "c2")}
    net.set_conv_mode("f16x3")
    _, prof = _profiled(net, lambda: _forward(net, data, info))
    assert prof[KERNEL] == (1 if method == "AVE" else 0) and prof[OLD_KERNEL] == 0, (method, prof[KERNEL], prof[OLD_KERNEL])
    fused_c2 = H.read_fused_blob(net, onet, data, info, mode="f16x3")            # what the fused pass left behind the pool
    e = H.rel_err(fused_c2, want["c2"][0])
    print("fold %s: c2 of the fused pass rel err %.3g" % (method, e))
    assert e < ACT_TOL, (method, e)
    for name in ("c1", "p", "c2"):
        e = H.rel_err(_blob(net, name), want[name])
        assert e < ACT_TOL, (method, name, e)
    c1 = _blob(net, "c1")
    _same(_blob(net, "p"), K.pool_ref(c1, method, 2, 2, 2, 2, 0, 0, False)[0], (method, "p is the pool of c1"))


# ---- 5. views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [12, 6])
def test_concat_members_on_both_sides(C):
    data = K.int_grid((1, 16, 7, 9), seed=12 + C)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    params = {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)]}
    net = _net(K.concat_net_text(C), params)
    wa = K.pool_ref(data[:, p0], "MAX", 3, 3, 2, 2, 1, 1, False)[0]
    for mode in ("fp32", "f16x3", "f64"):
        wb = K.pool_ref(data[:, p1], "AVE", 3, 3, 2, 2, 1, 1, False, f64=mode == "f64")[0]
        net.set_conv_mode(mode)
        _, prof = _profiled(net, lambda: _forward(net, data))
        # C = 12: `m0` is maxpool_kernel's (MAX, square, quads), `p1` the pooling kernel's; C = 6: both are the pooling kernel's
        assert (prof[KERNEL], prof[OLD_KERNEL]) == ((1, 1) if C == 12 else (2, 0)), (mode, prof[KERNEL], prof[OLD_KERNEL])
        _same(_blob(net, "cin"), np.concatenate([data[:, p0], data[:, p1]], axis=1), (mode, "cin"))
        _same(_blob(net, "b"), wb, (mode, "b"))            # read at coff C of cstride 2 C, written at coff C of cstride 2 C
        _same(_blob(net, "a"), wa, (mode, "a: the neighbour is untouched"))
        _same(_blob(net, "cat"), np.concatenate([wa, wb], axis=1), (mode, "cat"))


# ---- 6. the grouped pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f64"])
def test_grouped_pass_is_one_launch_per_layer_and_equals_the_single_forwards(mode):
    C = 16
    root = _net(K.group_net_text(*K.GROUP_SIZES[0], C=C), {"pre": G.feeder_params(C, False)[0]["pre"]})
    lanes = [root.clone() for _ in K.GROUP_SIZES]
    units = [K.random_grid((1, C, h, w), seed=h) for h, w in K.GROUP_SIZES]
    assert [h * w > K.GLOBAL_T for h, w in K.GROUP_SIZES] == [False, True, True]
    root.set_conv_mode(mode)
    try:
        single = []
        for x in units:
            _forward(root, x)
            single.append({k: _blob(root, k) for k in ("a1", "a2", "g")})
        ins = []
        for lane, x in zip(lanes, units):
            lane.blobs["data"].reshape(*x.shape)
            lane.blobs["im_info"].reshape(1, 3)
            ins.append({"data": x, "im_info": _info(x)})
        outs, prof = _profiled(root, lambda: root.forward_group(lanes, ins))
        assert prof[KERNEL] == 3 and prof[OLD_KERNEL] == 0, (prof[KERNEL], prof[OLD_KERNEL])
        for k, (lane, x) in enumerate(zip(lanes, units)):
            for name in ("a1", "a2", "g"):
                _same(_blob(lane, name), single[k][name], (mode, k, name))
            a1 = K.pool_ref(x, "AVE", 2, 2, 2, 2, 0, 0, False, f64=mode == "f64")[0]
            _same(_blob(lane, "a1"), a1, (mode, k, "a1 against the reference"))
            _same(_blob(lane, "a2"), K.pool_ref(a1, "AVE", 3, 3, 1, 1, 1, 1, False, f64=mode == "f64")[0], (mode, k, "a2"))
            assert tuple(lane.blobs["g"].shape) == (1, C, 1, 1)
    finally:
        root.set_conv_mode("fp32")


# ---- 7. the activation exponent -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** 10], ids=["2^-20", "2^10"])
def test_pooled_blob_publishes_its_activation_exponent(scale):
    from oracle import oracle as O
    h, w, C = 9, 11, 64
    text = K.exponent_net_text(h, w, C)
    msg = P.parse(text)
    params = O.synth_params(msg, seed=6)
    params["pre"] = G.feeder_params(C, False)[0]["pre"]
    onet = K.PoolOracleNet(msg, params={k: [np.array(v) for v in b] for k, b in params.items()})
    net = _net(text, params)
    data = (K.random_grid((1, C, h, w), seed=9) * F32(scale)).astype(F32)
    info = _info(data)
    K.forwarded(onet, data, info)
    want = onet.blobs["c"].data.copy()
    assert np.abs(want).max() > 0
    net.set_conv_mode("f16x3")
    redos = net.range_fallbacks
    _, prof = _profiled(net, lambda: _forward(net, data, info))
    assert prof[KERNEL] == 1
    fused = H.read_fused_blob(net, onet, data, info, mode="f16x3")
    e_fused, e_plain = H.rel_err(fused, want[0]), H.rel_err(_blob(net, "c"), want)
    print("exponent %g: max |c| %.3g, rel err fused %.3g, per layer %.3g" % (scale, float(np.abs(want).max()), e_fused, e_plain))
    assert e_fused < ACT_TOL and e_plain < ACT_TOL, (e_fused, e_plain)
    assert net.range_fallbacks == redos == 0


# ---- 8. reshape ---------------------------------------------------------------------------------------------------------------------
def test_a_global_layer_follows_every_reshape_and_allocates_nothing_at_a_seen_size():
    from smallhardface_amd import caffe
    C = 16
    net = _net(K.global_net_text(7, 9, C), {"pre": G.feeder_params(C, False)[0]["pre"]})
    first, second = K.int_grid((1, C, 7, 9), seed=1), K.int_grid((1, C, 12, 5), seed=2)          # (both above T: integer grids are exact)

    def want(x):
        return K.pool_ref(x, "AVE", 0, 0, 1, 1, 0, 0, True)[0]
    _same(_forward(net, first)["p"], want(first), "7 x 9")
    _same(_forward(net, second)["p"], want(second), "12 x 5")
    before = caffe.alloc_counts()
    _same(_forward(net, first)["p"], want(first), "7 x 9 again")
    assert caffe.alloc_counts() == before
    assert tuple(net.blobs["p"].shape) == (1, C, 1, 1) and tuple(net.blobs["pre"].shape) == (1, C, 7, 9)


# ---- 9. the detector ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mini():
    """The net, three lanes of it, and per group size the unit and the oracle's forwarded nets, fp32 and f64 (computed once)."""
    root = _net(K.pool_mini_text(*K.PM_SIZE), K.pool_mini_params())
    lanes = [root.clone() for _ in range(3)]
    units, oracles = [], []
    for h, w in K.PM_GROUP_SIZES:
        data, info = K.pool_mini_unit(h, w)
        units.append((data, info))
        oracles.append(K.forwarded(K.pool_mini_oracle(h, w), data, info))
    oracle64 = K.forwarded(K.pool_mini_oracle(*K.PM_SIZE, f64=True), *units[0])
    return root, lanes, units, oracles, oracle64


@pytest.fixture
def pm_cfg():
    old = (cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE)
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = K.PM_THRESH, K.PM_MIN_SIZE, 10000
    yield
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = old


def _match_rows(gb, gs, ob, os_):
    """tests/test_gpu_modules.py: every row has a partner of the same score (within SCORE_TOL); the largest box difference."""
    worst = 0.0
    for (ab, as_), (bb, bs) in (((gb, gs), (ob, os_)), ((ob, os_), (gb, gs))):
        for i in range(len(as_)):
            near = np.where(np.abs(bs[:, 1] - as_[i, 1]) < SCORE_TOL)[0]
            assert len(near) > 0, (i, as_[i])
            worst = max(worst, float(np.abs(bb[near] - ab[i]).max(axis=1).min()))
    return worst


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f64"])
def test_pool_mini_against_the_oracle(mini, pm_cfg, mode):
    root, lanes, units, oracles, oracle64 = mini
    data, info = units[0]
    onet = oracle64 if mode == "f64" else oracles[0]
    root.set_conv_mode(mode)
    try:
        redos = root.range_fallbacks
        go, prof = _profiled(root, lambda: _forward(root, data, info))
        assert root.range_fallbacks == redos
        # the three AVE layers are the pooling kernel's; `p1` (MAX 3x3/2 pad 1, 32 channels) stays maxpool_kernel's
        assert prof[KERNEL] == len(K.PM_NEW_POOLS) == 3 and prof[OLD_KERNEL] == 1, (prof[KERNEL], prof[OLD_KERNEL])
        for name, hw in K.pool_mini_map_sizes(*K.PM_SIZE).items():
            assert tuple(root.blobs[name].shape)[2:] == hw, name
        assert list(root.blobs.keys()) == list(onet.blobs.keys()) and MC.levels_of(root) == ["16"]
        gb, gs, ob, os_ = go["boxes_16"], go["cls_prob_16"], onet.blobs["boxes_16"].data, onet.blobs["cls_prob_16"].data
        assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 1, (gb.shape, ob.shape)
        ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
        db = _match_rows(gb, gs, ob, os_)
        print("pool_mini %s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (mode, len(gs), ds, db))
        assert ds < SCORE_TOL and db < BOX_TOL, (ds, db)
        for name in K.PM_BLOBS:
            e = H.rel_err(_blob(root, name), onet.blobs[name].data)
            print("pool_mini %s %s: rel err %.3g" % (mode, name, e))
            assert e < ACT_TOL, (name, e)
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_pool_mini_forward_group_and_clone_equal_the_single_forwards(mini, pm_cfg, mode):
    root, lanes, units, oracles, oracle64 = mini
    root.set_conv_mode(mode)
    try:
        single = [_forward(root, x, info) for x, info in units]
        assert all(len(s) == 2 and len(s["cls_prob_16"]) > 1 for s in single)
        ins = []
        for lane, (x, info) in zip(lanes, units):
            lane.blobs["data"].reshape(*x.shape)
            lane.blobs["im_info"].reshape(1, 3)
            ins.append({"data": x, "im_info": info})
        outs, prof = _profiled(root, lambda: root.forward_group(lanes, ins))
        assert prof[KERNEL] == 3 and prof[OLD_KERNEL] == 3, (prof[KERNEL], prof[OLD_KERNEL])       # one per pass; one per lane
        for k, (lane, out) in enumerate(zip(lanes, outs)):
            assert sorted(out.keys()) == sorted(single[k].keys())
            for key in out:
                _same(np.array(out[key]), single[k][key], "unit %d %s" % (k, key))
            assert out["cls_prob_16"].shape == oracles[k].blobs["cls_prob_16"].data.shape, k
            for name in K.PM_NEW_POOLS:
                assert H.rel_err(_blob(lane, name), oracles[k].blobs[name].data) < ACT_TOL, (k, name)
        twin = root.clone()                                                  # a lane on its own
        x, info = units[1]
        for key, v in _forward(twin, x, info).items():
            _same(v, single[1][key], "clone %s" % key)
    finally:
        root.set_conv_mode("fp32")


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------
def _bottoms():
    return G.conv_txt("pre", "data", 16, 1) + G.conv_txt("b0", "pre", 8, 1) + G.conv_txt("b1", "pre", 8, 1)


RESHAPE_3D = 'layer { name: "rs" type: "Reshape" bottom: "b0" top: "rs" reshape_param { shape { dim: 1 dim: -1 dim: 5 } } }\n'
BARE = 'layer { name: "%s" type: "Pooling" %s }\n'

REFUSALS = [
    (K.pool_txt("p_st", "b0", "STOCHASTIC", k=2), r"Pooling 'p_st'.*only MAX and AVE"),
    (K.pool_txt("p_both", "b0", "AVE", k=2, kh=2, kw=2), r"Pooling 'p_both'.*both kernel_size and kernel_h / kernel_w"),
    (K.pool_txt("p_none", "b0", "AVE", stride=2), r"Pooling 'p_none'.*no filter size"),
    (K.pool_txt("p_half", "b0", "AVE", kh=2), r"Pooling 'p_half'.*no filter size"),
    (BARE % ("p_bare", 'bottom: "b0" top: "y"'), r"Pooling 'p_bare'.*no filter size"),
    (K.pool_txt("p_gk", "b0", "AVE", k=2, global_pool=True), r"Pooling 'p_gk'.*global_pooling.*no kernel_size"),
    (K.pool_txt("p_gkh", "b0", "MAX", kh=2, kw=2, global_pool=True), r"Pooling 'p_gkh'.*global_pooling.*no kernel_size"),
    (K.pool_txt("p_gp", "b0", "AVE", pad=1, global_pool=True), r"Pooling 'p_gp'.*global_pooling pad must be 0 and stride 1"),
    (K.pool_txt("p_gs", "b0", "AVE", sh=2, sw=2, global_pool=True), r"Pooling 'p_gs'.*global_pooling pad must be 0 and stride 1"),
    (K.pool_txt("p_pad", "b0", "AVE", k=2, pad=2), r"Pooling 'p_pad'.*pad 2 x 2 must be smaller than the kernel 2 x 2"),
    (K.pool_txt("p_padw", "b0", "MAX", kh=3, kw=1, ph=1, pw=1), r"Pooling 'p_padw'.*pad 1 x 1 must be smaller than the kernel 3 x 1"),
    (K.pool_txt("p_k0", "b0", "AVE", k=0), r"Pooling 'p_k0'.*kernel of 1 \.\. 64"),
    (K.pool_txt("p_k65", "b0", "AVE", kh=65, kw=2), r"Pooling 'p_k65'.*kernel of 1 \.\. 64"),
    (K.pool_txt("p_s0", "b0", "AVE", k=2, stride=0), r"Pooling 'p_s0'.*stride of 1 \.\. 64"),
    (K.pool_txt("p_2pad", "b0", "AVE", k=3, pad=1, ph=1, pw=1), r"Pooling 'p_2pad'.*both pad and pad_h / pad_w"),
    (K.pool_txt("p_2st", "b0", "AVE", k=3, stride=1, sh=1, sw=1), r"Pooling 'p_2st'.*both stride and stride_h / stride_w"),
    (K.pool_txt("p_3d", "rs", "AVE", k=2), r"Pooling 'p_3d'.*'rs' is not 4-D"),
    (K.pool_txt("p_in", "data", "AVE", k=2), r"Pooling 'p_in'.*'data' is a net input.*put a convolution in between"),
    (K.pool_txt("p_flat", "im_info", "AVE", global_pool=True), r"Pooling 'p_flat'.*'im_info' is a net input"),
    (BARE % ("p_bots", 'bottom: "b0" bottom: "b1" top: "y" pooling_param { pool: AVE kernel_size: 2 }'), r"Pooling 'p_bots'.*exactly one bottom and one top"),
    (BARE % ("p_mask", 'bottom: "b0" top: "y" top: "mask" pooling_param { pool: MAX kernel_size: 2 }'), r"Pooling 'p_mask'.*second top 'mask'.*mask"),
    (K.pool_txt("p_place", "b0", "AVE", k=3, stride=1, pad=1, top="b0"), r"Pooling 'p_place'.*cannot run in place on 'b0'"),
    (K.pool_txt("p_big", "b0", "AVE", k=7), r"Pooling 'p_big'.*kernel 7 x 7 exceeds the padded input"),
]


@pytest.mark.parametrize("layers,match", REFUSALS, ids=[m.split("'")[1] for _, m in REFUSALS])
def test_graphs_refused_at_construction_by_layer_name(layers, match):
    from smallhardface_amd import caffe
    txt = H.single_layer_net(_bottoms() + RESHAPE_3D + layers, 16, 3, 5)
    with pytest.raises(Exception, match=match):
        caffe.Net(None, prototxt_text=txt)


def test_a_bottom_of_a_proposal_tail_is_refused_and_the_process_stays_usable():
    from smallhardface_amd import caffe
    txt = H.mini_detector(F.conv_layer("c0", "data", 128, 3, True), "c0", 8, 3, 8, 8) + K.pool_txt("p_tail", "cls_score_output", "AVE", k=2)
    with pytest.raises(Exception, match=r"Pooling 'p_tail'.*'cls_score_output'.*proposal tail"):
        caffe.Net(None, prototxt_text=txt)
    for layers, match in REFUSALS[:3]:
        with pytest.raises(Exception, match=match):
            caffe.Net(None, prototxt_text=H.single_layer_net(_bottoms() + layers, 16, 3, 5))
    case = K.WINDOW_CASES[0]
    data = K.case_inputs(case, "int")
    params, perm = K.layer_params(case)
    net = _net(K.layer_net_text(case), params)
    _same(_forward(net, data)["p"], K.case_ref(case, data[:, perm])[0], "a valid net after the refusals")


# ---- 11. unchanged ground ---------------------------------------------------------------------------------------------------------
def test_max_pools_on_channel_quads_stay_on_maxpool_kernel():
    C = 64
    txt = H.single_layer_net(G.conv_txt("pre", "data", C, 1) + K.pool_txt("m2", "pre", "MAX", k=2, stride=2) + G.conv_txt("s8", "pre", 8, 1) +
                             K.pool_txt("m3", "s8", "MAX", k=3, stride=2), C, 9, 11)
    s8, p8 = G.selection(8, C, seed=5)
    root = _net(txt, {"pre": G.feeder_params(C, False)[0]["pre"], "s8": [s8, np.zeros(8, F32)]})
    lanes = [root.clone() for _ in range(2)]
    from oracle import oracle as O
    for mode in ("fp32", "f16x3", "f64"):
        root.set_conv_mode(mode)
        try:
            x = K.int_grid((1, C, 9, 11), seed=3)
            _, prof = _profiled(root, lambda: _forward(root, x))
            assert prof[OLD_KERNEL] == 2 and prof[KERNEL] == 0, (mode, prof[OLD_KERNEL], prof[KERNEL])      # one per layer
            _same(_blob(root, "m2"), O.max_pool(x, 2, 2, 0), (mode, "m2"))
            _same(_blob(root, "m3"), O.max_pool(x[:, p8], 3, 2, 0), (mode, "m3"))
            ins = []
            for lane, hw in zip(lanes, [(9, 11), (6, 7)]):
                xi = K.int_grid((1, C) + hw, seed=hw[0])
                lane.blobs["data"].reshape(*xi.shape)
                lane.blobs["im_info"].reshape(1, 3)
                ins.append({"data": xi, "im_info": _info(xi)})
            _, prof = _profiled(root, lambda: root.forward_group(lanes, ins))
            assert prof[OLD_KERNEL] == 4 and prof[KERNEL] == 0, (mode, prof[OLD_KERNEL], prof[KERNEL])      # one per layer and lane
            for lane, inp in zip(lanes, ins):
                _same(_blob(lane, "m2"), O.max_pool(inp["data"], 2, 2, 0), (mode, "m2 of a lane"))
        finally:
            root.set_conv_mode("fp32")


# ---- 1b. the scalar form inside a fused pass --------------------------------------------------------------------------------------
def _scalar_fast_text(h, w, method):
    """`pre` (16) -> `sel` (1x1, 6 channels) -> 3x3/2 pad 1 pool `p` of 6 channels (the scalar form) -> `lift` (1x1, 6 -> 128) with
    `H.mini_detector`'s tail: every top is consumed, so a split-fp16 forward takes the fused path with `p` inside it."""
    txt = (G.conv_txt("pre", "data", 16, 1) + G.conv_txt("sel", "pre", 6, 1) + K.pool_txt("p", "sel", method, k=3, stride=2, pad=1) +
           G.conv_txt("lift", "p", 128, 1))
    return H.mini_detector(txt, "lift", 2, 16, h, w)


@pytest.mark.parametrize("method", ["AVE", "MAX"])
def test_scalar_form_inside_a_fused_pass(method):
    """What the FUSED pass left behind the 6-channel pool, read out exactly from `lift` (C = 128), is the oracle's within ACT_TOL
    (a wrong pool is O(1) off); `p` read through Blob.data afterwards is ``pool_ref`` of `sel` bit for bit."""
    from oracle import oracle as O
    h, w = 7, 9
    text = _scalar_fast_text(h, w, method)
    msg = P.parse(text)
    params = O.synth_params(msg, seed=4)
    s6, p6 = G.selection(6, 16, seed=5)
    params["pre"] = G.feeder_params(16, False)[0]["pre"]
    params["sel"] = [s6, np.zeros(6, F32)]
    onet = K.PoolOracleNet(msg, params={k: [np.array(v) for v in b] for k, b in params.items()})
    net = _net(text, params)
    data = K.random_grid((1, 16, h, w), seed=21)
    info = _info(data)
    K.forwarded(onet, data, info)
    want_lift = onet.blobs["lift"].data.copy()
    want_p = K.pool_ref(data[:, p6], method, 3, 3, 2, 2, 1, 1, False)[0]
    net.set_conv_mode("f16x3")
    redos = net.range_fallbacks
    _, prof = _profiled(net, lambda: _forward(net, data, info))
    assert prof[KERNEL] == 1 and prof[OLD_KERNEL] == 0 and prof["detect_tail"] >= 1, (prof[KERNEL], prof[OLD_KERNEL])
    fused = H.read_fused_blob(net, onet, data, info, mode="f16x3")
    e = H.rel_err(fused, want_lift[0])
    print("scalar form in the fused pass, %s: lift rel err %.3g" % (method, e))
    assert e < ACT_TOL and net.range_fallbacks == redos, e
    _same(_blob(net, "sel"), data[:, p6], "sel")
    _same(_blob(net, "p"), want_p, (method, "p through Blob.data"))


# ---- 12. more output rows than one grid holds ---------------------------------------------------------------------------------------
def test_more_rows_than_one_grid_holds():
    """AVE 2 x 1 stride 2 x 1 on a 4-channel map of 131 080 x 1: 65 540 output rows, five more than gridDim.y's 65 535 -- the launch
    goes out as two row ranges.  Integer grid: exact."""
    C, h = 4, 131080
    txt, bottom = G.feeder_txt(C, False)
    net = _net(H.single_layer_net(txt + K.pool_txt("p", bottom, "AVE", kh=2, kw=1, sh=2, sw=1), G.data_channels(C, False), h, 1),
               G.feeder_params(C, False)[0])
    perm = G.feeder_params(C, False)[1]
    data = K.int_grid((1, G.data_channels(C, False), h, 1), seed=8)
    x = data[:, perm]
    want = ((x[:, :, 0::2] + x[:, :, 1::2]) / F32(2)).astype(F32)
    out, prof = _profiled(net, lambda: _forward(net, data))
    assert prof[KERNEL] == 1, prof[KERNEL]
    assert out["p"].shape == (1, C, h // 2, 1) and h // 2 > 65535
    _same(out["p"], want, "65 540 rows")
    np.testing.assert_array_equal(out["p"][0, :, -6:, 0], want[0, :, -6:, 0])          # the rows of the second range
