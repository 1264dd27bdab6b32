"""The depthwise convolution (csrc/conv_dw.hip: conv_dw_kernel) through caffe.Net, Net.forward and Net.forward_group (run on
an MI355X: ``pytest -m gpu``).  Cases, graphs and references: tests/depthwise_cases.py; the references on their own:
tests/test_depthwise_host.py.

Without the kernel and its dispatch every test here fails at ``caffe.Net(...)`` ("group != 1 unsupported"), the refusals for
want of their new texts.

1. Every layer case, with and without bias and in-place ReLU, on integer grids in conv modes fp32, f16x3, bf16 and f64 on the
   per-layer path: equal to `O.convolution(group=Cin)`, element for element; shapes from the C side.
2. Every layer case on random grids: fp32 and f16x3 within ACT_TOL of the oracle; f64 within the per-element bound of
   tests/test_gpu_f64_mode.py, ulp32(ref) + 2 (K + 1) 2^-53 sum |a w| with K = k k.
3. Bit-identity with the dense form: `g` and `g_dense` (group 1, block-diagonal weights, the general-geometry kernel) in one
   net are equal bit for bit in fp32 mode.
4. Concat views: two depthwise layers write one Concat, 12 channels each (vector form at coff 12 of cstride 24) and 6 each
   (scalar form); exact on integer grids in the four modes.
5. Fold: dw + BatchNorm + Scale (+ ReLU) is bit-equal to the bare layer with `norm_cases.fold` of the blobs, one launch of the
   new class and no channel_affine launch; Net.params keeps the unfolded blobs; a BatchNorm commit is followed.
6. Split-fp16 neighbours on the fused path: within ACT_TOL; with an output of magnitude 1e3 (the published exponent); with a
   9-tap sum beyond the fp16 range (the range flag: one fp32 redo, blobs equal fp32 mode's).
7. The MobileNet-shaped detector against `NormOracleNet`, its boxes, forward_group over three lanes, the profiler's count.
8. Refusals by layer name, a refused reshape, a caffemodel with the dense blob count.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import depthwise_cases as D
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC
from tests import norm_cases as N

pytestmark = pytest.mark.gpu

F32 = np.float32
ACT_TOL = 2e-5          # tests/test_gpu_parity.py
SCORE_TOL = 1e-4
BOX_TOL = 1e-3
EXACT_MODES = ["fp32", "f16x3", "bf16", "f64"]
KERNEL = "conv_dw_kernel"
AFFINE = "channel_affine"
INFO = np.array([[8, 8, 1]], F32)


def _net(text, params):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=text)
    H.load_params(net, params)
    return net


def _forward(net, data, info=INFO):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {k: np.array(v) for k, v in net.forward(data=data, im_info=info).items()}


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


# ---- 1. integer grids: exact in every mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias,relu", D.VARIANTS, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("case", D.LAYER_CASES, ids=D.case_id)
def test_integer_grids_are_exact_in_every_mode(case, bias, relu):
    data, wt, bs = D.int_inputs(case, bias)
    params, perm = D.g_params(case, wt, bs)
    net = _net(D.layer_net_text(case, bias, relu), params)
    want = D.oracle_layer(case, data[:, perm], wt, bs, relu)
    assert relu or (want < 0).any()
    for mode in EXACT_MODES:
        net.set_conv_mode(mode)
        _forward(net, data)
        got = _blob(net, "g")
        assert tuple(net.blobs["g"].shape) == want.shape == (1, D.cout(case)) + D.out_size(case), mode
        np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=mode)
        np.testing.assert_array_equal(_blob(net, D.feeder_txt(case[0])[1]), data[:, perm], err_msg=mode)


# ---- 2. random grids ----------------------------------------------------------------------------------------------------------
def _assert_within_f64_bound(got, ref, mag, K, relu, what):
    """tests/test_gpu_f64_mode.py: |got - fl32(ref)| <= ulp32(ref) + 2 (K + 1) 2^-53 sum |a w| for every element."""
    r32 = ref.astype(F32)
    bound = np.spacing(np.abs(r32)).astype(np.float64) + 2.0 * (K + 1) * 2.0 ** -53 * mag
    want = np.maximum(r32, 0) if relu else r32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = int(np.argmax(err - bound))
    print("%s: K %d, %d elements, %d not bit-equal to fl32(ref), max err %.3e (bound there %.3e)"
          % (what, K, err.size, int((got != want).sum()), float(err.flat[worst]), float(bound.flat[worst])))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (err <= bound).all(), (what, float(err.flat[worst]), float(bound.flat[worst]))


@pytest.mark.parametrize("bias,relu", [(True, True), (False, False)], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("case", D.LAYER_CASES, ids=D.case_id)
def test_random_grids_against_the_oracle(case, bias, relu):
    cin, m, k, s, p, d, h, w = case
    data, wt, bs = D.random_inputs(case, bias)
    params, perm = D.g_params(case, wt, bs)
    net = _net(D.layer_net_text(case, bias, relu), params)
    x = data[:, perm]
    want = D.oracle_layer(case, x, wt, bs, relu)
    for mode in ("fp32", "f16x3"):
        net.set_conv_mode(mode)
        _forward(net, data)
        e = H.rel_err(_blob(net, "g"), want)
        print("%s %s: rel err %.3g" % (D.case_id(case), mode, e))
        assert e < ACT_TOL, (mode, e)
    net.set_conv_mode("f64")
    _forward(net, data)
    ref, mag = D.naive_depthwise(x[0], wt, bs, s, p, d, m)
    _assert_within_f64_bound(_blob(net, "g")[0], ref, mag, k * k, relu, D.case_id(case))


# ---- 3. bit-identity with the dense form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias,relu", [(True, True), (False, False)], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("case", D.DENSE_TWIN_CASES, ids=D.case_id)
def test_bit_identical_to_the_dense_form_on_the_general_kernel(case, bias, relu):
    data, wt, bs = D.random_inputs(case, bias, seed=3)
    params, perm = D.g_params(case, wt, bs, dense_twin=True)
    net = _net(D.layer_net_text(case, bias, relu, dense_twin=True), params)
    net.set_conv_mode("fp32")
    _, prof = _profiled(net, lambda: _forward(net, data))
    assert prof[KERNEL] == 1 and prof["conv_mfma_gen_kernel"] == 1, prof
    got, dense = _blob(net, "g"), _blob(net, "g_dense")
    assert np.abs(dense).max() > 0.1
    _same(got, dense, D.case_id(case))


# ---- 4. Concat views --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [12, 6])
def test_concat_members_are_exact(C):
    rng = np.random.default_rng(12 + C)
    data = rng.integers(-4, 5, (1, 16, 7, 9)).astype(F32)
    sel, perm = G.selection(C, 16)
    params = {"pre": G.feeder_params(16, False)[0]["pre"], "sel": [sel, np.zeros(C, F32)]}
    for name, k in (("g0", 3), ("g1", 5)):
        params[name] = [rng.integers(-2, 3, (C, 1, k, k)).astype(F32), rng.integers(-8, 9, (C,)).astype(F32)]
    net = _net(D.concat_net_text(C), params)
    x = data[:, perm]
    w0 = np.maximum(O.convolution(x, params["g0"][0], params["g0"][1], pad=1, group=C), 0)
    w1 = O.convolution(x, params["g1"][0], params["g1"][1], pad=2, group=C)
    assert (w1 < 0).any()
    for mode in EXACT_MODES:
        net.set_conv_mode(mode)
        _forward(net, data)
        np.testing.assert_array_equal(_blob(net, "g1"), w1, err_msg=mode)     # the view at coff C of cstride 2 C
        np.testing.assert_array_equal(_blob(net, "g0"), w0, err_msg=mode)
        np.testing.assert_array_equal(_blob(net, "cat"), np.concatenate([w0, w1], axis=1), err_msg=mode)


# ---- 5. the fold -----------------------------------------------------------------------------------------------------------------
def _oracle(msg, params, data):
    onet = N.NormOracleNet(msg, params=params)
    return D.forwarded(onet, data, np.array([[data.shape[2], data.shape[3], 1]], F32))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("C", [32, 5])
def test_fold_equals_the_bare_layer_with_folded_blobs(C, bias, relu):
    msg_a, pa, msg_b, pb, data = D.fold_pair(C, bias, relu)
    a, b = _net(P.dumps(msg_a), pa), _net(P.dumps(msg_b), pb)
    want = _oracle(msg_a, pa, data).blobs["g"].data
    assert len(a.params["g"]) == (2 if bias else 1) and len(b.params["g"]) == 2
    for mode in ("fp32", "f16x3", "f64"):
        a.set_conv_mode(mode)
        b.set_conv_mode(mode)
        oa, prof = _profiled(a, lambda: _forward(a, data))
        ob = _forward(b, data)
        assert prof[KERNEL] == 1 and prof[AFFINE] == 0, (mode, prof[KERNEL], prof[AFFINE])
        _same(oa["g"], ob["g"], (C, mode))
        _same(_blob(a, "g"), _blob(b, "g"), (C, mode, "blob"))
        err = H.rel_err(oa["g"], want)
        print("fold C %d %s: rel_err %.3g" % (C, mode, err))
        assert err < ACT_TOL, (C, mode, err)
        assert relu or (oa["g"] < 0).any()
    # Net.params keeps Caffe's unfolded blobs
    _same(np.array(a.params["g"][0].data), pa["g"][0], "unfolded weights")
    # a BatchNorm commit re-folds and re-packs: the output follows
    a.set_conv_mode("fp32")
    first = _forward(a, data)["g"]
    p2 = {k: [np.array(v) for v in blobs] for k, blobs in pa.items()}
    pre_bn = _oracle(msg_a, pa, data).snapshots[("g", "g")]
    p2["g_bn"] = N.norm_blobs("BatchNorm", pre_bn, np.random.default_rng(8), factor=37.5)
    for i, arr in enumerate(p2["g_bn"]):
        a.params["g_bn"][i].data[...] = arr
    a.commit_params()
    second, prof = _profiled(a, lambda: _forward(a, data)["g"])
    assert prof[KERNEL] == 1 and prof[AFFINE] == 0 and H.rel_err(second, first) > 1e-3
    fresh = _net(P.dumps(msg_a), p2)
    _same(second, _forward(fresh, data)["g"], "new statistics")
    assert H.rel_err(second, _oracle(msg_a, p2, data).blobs["g"].data) < ACT_TOL


# ---- 6. split-fp16 neighbours on the fused path -------------------------------------------------------------------------------
NB_HW = (13, 19)


def _neighbours():
    msg = P.parse(D.neighbours_text(*NB_HW))
    params = O.synth_params(msg, seed=5, cls_bias=1.0)
    data, info = H.synth_image_blob(*NB_HW, seed=3), np.array([[NB_HW[0], NB_HW[1], 1.0]], F32)
    return msg, params, data, info


def _check_neighbours(msg, params, data, info, what):
    onet = G.FusionOracleNet(msg, params={k: [np.array(v) for v in b] for k, b in params.items()})
    gnet = _net(P.dumps(msg), params)
    gnet.set_conv_mode("f16x3")
    redos = gnet.range_fallbacks
    H.run_both(gnet, onet, data, info)
    assert tuple(gnet.blobs["dw"].shape) == (1, 64) + NB_HW == onet.blobs["dw"].data.shape
    mags = {}
    for name in D.NEIGHBOUR_BLOBS:
        e = H.rel_err(_blob(gnet, name), onet.blobs[name].data)
        mags[name] = float(np.abs(onet.blobs[name].data).max())
        print("%s %s: max %.3g, rel err %.3g" % (what, name, mags[name], e))
        assert e < ACT_TOL, (what, name, e)
    # what the FUSED pass itself left in the last map (the blobs above are re-run layer by layer when read)
    want = onet.blobs["c3"].data[0].copy()
    fused = H.read_fused_blob(gnet, onet, data, info, mode="f16x3")
    e = H.rel_err(fused, want)
    print("%s c3 of the fused pass: rel err %.3g" % (what, e))
    assert e < ACT_TOL, (what, e)
    assert gnet.range_fallbacks == redos
    return mags


def test_split_fp16_neighbours_on_the_fused_path():
    _check_neighbours(*_neighbours(), "neighbours")


def test_split_fp16_neighbours_with_a_large_depthwise_output():
    """The depthwise weights scaled so that its output is of magnitude 1e3 (the 1x1 behind scaled back): the GEMM kernel
    lifts its input by the exponent the depthwise launch published."""
    msg, params, data, info = _neighbours()
    onet = D.forwarded(G.FusionOracleNet(msg, params=params), data, info)
    s = F32(1e3 / np.abs(onet.blobs["dw"].data).max())
    params["dw"][0] = (params["dw"][0] * s).astype(F32)
    params["pw"][0] = (params["pw"][0] / s).astype(F32)
    mags = _check_neighbours(msg, params, data, info, "neighbours x1e3")
    assert 900 < mags["dw"] < 1100 and mags["pw"] < 100


def test_a_tap_sum_beyond_the_fp16_range_redoes_the_forward_in_fp32():
    """c1 gives 3e4 everywhere (zero weights, bias 3e4), the depthwise weights are 1: every input is inside the fp16 range, the
    9-tap sum (2.7e5) outside it.  The depthwise launch raises the range flag, the forward is redone on the fp32 kernels."""
    msg, params, data, info = _neighbours()
    params["c1"][0][...] = 0
    params["c1"][1][...] = 3e4
    params["dw"][0][...] = 1
    params["dw"][1][...] = 0
    params["pw"][0] = (params["pw"][0] * F32(2.0 ** -14)).astype(F32)
    onet = D.forwarded(G.FusionOracleNet(msg, params=params), data, info)
    m = {k: float(np.abs(onet.blobs[k].data).max()) for k in D.NEIGHBOUR_BLOBS}
    print(m)
    assert m["c1"] == 3e4 and m["dw"] == 2.7e5 and m["pw"] < 1000 and m["c3"] < 1000
    gnet, fnet = _net(P.dumps(msg), params), _net(P.dumps(msg), params)
    gnet.set_conv_mode("f16x3")
    fnet.set_conv_mode("fp32")
    before = gnet.range_fallbacks
    (go, _), prof = _profiled(gnet, lambda: H.run_both(gnet, onet, data, info))
    fo = _forward(fnet, data, info)
    assert gnet.range_fallbacks == before + 1 and fnet.range_fallbacks == 0
    assert prof[KERNEL] == 2, prof[KERNEL]          # the launch, and once more in the fp32 redo
    for key in fo:
        _same(np.array(go[key]), fo[key], key)
    for name in D.NEIGHBOUR_BLOBS:
        _same(_blob(gnet, name), _blob(fnet, name), name)
        assert H.rel_err(_blob(gnet, name), onet.blobs[name].data) < ACT_TOL, name


# ---- 7. the MobileNet-shaped detector -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mbnet():
    """The net, three lanes of it, and per group size the unit and the oracle's forwarded net (computed once)."""
    root = _net(D.mbnet_text(*D.MB_SIZE), D.mbnet_params())
    lanes = [root.clone() for _ in range(3)]
    units, oracles = [], []
    for h, w in D.MB_GROUP_SIZES:
        data, info = D.mbnet_unit(h, w)
        units.append((data, info))
        oracles.append(D.forwarded(D.mbnet_oracle(h, w), data, info))
    return root, lanes, units, oracles


@pytest.fixture
def mb_cfg():
    old = (cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE)
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = D.MB_THRESH, D.MB_MIN_SIZE, 10000
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


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_mbnet_against_the_oracle(mbnet, mb_cfg, mode):
    root, lanes, units, oracles = mbnet
    data, info = units[0]
    onet = oracles[0]
    root.set_conv_mode(mode)
    try:
        redos = root.range_fallbacks
        go, prof = _profiled(root, lambda: _forward(root, data, info))
        assert root.range_fallbacks == redos
        assert prof[KERNEL] == len(D.MB_DW_LAYERS) and prof[AFFINE] == 0, (prof[KERNEL], prof[AFFINE])
        for name, hw in D.mbnet_map_sizes(*D.MB_SIZE).items():     # (blob shapes come from the C side)
            assert tuple(root.blobs[name].shape)[2:] == hw, name
        assert list(root.blobs.keys()) == list(onet.blobs.keys()) and MC.levels_of(root) == ["8", "16"]
        for m in D.MB_MODULES:
            gb, gs, ob, os_ = go["boxes_" + m], go["cls_prob_" + m], onet.blobs["boxes_" + m].data, onet.blobs["cls_prob_" + m].data
            assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 1, (m, gb.shape, ob.shape)
            ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
            db = _match_rows(gb, gs, ob, os_)
            print("mbnet %s module %s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (mode, m, len(gs), ds, db))
            assert ds < SCORE_TOL and db < BOX_TOL, (m, ds, db)
        for name in D.MB_BLOBS:
            e = H.rel_err(_blob(root, name), onet.blobs[name].data)
            print("mbnet %s %s: rel err %.3g" % (mode, name, e))
            assert e < ACT_TOL, (name, e)
    finally:
        root.set_conv_mode("fp32")


def _stage_group(lanes, units):
    ins = []
    for lane, (x, info) in zip(lanes, units):
        lane.blobs["data"].reshape(*x.shape)
        lane.blobs["im_info"].reshape(1, 3)
        ins.append({"data": x, "im_info": info})
    return ins


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_mbnet_forward_group_equals_the_units_one_at_a_time(mbnet, mb_cfg, mode):
    root, lanes, units, oracles = mbnet
    root.set_conv_mode(mode)
    try:
        single = [_forward(root, x, info) for x, info in units]
        assert all(len(s) == 4 and len(s["cls_prob_8"]) > 1 for s in single)
        outs = root.forward_group(lanes, _stage_group(lanes, units))
        for k, (lane, out) in enumerate(zip(lanes, outs)):
            assert sorted(out.keys()) == sorted(single[k].keys())
            for key in out:
                _same(np.array(out[key]), single[k][key], "unit %d %s" % (k, key))
            for m in D.MB_MODULES:
                assert out["cls_prob_" + m].shape == oracles[k].blobs["cls_prob_" + m].data.shape, (k, m)
            e = H.rel_err(_blob(lane, "f16"), oracles[k].blobs["f16"].data)
            assert e < ACT_TOL, (k, e)
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f64"])
def test_profiler_books_five_launches_per_pass_for_a_group(mbnet, mb_cfg, mode):
    root, lanes, units, oracles = mbnet
    ins = _stage_group(lanes, units)
    root.set_conv_mode(mode)
    try:
        root.forward_group(lanes, ins)
        redos = root.range_fallbacks
        root.prof_enable(True)
        root.prof_reset()
        root.forward_group(lanes, ins)
        prof = root.prof_read()
        assert root.range_fallbacks == redos
        assert int(prof[KERNEL]["launches"]) == len(D.MB_DW_LAYERS) == 5, prof[KERNEL]
        assert int(prof[AFFINE]["launches"]) == 0 and prof[KERNEL]["flops"] > 0
    finally:
        root.prof_enable(False)
        root.set_conv_mode("fp32")


def test_profiler_books_none_for_a_graph_without_depthwise_layers():
    net = _net(G.s3fd_text(*G.S3FD_SIZE), G.s3fd_params())
    data, info = G.s3fd_unit(*G.S3FD_SIZE)
    _forward(net, data, info)
    _, prof = _profiled(net, lambda: _forward(net, data, info))
    assert KERNEL in prof and prof[KERNEL] == 0
    assert prof["conv_mfma_gen_kernel"] == len(G.S3FD_GENERAL_LAYERS)


# ---- 8. refusals and survival -----------------------------------------------------------------------------------------------------
def test_refusals_at_construction():
    from smallhardface_amd import caffe
    pre = G.conv_txt("pre", "data", 16, 1)
    # a group that is not the bottom's channel count
    with pytest.raises(RuntimeError, match=r"Convolution 'g': group != 1 unsupported unless depthwise \(group == bottom channels\); got group 2 of 16"):
        caffe.Net(None, prototxt_text=H.single_layer_net(pre + G.conv_txt("g", "pre", 16, 3, 2, 1, 1, group=2), 16, 8, 8))
    with pytest.raises(RuntimeError, match=r"Convolution 'g': group != 1 unsupported unless depthwise .*got group 8 of 16"):
        caffe.Net(None, prototxt_text=H.single_layer_net(pre + G.conv_txt("g", "pre", 16, 3, 1, 1, 1, group=8), 16, 8, 8))
    # on the NCHW net input
    with pytest.raises(RuntimeError, match=r"Convolution 'g': depthwise .*bottom 'data', a net input.*put a convolution in between"):
        caffe.Net(None, prototxt_text=H.single_layer_net(D.dw_txt("g", "data", 16, 1, 3, 1, 1, 1), 16, 8, 8))
    # as a predictor of a proposal tail: a 4-channel head, A = 2, class predictor with group 4
    pstr = "{'feat_stride': [8,8],'scales': [1,2], 'ratios':[1,]}"
    tail = MC.module_tail("8", ["f"], 2, pstr)
    dense = "num_output: 4 kernel_size: 1 pad: 0 stride: 1"
    assert tail.count(dense) == 1
    txt = pre + G.conv_txt("f", "pre", 4, 1)
    caffe.Net(None, prototxt_text=H.single_layer_net(txt + tail, 16, 8, 8))          # (the dense predictor loads)
    with pytest.raises(RuntimeError, match=r"Convolution 'cls_score_m8': depthwise .*predictor of ProposalLayer 'proposal_m8'"):
        caffe.Net(None, prototxt_text=H.single_layer_net(txt + tail.replace(dense, dense + " group: 4"), 16, 8, 8))
    # a kernel extent beyond the padded input
    with pytest.raises(RuntimeError, match=r"Convolution 'g': kernel extent 5 .*padded input 4 x 8"):
        caffe.Net(None, prototxt_text=H.single_layer_net(pre + D.dw_txt("g", "pre", 16, 1, 5, 1, 0, 1), 16, 4, 8))
    net = caffe.Net(None, prototxt_text=H.single_layer_net(pre + D.dw_txt("g", "pre", 16, 2, 5, 1, 0, 1), 16, 5, 8))
    assert tuple(net.blobs["g"].shape) == (1, 32, 1, 4)


def test_a_refused_reshape_leaves_the_net_usable():
    case = (16, 1, 3, 1, 0, 1, 5, 6)
    data, wt, bs = D.int_inputs(case, True)
    params, perm = D.g_params(case, wt, bs)
    net = _net(D.layer_net_text(case), params)
    want = D.oracle_layer(case, data, wt, bs, False)
    np.testing.assert_array_equal(_forward(net, data)["g"], want)
    small = np.zeros((1, 16, 2, 6), F32)
    for _ in range(2):
        with pytest.raises(RuntimeError, match=r"Convolution 'g': kernel extent 3 .*padded input 2 x 6"):
            _forward(net, small)
    # back at the size of the last good forward, and at a new one
    np.testing.assert_array_equal(_forward(net, data)["g"], want)
    assert tuple(net.blobs["g"].shape) == (1, 16, 3, 4)
    big = np.random.default_rng(1).integers(-4, 5, (1, 16, 7, 9)).astype(F32)
    np.testing.assert_array_equal(_forward(net, big)["g"], D.oracle_layer((16, 1, 3, 1, 0, 1, 7, 9), big, wt, bs, False))


def test_caffemodel_with_the_dense_blob_count_is_refused(tmp_path):
    from smallhardface_amd import caffe, caffemodel
    case = (16, 1, 3, 1, 1, 1, 5, 6)
    data, wt, bs = D.int_inputs(case, True)
    params, perm = D.g_params(case, wt, bs)
    txt = D.layer_net_text(case)
    path = caffemodel.write_caffemodel(str(tmp_path / "dw.caffemodel"), params)
    loaded = caffe.Net(None, path, caffe.TEST, prototxt_text=txt)
    assert tuple(loaded.params["g"][0].data.shape) == (16, 1, 3, 3)
    np.testing.assert_array_equal(_forward(loaded, data)["g"], D.oracle_layer(case, data, wt, bs, False))
    bad = dict(params, g=[D.dense_weights(wt, 16, 1), bs])
    caffemodel.write_caffemodel(str(tmp_path / "dense.caffemodel"), bad)
    with pytest.raises(Exception, match=r"Cannot copy param 0 weights from layer 'g'; shape mismatch"):
        caffe.Net(None, str(tmp_path / "dense.caffemodel"), caffe.TEST, prototxt_text=txt)
