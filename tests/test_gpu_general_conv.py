"""The general-geometry convolution (csrc/conv_gen.h: conv_mfma_gen_kernel) through caffe.Net, Net.forward and
Net.forward_group (run on an MI355X: ``pytest -m gpu``).  Cases, graphs and references: tests/general_conv_cases.py; the
references on their own: tests/test_general_conv_host.py.

Without the kernel and its dispatch every test here but item 7 fails: at ``caffe.Net(...)`` ("stride != 1 unsupported", "only
3x3 pad==dilation and 1x1 pad 0 are supported"), or for want of the profiler class.

1. Every layer case, with and without bias and in-place ReLU, on integer grids in conv modes fp32, f16x3, bf16 and f64
   through Net.forward on the per-layer path: equal to `O.convolution`, element for element.  The Concat case likewise.
2. Every layer case on random grids: fp32 and f16x3 within ACT_TOL of the oracle; f64 within the per-element bound of
   tests/test_gpu_f64_mode.py (one fp32 rounding + the binary64 sum's 2 (K + 1) 2^-53 sum |a w|).
3. Split-format neighbours on the fused path (f16x3): every blob within ACT_TOL, the fused pass's own last map through the
   tail's read-out, range_fallbacks unchanged.
4. The S3FD-shaped graph in fp32 and f16x3: every blob within ACT_TOL, each boxes_<level> against the oracle (equal counts,
   SCORE_TOL, BOX_TOL), blob shapes from the C side; forward_group over three lanes of different sizes equals the units run
   one at a time, bit for bit.
5. The profiler books one conv_mfma_gen_kernel launch per general layer and pass for a 3-lane group, none for a graph without.
6. Refusals: group 2; a kernel extent beyond the padded input at construction and after a reshape, the net staying usable.
7. Constructing the unchanged template nets allocates what it allocated before this kernel existed.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC

pytestmark = pytest.mark.gpu

ACT_TOL = 2e-5          # tests/test_gpu_parity.py
SCORE_TOL = 1e-4
BOX_TOL = 1e-3
EXACT_MODES = ["fp32", "f16x3", "bf16", "f64"]
KERNEL = "conv_mfma_gen_kernel"
INFO = np.array([[8, 8, 1]], np.float32)


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


# ---- 1. integer grids: exact in every mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias,relu", G.VARIANTS, ids=lambda v: str(int(v)))
@pytest.mark.parametrize("case_first", G.ALL_CASES, ids=G.case_id)
def test_integer_grids_are_exact_in_every_mode(case_first, bias, relu):
    case, first = case_first
    data, wt, bs = G.int_inputs(case, first, bias)
    params, perm = G.g_params(case, first, wt, bs)
    net = _net(G.layer_net_text(case, first, bias, relu), params)
    want = G.oracle_layer(case, data[:, perm], wt, bs, relu)
    assert relu or (want < 0).any()
    for mode in EXACT_MODES:
        net.set_conv_mode(mode)
        _forward(net, data)
        got = _blob(net, "g")
        assert tuple(net.blobs["g"].shape) == want.shape == (1, case[1]) + G.out_size(case), mode
        np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=mode)
        if not first:
            np.testing.assert_array_equal(_blob(net, G.feeder_txt(case[0], first)[1]), data[:, perm], err_msg=mode)


def test_concat_members_are_exact():
    rng = np.random.default_rng(12)
    data = rng.integers(-4, 5, (1, 16, 9, 11)).astype(np.float32)
    params = {"pre": G.feeder_params(16, False)[0]["pre"]}
    for name, k in (("g0", 3), ("g1", 5)):
        params[name] = [rng.integers(-2, 3, (12, 16, k, k)).astype(np.float32), rng.integers(-8, 9, (12,)).astype(np.float32)]
    net = _net(G.concat_net_text(), params)
    w0 = np.maximum(O.convolution(data, params["g0"][0], params["g0"][1], pad=1, stride=2), 0)
    w1 = O.convolution(data, params["g1"][0], params["g1"][1], pad=2, stride=2)
    assert (w1 < 0).any()
    for mode in EXACT_MODES:
        net.set_conv_mode(mode)
        _forward(net, data)
        np.testing.assert_array_equal(_blob(net, "g1"), w1, err_msg=mode)     # the view at coff 12 of cstride 24
        np.testing.assert_array_equal(_blob(net, "g0"), w0, err_msg=mode)
        np.testing.assert_array_equal(_blob(net, "cat"), np.concatenate([w0, w1], axis=1), err_msg=mode)


# ---- 2. random grids ----------------------------------------------------------------------------------------------------------
def _assert_within_f64_bound(got, ref, mag, K, relu, what):
    """tests/test_gpu_f64_mode.py: |got - fl32(ref)| <= ulp32(ref) + 2 (K + 1) 2^-53 sum |a w| for every element."""
    r32 = ref.astype(np.float32)
    bound = np.spacing(np.abs(r32)).astype(np.float64) + 2.0 * (K + 1) * 2.0 ** -53 * mag
    want = np.maximum(r32, 0) if relu else r32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = int(np.argmax(err - bound))
    print("%s: K %d, %d elements, %d not bit-equal to fl32(ref), max err %.3e (bound there %.3e)"
          % (what, K, err.size, int((got != want).sum()), float(err.flat[worst]), float(bound.flat[worst])))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (err <= bound).all(), (what, float(err.flat[worst]), float(bound.flat[worst]))


@pytest.mark.parametrize("bias,relu", [(True, True), (False, False)], ids=["bias_relu", "plain"])
@pytest.mark.parametrize("case_first", G.ALL_CASES, ids=G.case_id)
def test_random_grids_against_the_oracle(case_first, bias, relu):
    case, first = case_first
    cin, cout, k, s, p, d, h, w = case
    data, wt, bs = G.random_inputs(case, first, bias)
    params, perm = G.g_params(case, first, wt, bs)
    net = _net(G.layer_net_text(case, first, bias, relu), params)
    x = data[:, perm]
    want = G.oracle_layer(case, x, wt, bs, relu)
    for mode in ("fp32", "f16x3"):
        net.set_conv_mode(mode)
        _forward(net, data)
        e = H.rel_err(_blob(net, "g"), want)
        print("%s %s: rel err %.3g" % (G.case_id(case_first), mode, e))
        assert e < ACT_TOL, (mode, e)
    net.set_conv_mode("f64")
    _forward(net, data)
    ref, mag = G.naive_conv(x[0], wt, bs, s, p, d, np.float64)
    _assert_within_f64_bound(_blob(net, "g")[0], ref, mag, cin * k * k, relu, G.case_id(case_first))


# ---- 3. split-format neighbours on the fused path -----------------------------------------------------------------------------
def test_split_format_neighbours_on_the_fused_path():
    h, w = 13, 19
    msg = P.parse(G.neighbours_text(h, w))
    params = O.synth_params(msg, seed=5, cls_bias=1.0)
    onet = G.FusionOracleNet(msg, params=params)
    gnet = _net(P.dumps(msg), params)
    data, info = H.synth_image_blob(h, w, seed=3), np.array([[h, w, 1.0]], np.float32)
    gnet.set_conv_mode("f16x3")
    redos = gnet.range_fallbacks
    H.run_both(gnet, onet, data, info)
    assert tuple(gnet.blobs["g"].shape) == (1, 128, 7, 10) == onet.blobs["g"].data.shape
    for name in ("c1", "c2", "g", "c3"):
        e = H.rel_err(_blob(gnet, name), onet.blobs[name].data)
        print("neighbours %s: rel err %.3g" % (name, e))
        assert e < ACT_TOL, (name, e)
    # what the FUSED pass itself left in the last map (the blobs above are re-run layer by layer when read)
    want = onet.blobs["c3"].data[0].copy()
    fused = H.read_fused_blob(gnet, onet, data, info, mode="f16x3")
    e = H.rel_err(fused, want)
    print("neighbours c3 of the fused pass: rel err %.3g" % e)
    assert e < ACT_TOL, e
    assert gnet.range_fallbacks == redos


# ---- 4. the S3FD-shaped graph ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s3fd():
    """The net, three lanes of it, and per group size the unit and the oracle's forwarded net (computed once)."""
    root = _net(G.s3fd_text(*G.S3FD_SIZE), G.s3fd_params())
    lanes = [root.clone() for _ in range(3)]
    units, oracles = [], []
    for h, w in G.S3FD_GROUP_SIZES:
        data, info = G.s3fd_unit(h, w)
        onet = G.s3fd_oracle(h, w)
        onet.blobs["data"].reshape(*data.shape)
        onet.blobs["im_info"].reshape(1, 3)
        onet.forward(data=data, im_info=info)
        units.append((data, info))
        oracles.append(onet)
    return root, lanes, units, oracles


def _s3fd_cfg():
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = G.S3FD_THRESH, G.S3FD_MIN_SIZE, 10000


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
def test_s3fd_shaped_graph_against_the_oracle(s3fd, mode):
    root, lanes, units, oracles = s3fd
    _s3fd_cfg()
    data, info = units[0]
    onet = oracles[0]
    root.set_conv_mode(mode)
    try:
        redos = root.range_fallbacks
        go = _forward(root, data, info)
        assert root.range_fallbacks == redos
        for name, hw in G.s3fd_map_sizes(*G.S3FD_SIZE).items():     # (blob shapes come from the C side)
            assert tuple(root.blobs[name].shape)[2:] == hw, name
        assert list(root.blobs.keys()) == list(onet.blobs.keys()) and MC.levels_of(root) == ["8", "16", "32"]
        for m in G.S3FD_MODULES:
            gb, gs, ob, os_ = go["boxes_" + m], go["cls_prob_" + m], onet.blobs["boxes_" + m].data, onet.blobs["cls_prob_" + m].data
            assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 1, (m, gb.shape, ob.shape)
            ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
            db = _match_rows(gb, gs, ob, os_)
            print("s3fd %s module %s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (mode, m, len(gs), ds, db))
            assert ds < SCORE_TOL and db < BOX_TOL, (m, ds, db)
        for name in ("stem", "c2", "p2", "c3", "f8", "e1a", "f16", "e2a", "f32"):
            e = H.rel_err(_blob(root, name), onet.blobs[name].data)
            print("s3fd %s %s: rel err %.3g" % (mode, name, e))
            assert e < ACT_TOL, (name, e)
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_s3fd_forward_group_equals_the_units_one_at_a_time(s3fd, mode):
    root, lanes, units, oracles = s3fd
    _s3fd_cfg()
    root.set_conv_mode(mode)
    try:
        single = [_forward(root, x, info) for x, info in units]
        assert all(len(s) == 6 and len(s["cls_prob_8"]) > 1 for s in single)
        ins = []
        for lane, (x, info) in zip(lanes, units):
            lane.blobs["data"].reshape(*x.shape)
            lane.blobs["im_info"].reshape(1, 3)
            ins.append({"data": x, "im_info": info})
        outs = root.forward_group(lanes, ins)
        for k, (lane, out) in enumerate(zip(lanes, outs)):
            assert sorted(out.keys()) == sorted(single[k].keys())
            for key in out:
                np.testing.assert_array_equal(out[key], single[k][key], err_msg="unit %d %s" % (k, key))
            # ... and the oracle's rows at this unit's size (tiles decoded across the member boundaries)
            for m in G.S3FD_MODULES:
                assert out["cls_prob_" + m].shape == oracles[k].blobs["cls_prob_" + m].data.shape, (k, m)
            e = H.rel_err(_blob(lane, "f32"), oracles[k].blobs["f32"].data)
            assert e < ACT_TOL, (k, e)
    finally:
        root.set_conv_mode("fp32")


# ---- 5. the profiler ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f64"])
def test_profiler_books_one_launch_per_general_layer_and_pass(s3fd, mode):
    root, lanes, units, oracles = s3fd
    _s3fd_cfg()
    ins = []
    for lane, (x, info) in zip(lanes, units):
        lane.blobs["data"].reshape(*x.shape)
        lane.blobs["im_info"].reshape(1, 3)
        ins.append({"data": x, "im_info": info})
    root.set_conv_mode(mode)
    try:
        root.forward_group(lanes, ins)
        redos = root.range_fallbacks
        root.prof_enable(True)
        root.prof_reset()
        root.forward_group(lanes, ins)
        rec = root.prof_read()[KERNEL]
        assert root.range_fallbacks == redos
        assert int(rec["launches"]) == len(G.S3FD_GENERAL_LAYERS), rec
        assert rec["flops"] > 0
    finally:
        root.prof_enable(False)
        root.set_conv_mode("fp32")


def test_profiler_books_none_for_a_graph_without_general_layers():
    net = _net(MC.mini_text(13, 19), MC.mini_params(7))
    x = np.random.default_rng(3).normal(0, 64, (1, 128, 13, 19)).astype(np.float32)
    info = np.array([[101, 147, 1.0]], np.float32)
    _forward(net, x, info)
    net.prof_enable(True)
    net.prof_reset()
    try:
        _forward(net, x, info)
        prof = net.prof_read()
        assert KERNEL in prof and int(prof[KERNEL]["launches"]) == 0
        assert sum(int(v["launches"]) for v in prof.values()) > 0
    finally:
        net.prof_enable(False)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_at_construction():
    from smallhardface_amd import caffe
    pre = G.conv_txt("pre", "data", 16, 1)
    with pytest.raises(RuntimeError, match=r"Convolution 'g': group != 1 unsupported"):
        caffe.Net(None, prototxt_text=H.single_layer_net(pre + G.conv_txt("g", "pre", 16, 3, 2, 1, 1, group=2), 16, 8, 8))
    # 5x5 'valid' on a 4 x 8 map; dilation 3 makes a 3x3 kernel 7 wide on 2 + 2 * 2 = 6 rows
    with pytest.raises(RuntimeError, match=r"Convolution 'g': kernel extent 5 .*padded input 4 x 8"):
        caffe.Net(None, prototxt_text=H.single_layer_net(pre + G.conv_txt("g", "pre", 16, 5, 1, 0, 1), 16, 4, 8))
    with pytest.raises(RuntimeError, match=r"Convolution 'g': kernel extent 7 .*padded input 6 x 13"):
        caffe.Net(None, prototxt_text=H.single_layer_net(pre + G.conv_txt("g", "pre", 16, 3, 2, 2, 3), 16, 2, 9))
    # the extent that just fits is accepted: a 1 x 4 output
    net = caffe.Net(None, prototxt_text=H.single_layer_net(pre + G.conv_txt("g", "pre", 16, 5, 1, 0, 1), 16, 5, 8))
    assert tuple(net.blobs["g"].shape) == (1, 16, 1, 4)


def test_a_refused_reshape_leaves_the_net_usable():
    case = (16, 32, 3, 1, 0, 1, 5, 6)
    data, wt, bs = G.int_inputs(case, False, True)
    params, perm = G.g_params(case, False, wt, bs)
    net = _net(G.layer_net_text(case, False), params)
    want = G.oracle_layer(case, data, wt, bs, False)
    np.testing.assert_array_equal(_forward(net, data)["g"], want)
    small = np.zeros((1, 16, 2, 6), np.float32)
    for _ in range(2):
        with pytest.raises(RuntimeError, match=r"Convolution 'g': kernel extent 3 .*padded input 2 x 6"):
            _forward(net, small)
    # back at the size of the last good forward, and at a new one
    np.testing.assert_array_equal(_forward(net, data)["g"], want)
    assert tuple(net.blobs["g"].shape) == (1, 32, 3, 4)
    big = np.random.default_rng(1).integers(-4, 5, (1, 16, 7, 9)).astype(np.float32)
    np.testing.assert_array_equal(_forward(net, big)["g"], G.oracle_layer((16, 32, 3, 1, 0, 1, 7, 9), big, wt, bs, False))


# ---- 7. no side effects on the nets that loaded before --------------------------------------------------------------------------
# device allocations of constructing the template nets (parameters, packs, blobs, workspaces), recorded on the parent of the
# commit that added the general kernel with this very function (MI355X, default conv mode)
TEMPLATE_DEVICE_ALLOCS = {True: 104, False: 90}


def template_device_allocs(different_dilation):
    from smallhardface_amd import caffe
    text = P.dumps(H.detector_msg(different_dilation))
    before = caffe.alloc_counts()
    net = caffe.Net(None, prototxt_text=text)
    after = caffe.alloc_counts()
    del net
    return after[0] - before[0]


@pytest.mark.parametrize("different_dilation", [True, False])
def test_template_nets_allocate_what_they_did(different_dilation):
    assert template_device_allocs(different_dilation) == TEMPLATE_DEVICE_ALLOCS[different_dilation]
