"""BatchNorm and Scale on the GPU: the channel-affine kernels of csrc/norm.hip behind Net.forward() and forward_group(), the
in-place chain as one launch, the fold into the producing convolution, commits, the range guard, the caffemodel loader and
the refusals.

How outputs are observed (as in tests/test_gpu_fusion_layers.py).  A layer under test is judged from the GPU's own bottom,
read back as a blob, so only that layer is on trial; graphs without a proposal tail run the per-layer path in every mode, and
the profiler's class `channel_affine` says how many launches of the new kernel ran.  The bottoms `b0` .. are 1x1
convolutions of a 16-channel layer `pre` on a 16-channel net input: any channel count C, values of both signs.

Bounds.  The stand-alone launches are exact: bit for bit the fp32 references of tests/norm_cases.py (every operation rounded
once) and, in conv mode "f64", the binary64 statement rounded once.  The fold is exact against a bare convolution that holds
`norm_cases.fold` of the same blobs; against the layer-by-layer oracle it is held to ACT_TOL in the parity modes (fp32, f16x3,
f64), half of which the fold arithmetic may use (measured on the CPU: tests/test_norm_layers_host.py).  bf16 is a throughput
mode with 8 mantissa bits (tests/test_gpu_reduced_modes.py: ~1.5e-2): there the fold is held to bit identity alone.

Shapes (C, h, w): (4, 1, 1) one quad, one pixel; (6, 3, 5) the scalar form; (12, 3, 5) three quads; (64, 5, 7) a wave spans
several pixels; (64, 11, 67) more than one block.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import fusion_cases as F
from tests import helpers as H
from tests import norm_cases as N

pytestmark = pytest.mark.gpu

ACT_TOL = 2e-5          # tests/test_gpu_parity.py
SCORE_TOL = 1e-4        # tests/test_gpu_parity.py
BOX_TOL = 1e-3          # px (tests/test_gpu_modules.py)
MODES = ["fp32", "f16x3"]
SHAPES = [(4, 1, 1), (6, 3, 5), (12, 3, 5), (64, 5, 7), (64, 11, 67)]
KERNEL = "channel_affine"
COMBINE = "eltwise_combine"
F32 = np.float32


# ---- harness ------------------------------------------------------------------------------------------------------------------
def _bottoms(C, names):
    txt = F.conv_layer("pre", "data", 16, 1)
    for name, ch in names:
        txt += F.conv_layer(name, "pre", ch if ch else C, 1)
    return txt


def _data(h, w, seed=0, cin=16):
    return np.random.default_rng(100 + seed).normal(0, 1, (1, cin, h, w)).astype(F32)


def _net(txt, data, seed=0, factors=None):
    """(net, message, parameters): the graph with `norm_cases.synth_norm_params` of an oracle forward of `data`."""
    from smallhardface_amd import caffe
    msg = P.parse(txt)
    params = N.synth_norm_params(msg, data, seed=seed, factors=factors)
    net = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(net, params)
    return net, msg, params


def _oracle(msg, params, data, info=None, **kw):
    onet = N.NormOracleNet(msg, params=params, **kw)
    onet.blobs["data"].reshape(*data.shape)
    onet.blobs["im_info"].reshape(1, 3)
    onet.forward(data=data, im_info=np.array([[data.shape[2], data.shape[3], 1]], F32) if info is None else info)
    return onet


def _stage(net, data):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {"data": data, "im_info": np.array([[data.shape[2], data.shape[3], 1]], F32)}


def _forward(net, data):
    return net.forward(**_stage(net, data))


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


def _blob(net, name):
    return np.array(net.blobs[name].data)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(what))


# ---- 1. stand-alone launches, bit for bit ---------------------------------------------------------------------------------------
def _standalone_text(C, h, w):
    """b0 -> `bn` -> `sc` (bias_term) / `scn` (none) -> ReLU slope 0 `r0` / slope 0.3 `r3`, every layer with a top of its own;
    `sc_only` a Scale alone on b0; `bn0` a BatchNorm whose blob2 is 0; `bn_v6` / `bn_v8` read the second member of a zero-copy
    Concat at channel offset 6 (scalar form) / 8 (vector form, when C allows); `bn_t` writes a member of the Concat `cc_t`."""
    txt = _bottoms(C, [("b0", 0), ("b1", 0), ("b2", 0), ("m6", 6), ("m8", 8), ("m8t", 8)])
    txt += (N.bn_layer("bn", "b0", top="bn") + N.scale_layer("sc", "bn", top="sc") + N.scale_layer("scn", "bn", top="scn", bias=False) +
            F.relu_layer("r0", "sc", top="r0") + F.relu_layer("r3", "sc", top="r3", slope=0.3) +
            N.scale_layer("sc_only", "b0", top="sc_only") + N.bn_layer("bn0", "b0", top="bn0", eps=1e-3) +
            F.concat_layer("cc6", ["m6", "b1"]) + F.concat_layer("cc8", ["m8", "b2"]) +
            N.bn_layer("bn_v6", "b1", top="bn_v6") + N.bn_layer("bn_v8", "b2", top="bn_v8") +
            N.bn_layer("bn_t", "b0", top="bn_t") + F.concat_layer("cc_t", ["m8t", "bn_t"]))
    return H.single_layer_net(txt, 16, h, w)


STANDALONE_LAUNCHES = 8      # bn, sc, scn, sc_only, bn0, bn_v6, bn_v8, bn_t (the two ReLUs are combine launches)


@pytest.mark.parametrize("C,h,w", SHAPES)
def test_standalone_layers_bit_for_bit(C, h, w):
    x = _data(h, w, C)
    net, _, p = _net(_standalone_text(C, h, w), x, seed=C + h, factors={"bn0": 0.0})
    assert p["bn0"][2][0] == 0 and p["bn"][2][0] == F32(N.FACTOR)
    for mode in MODES + ["f64"]:
        net.set_conv_mode(mode)
        falls = net.range_fallbacks
        out, prof = _profiled(net, lambda: _forward(net, x))
        assert prof[KERNEL] == STANDALONE_LAUNCHES and prof[COMBINE] == 2 and net.range_fallbacks == falls, (mode, prof[KERNEL])
        b0, b1, b2, bn, sc = (_blob(net, n) for n in ("b0", "b1", "b2", "bn", "sc"))
        assert b0.shape == (1, C, h, w) and (b0.size < 64 or ((b0 < 0).any() and (b0 > 0).any()))
        if mode == "f64":        # the binary64 statement, rounded once
            bnf = lambda v, blobs, eps=N.EPS: N.chain64(v, bn=blobs, eps=eps)
            scf = lambda v, blobs: N.chain64(v, sc=blobs)
        else:                    # Caffe's fp32 operations
            bnf = lambda v, blobs, eps=N.EPS: N.batch_norm(v, blobs, eps)
            scf = lambda v, blobs: N.scale(v, *blobs)
        _same(bn, bnf(b0, p["bn"]), (mode, "bn", C, h, w))
        _same(sc, scf(bn, p["sc"]), (mode, "sc"))
        _same(_blob(net, "scn"), scf(bn, p["scn"]), (mode, "scn"))
        _same(_blob(net, "r0"), F.relu(sc), (mode, "r0"))
        _same(_blob(net, "r3"), F.relu(sc, 0.3), (mode, "r3"))
        _same(_blob(net, "sc_only"), scf(b0, p["sc_only"]), (mode, "sc_only"))
        _same(_blob(net, "bn0"), bnf(b0, p["bn0"], 1e-3), (mode, "bn0"))
        _same(_blob(net, "bn_v6"), bnf(b1, p["bn_v6"]), (mode, "bn_v6"))
        _same(_blob(net, "bn_v8"), bnf(b2, p["bn_v8"]), (mode, "bn_v8"))
        _same(_blob(net, "bn_t"), bnf(b0, p["bn_t"]), (mode, "bn_t"))
        # the views: the Concats hold their members
        _same(_blob(net, "cc6"), np.concatenate([_blob(net, "m6"), b1], axis=1), (mode, "cc6"))
        _same(_blob(net, "cc_t"), np.concatenate([_blob(net, "m8t"), _blob(net, "bn_t")], axis=1), (mode, "cc_t"))
        _same(np.array(out["bn_v8"]), _blob(net, "bn_v8"), (mode, "out"))
        assert len(p["scn"]) == 1 and (C < 64 or (p["sc"][0] < 0).any())          # (a fifth of the gammas are negative)


# ---- 2. the in-place chain is one launch -----------------------------------------------------------------------------------------
def _chain_text(C, h, w, slope=None, reader=False):
    """Eltwise `s` = b0 + b1, then BatchNorm, Scale and ReLU in place on `s`; `reader`: a non-in-place ReLU `peek` reads `s`
    between the Scale and the ReLU."""
    txt = (_bottoms(C, [("b0", 0), ("b1", 0)]) + F.eltwise_layer("s", ["b0", "b1"]) + N.bn_layer("s_bn", "s") + N.scale_layer("s_sc", "s") +
           (F.relu_layer("peek", "s", top="peek", slope=0.5) if reader else "") + F.relu_layer("s_relu", "s", slope=slope))
    return H.single_layer_net(txt, 16, h, w)


@pytest.mark.parametrize("slope", [None, 0.3])
@pytest.mark.parametrize("C,h,w", [(6, 3, 5), (64, 11, 67)])
def test_in_place_chain_is_one_launch(C, h, w, slope):
    x = _data(h, w, C + 1)
    net, _, p = _net(_chain_text(C, h, w, slope), x, seed=C)
    peek, _, _ = _net(_chain_text(C, h, w, slope, reader=True), x, seed=C)
    H.load_params(peek, p)
    for mode in MODES + ["f64"]:
        chain = N.chain64 if mode == "f64" else N.chain32
        for g in (net, peek):
            g.set_conv_mode(mode)
        _, prof = _profiled(net, lambda: _forward(net, x))
        assert prof[KERNEL] == 1 and prof[COMBINE] == 1, (mode, prof[KERNEL], prof[COMBINE])          # the Eltwise, the chain
        pre = F.eltwise([_blob(net, "b0"), _blob(net, "b1")])
        want = chain(pre, p["s_bn"], p["s_sc"], slope=slope or 0.0)
        _same(_blob(net, "s"), want, (mode, "s", slope))
        assert (want == 0).any() or slope
        # a reader in between: BatchNorm + Scale are one launch, the ReLU runs on its own behind the reader (the Eltwise, `peek`
        # and it: three combine launches) -- the chain took more than one launch, the values are the same
        _, prof = _profiled(peek, lambda: _forward(peek, x))
        assert prof[KERNEL] == 1 and prof[COMBINE] == 3 and prof[KERNEL] + prof[COMBINE] - 2 > 1, (mode, prof[KERNEL], prof[COMBINE])
        _same(_blob(peek, "s"), want, (mode, "s behind the reader"))
        _same(_blob(peek, "peek"), F.relu(chain(pre, p["s_bn"], p["s_sc"]), 0.5), (mode, "peek"))


# ---- 3. the fold is exact by construction ----------------------------------------------------------------------------------------
FOLD_MODES = ["fp32", "f16x3", "bf16", "f64"]
PARITY_MODES = ["fp32", "f16x3", "f64"]


@pytest.mark.parametrize("bias,bn,sc", N.FOLD_VARIANTS, ids=["b%d_bn%d_sc%d" % v for v in N.FOLD_VARIANTS])
@pytest.mark.parametrize("case", sorted(N.FOLD_CASES))
def test_fold_equals_the_bare_convolution_with_folded_blobs(case, bias, bn, sc):
    from smallhardface_amd import caffe
    msg_a, pa, msg_b, pb, data = N.fold_pair(case, bias, bn, sc)
    a, b = caffe.Net(None, prototxt_text=P.dumps(msg_a)), caffe.Net(None, prototxt_text=P.dumps(msg_b))
    H.load_params(a, pa)
    H.load_params(b, pb)
    onet = _oracle(msg_a, pa, data)
    want = onet.blobs["c"].data
    assert len(a.params["c"]) == (2 if bias else 1) and len(b.params["c"]) == 2
    for mode in FOLD_MODES:
        a.set_conv_mode(mode)
        b.set_conv_mode(mode)
        oa, prof = _profiled(a, lambda: _forward(a, data))
        ob = _forward(b, data)
        assert prof[KERNEL] == 0 and prof[COMBINE] == 0, (mode, prof[KERNEL], prof[COMBINE])
        _same(np.array(oa["c"]), np.array(ob["c"]), (case, mode))
        _same(_blob(a, "c"), _blob(b, "c"), (case, mode, "blob"))
        if mode in PARITY_MODES:
            err = H.rel_err(oa["c"], want)
            print("%s %s: rel_err %.3g" % (case, mode, err))
            assert err < ACT_TOL, (case, mode, err)
    # Net.params keeps Caffe's unfolded blobs
    _same(np.array(a.params["c"][0].data), pa["c"][0], "unfolded weights")


# ---- 4. where the fold must not happen --------------------------------------------------------------------------------------------
def _nofold_text(kind, h=9, w=13):
    pre = N.conv_layer("pre", "data", 64, 1, 0) + F.relu_layer("pre_relu", "pre")
    if kind == "shared":       # two convolutions share their blobs, each under a BatchNorm of its own
        txt = (N.conv_layer("c", "pre", 64, 3, pnames=["w", "b"]) + N.bn_layer("c_bn", "c") +
               N.conv_layer("c2", "pre", 64, 3, pnames=["w", "b"]) + N.bn_layer("c2_bn", "c2"))
    elif kind == "own_top":    # a BatchNorm with a top of its own
        txt = N.conv_layer("c", "pre", 64, 3) + N.bn_layer("c_bn", "c", top="y") + N.scale_layer("y_sc", "y")
    else:                      # the convolution's top is read before the BatchNorm rewrites it
        txt = N.conv_layer("c", "pre", 64, 3) + F.relu_layer("peek", "c", top="peek", slope=0.25) + N.bn_layer("c_bn", "c") + N.scale_layer("c_sc", "c")
    return H.single_layer_net(pre + txt, 3, h, w)


@pytest.mark.parametrize("kind,launches", [("shared", 2), ("own_top", 1), ("read_before", 1)])
def test_unfoldable_layers_run_the_launch(kind, launches):
    data = H.synth_image_blob(9, 13, seed=2)
    net, msg, p = _net(_nofold_text(kind), data, seed=5)
    onet = _oracle(msg, p, data)
    for mode in MODES:
        net.set_conv_mode(mode)
        _, prof = _profiled(net, lambda: _forward(net, data))
        assert prof[KERNEL] == launches, (kind, mode, prof[KERNEL])
        for name in {"shared": ["c", "c2"], "own_top": ["c", "y"], "read_before": ["c", "peek"]}[kind]:
            err = H.rel_err(_blob(net, name), onet.blobs[name].data)
            assert err < ACT_TOL, (kind, mode, name, err)
        if kind == "own_top":      # the convolution's own top still holds the un-normalised values, the launch is exact on them
            _same(_blob(net, "y"), N.chain32(_blob(net, "c"), p["c_bn"], p["y_sc"]), (mode, "y"))
        if kind == "shared":
            assert p["c"][0] is p["c2"][0] and H.rel_err(onet.blobs["c"].data, onet.blobs["c2"].data) > 1e-2


def test_an_unfolded_chain_in_front_of_a_pool_keeps_the_pool_a_launch():
    """conv -> ReLU -> BatchNorm -> Scale, the three in place, -> MAX 2x2/2 pool under a proposal tail.  The ReLU is the
    convolution's epilogue, so the BatchNorm / Scale behind it cannot fold and rewrite the pool's bottom with a launch of their
    own: the convolution must not pool in its epilogue (it would pool the un-normalised values; with negative gammas not even
    monotonically related).  The fused pass's own `f`, read through one-hot predictors, and every blob against the oracle."""
    h, w = 20, 28
    txt = H.mini_detector(F.conv_layer("c0", "data", 64, 3, True) + F.conv_layer("c", "c0", 128, 3, True) + N.bn_layer("c_bn", "c") +
                          N.scale_layer("c_sc", "c") + F.pool_layer("p", "c") + F.conv_layer("f", "p", 128, 3, True), "f", 2, 3, h, w)
    data, info = H.synth_image_blob(h, w, seed=6), np.array([[h, w, 1]], F32)
    gnet, msg, p = _net(txt, data, seed=9)
    assert (p["c_sc"][0] < 0).any()
    onet = _oracle(msg, p, data, info)
    want = {k: np.array(onet.blobs[k].data) for k in ("c", "p", "f")}
    assert want["p"].shape == (1, 128, 10, 14) and (want["p"] < 0).any()
    gnet.set_conv_mode("f16x3")
    _, prof = _profiled(gnet, lambda: _forward(gnet, data))
    assert prof[KERNEL] == 1 and prof["maxpool_kernel"] == 1 and prof["detect_tail"] >= 1, (prof[KERNEL], prof["maxpool_kernel"])
    fused = H.read_fused_blob(gnet, onet, data, info, "f16x3")
    err = H.rel_err(fused, want["f"][0])
    print("fused path: f rel err %.3g" % err)
    assert err < ACT_TOL, err
    for mode in MODES:
        gnet.set_conv_mode(mode)
        _forward(gnet, data)
        for name in ("c", "p", "f"):
            assert H.rel_err(_blob(gnet, name), want[name]) < ACT_TOL, (mode, name)
        _same(_blob(gnet, "p"), O.max_pool(_blob(gnet, "c"), 2, 2, 0), (mode, "the pool of the rewritten blob"))


# ---- 5. commits ------------------------------------------------------------------------------------------------------------------
def test_commits_refold_and_repack():
    from smallhardface_amd import caffe
    msg, pa, _, _, data = N.fold_pair("c3x3", True, True, True)[:5]
    txt = P.dumps(msg)
    net = caffe.Net(None, prototxt_text=txt)
    H.load_params(net, pa)
    net.set_conv_mode("fp32")
    first = np.array(_forward(net, data)["c"])

    def fresh(params, mode="fp32"):
        g = caffe.Net(None, prototxt_text=txt)
        H.load_params(g, params)
        g.set_conv_mode(mode)
        return np.array(_forward(g, data)["c"])

    rng = np.random.default_rng(8)
    p2 = {k: [np.array(v) for v in blobs] for k, blobs in pa.items()}
    p2["c_bn"] = N.norm_blobs("BatchNorm", _oracle(msg, pa, data).snapshots[("c", "c")], rng, factor=37.5)
    for i, arr in enumerate(p2["c_bn"]):
        net.params["c_bn"][i].data[...] = arr
    net.commit_params()
    second, prof = _profiled(net, lambda: np.array(_forward(net, data)["c"]))
    assert prof[KERNEL] == 0 and H.rel_err(second, first) > 1e-3
    _same(second, fresh(p2), "new statistics")
    # the folded convolution's own weights
    p2["c"][0] = (p2["c"][0] * F32(0.5) + rng.normal(0, 0.01, p2["c"][0].shape)).astype(F32)
    net.params["c"][0].data[...] = p2["c"][0]
    net.commit_params()
    third = np.array(_forward(net, data)["c"])
    _same(third, fresh(p2), "new weights")
    _same(np.array(net.params["c"][0].data), p2["c"][0], "Net.params reads the unfolded weights")
    # a Scale commit in split-fp16 mode, then there and back
    net.set_conv_mode("f16x3")
    p2["c_sc"][0] = (p2["c_sc"][0] * F32(-1.25)).astype(F32)
    net.params["c_sc"][0].data[...] = p2["c_sc"][0]
    net.commit_params()
    _same(np.array(_forward(net, data)["c"]), fresh(p2, "f16x3"), "new gamma, f16x3")
    net.set_conv_mode("fp32")
    _same(np.array(_forward(net, data)["c"]), fresh(p2), "back in fp32")
    net.set_conv_mode("f16x3")
    _same(np.array(_forward(net, data)["c"]), fresh(p2, "f16x3"), "and f16x3 again")


def test_the_fp16_weight_check_sees_the_effective_weights():
    """Unfolded weights of a few tenths under a gamma of 1e7: W_eff leaves the fp16 range, the split-fp16 mode is refused with
    the convolution's name, the net stays in fp32 mode and forwards."""
    from smallhardface_amd import caffe
    msg, pa, _, _, data = N.fold_pair("c3x3", True, True, True)
    pa = dict(pa, c_sc=[(pa["c_sc"][0] * F32(1e7)).astype(F32), pa["c_sc"][1]])
    assert np.abs(pa["c"][0]).max() < 1 and np.abs(N.fold(pa["c"][0], pa["c"][1], pa["c_bn"], pa["c_sc"])[0]).max() > 65504
    net = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(net, pa)
    with pytest.raises(Exception, match=r"layer 'c'.*outside the fp16 range"):
        net.set_conv_mode("f16x3")
    assert net.conv_mode == "fp32"
    assert H.rel_err(_forward(net, data)["c"], _oracle(msg, pa, data).blobs["c"].data) < ACT_TOL


def test_commit_on_an_unfolded_layer_rederives_its_vectors():
    C, h, w = 12, 3, 5
    x = _data(h, w, 3)
    net, _, p = _net(_chain_text(C, h, w), x, seed=3)
    _forward(net, x)
    pre = F.eltwise([_blob(net, "b0"), _blob(net, "b1")])
    nb = N.norm_blobs("BatchNorm", pre, np.random.default_rng(1), factor=2.0)
    for i, arr in enumerate(nb):
        net.params["s_bn"][i].data[...] = arr
    net.commit_params()
    for mode in ("fp32", "f64"):
        net.set_conv_mode(mode)
        _forward(net, x)
        pre = F.eltwise([_blob(net, "b0"), _blob(net, "b1")])          # (the mode's own bottoms)
        _same(_blob(net, "s"), (N.chain64 if mode == "f64" else N.chain32)(pre, nb, p["s_sc"], slope=0.0), mode)


# ---- 6. the grouped pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_forward_group_is_one_launch_and_equals_single_forwards(mode):
    sizes = [(24, 32), (17, 23), (8, 8)]
    C = 12
    x0 = _data(*sizes[0], 5)
    root, _, p = _net(_chain_text(C, *sizes[0], slope=0.3), x0, seed=6)
    solo, _, _ = _net(_chain_text(C, *sizes[0], slope=0.3), x0, seed=6)
    lanes = [root, root.clone(), root.clone()]
    datas = [_data(h, w, 7 + j) for j, (h, w) in enumerate(sizes)]
    root.set_conv_mode(mode)
    solo.set_conv_mode(mode)
    outs, prof = _profiled(root, lambda: root.forward_group(lanes, [_stage(m, x) for m, x in zip(lanes, datas)]))
    assert prof[KERNEL] == 1 and prof[COMBINE] == 1, (mode, prof[KERNEL], prof[COMBINE])
    for j, (m, x, out) in enumerate(zip(lanes, datas, outs)):
        want = _forward(solo, x)
        _same(np.array(out["s"]), np.array(want["s"]), (mode, j, "out"))
        _same(_blob(m, "s"), _blob(solo, "s"), (mode, j, "blob"))
        _same(_blob(m, "s"), N.chain32(F.eltwise([_blob(m, "b0"), _blob(m, "b1")]), p["s_bn"], p["s_sc"], slope=0.3), (mode, j, "reference"))
        assert _blob(m, "s").shape == (1, C) + sizes[j]


# ---- 7. the range guard ------------------------------------------------------------------------------------------------------------
def test_a_scale_beyond_the_fp16_range_redoes_the_forward_in_fp32():
    """A 128-channel map is normalised into `n` and scaled in place: gamma and beta are set so that the top reaches 2e4 on the
    image and, on the image times 4, passes 65504 (9.1e4 on the CPU reference; the convolutions' own tops stay below 100).  A
    split-fp16 convolution reads it: the channel-affine launch raises the range flag, the forward is redone on the fp32
    kernels, the result is finite and right; the next forward, of the image itself, is clean."""
    from smallhardface_amd import caffe
    h, w = 20, 28
    txt = H.single_layer_net(F.conv_layer("c0", "data", 64, 3, True) + F.conv_layer("a", "c0", 128, 3) + N.bn_layer("a_bn", "a", top="n") +
                             N.scale_layer("n_sc", "n") + F.conv_layer("c2", "n", 128, 3, True), 3, h, w)
    msg = P.parse(txt)
    small = H.synth_image_blob(h, w, seed=3)
    big = small * F32(4)
    params = N.synth_norm_params(msg, small, seed=17)
    onet = _oracle(msg, params, small)
    s = F32(2.0e4 / np.abs(onet.blobs["n"].data).max())
    params["n_sc"][0] *= s
    params["n_sc"][1] *= s
    params["c2"][0] *= F32(2.0 ** -14)               # (c2's own outputs stay small: only the scaled map leaves the range)
    onet = _oracle(msg, params, big)
    m = {k: float(np.abs(onet.blobs[k].data).max()) for k in ("c0", "a", "n", "c2")}
    print(m)
    assert m["n"] > 65504 * 1.1 and m["a"] < 1000 and m["c0"] < 1000 and m["c2"] < 1000
    gnet = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(gnet, params)
    gnet.set_conv_mode("f16x3")
    before = gnet.range_fallbacks
    go, prof = _profiled(gnet, lambda: _forward(gnet, big))
    assert gnet.range_fallbacks == before + 1 and prof[KERNEL] == 2          # the launch, and once more in the fp32 redo
    assert np.isfinite(go["c2"]).all()
    for name in ("a", "n", "c2"):
        assert H.rel_err(_blob(gnet, name), onet.blobs[name].data) < ACT_TOL, name
    onet = _oracle(msg, params, small)
    assert float(np.abs(onet.blobs["n"].data).max()) < 65504 / 2
    n0 = gnet.range_fallbacks
    go = _forward(gnet, small)
    assert gnet.range_fallbacks == n0 and H.rel_err(go["c2"], onet.blobs["c2"].data) < ACT_TOL


# ---- 8. the whole graph --------------------------------------------------------------------------------------------------------------
RES_SEED, RES_THRESH, RES_MIN_SIZE = 22, 0.5, 3.0


@pytest.mark.parametrize("mode", MODES)
def test_resblock_against_the_oracle_net(mode):
    """norm_cases.resblock(64, 96) end to end.  Parameter seed 22, image seed 4, SCORE_THRESH 0.5: on the CPU reference alone
    the nearest foreground score is 1.2e-3 from the threshold (> 2 SCORE_TOL) and the nearest box side 0.106 px from the
    min-size cut -- asserted below -- so the row set does not hinge on the last digits (106 rows).  Five convolutions carry
    their BatchNorm + Scale (+ ReLU) folded in; the pre-activation chain behind the Eltwise is the one launch of the new class."""
    from smallhardface_amd import caffe
    msg = N.resblock(64, 96)
    data, info = H.synth_image_blob(64, 96, seed=4), np.array([[61, 93, 0.75]], F32)
    params = N.synth_norm_params(msg, data, info, seed=RES_SEED)
    old = (cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.SCORE_THRESH)
    cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.SCORE_THRESH = RES_MIN_SIZE, RES_THRESH
    try:
        onet = N.NormOracleNet(msg, params=params, proposal_cfg=O.ProposalParams(
            pre_nms_topN=int(cfg.TEST.N_DETS_PER_MODULE), score_thresh=RES_THRESH, min_size=RES_MIN_SIZE))
        gnet = caffe.Net(None, prototxt_text=P.dumps(msg))
        H.load_params(gnet, params)
        gnet.set_conv_mode(mode)
        (go, oo), prof = _profiled(gnet, lambda: H.run_both(gnet, onet, data, info))
        d_score, d_side, ties = N.resblock_margins(onet, info, RES_MIN_SIZE, RES_THRESH)
        assert d_score > 2 * SCORE_TOL and d_side > 0.01 and not ties, (d_score, d_side, ties)
        assert prof[KERNEL] == 1, prof[KERNEL]
        assert sorted(go.keys()) == sorted(onet.outputs) == ["boxes", "cls_prob"]
        gb, gs, ob, os_ = go["boxes"], go["cls_prob"], oo["boxes"], oo["cls_prob"]
        assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 10, (gb.shape, ob.shape)
        ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
        worst = 0.0
        for (ab, as_), (bb, bs) in (((gb, gs), (ob, os_)), ((ob, os_), (gb, gs))):
            for i in range(len(as_)):
                near = np.where(np.abs(bs[:, 1] - as_[i, 1]) < SCORE_TOL)[0]
                assert len(near) > 0, (i, as_[i])
                worst = max(worst, float(np.abs(bb[near] - ab[i]).max(axis=1).min()))
        print("resblock %s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (mode, len(gs), ds, worst))
        assert ds < SCORE_TOL and worst < BOX_TOL, (ds, worst)
        for name in N.RES_BLOBS:
            err = H.rel_err(_blob(gnet, name), onet.blobs[name].data)
            print("  %s rel_err %.3g" % (name, err))
            assert err < ACT_TOL, (name, err)
        assert (_blob(gnet, "res2a_branch2c") < 0).any() and (_blob(gnet, "res2a") >= 0).all()
    finally:
        cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.SCORE_THRESH = old


# ---- 9. caffemodel -----------------------------------------------------------------------------------------------------------------
def test_caffemodel_with_batchnorm_and_scale_blobs(tmp_path):
    from smallhardface_amd import caffe, caffemodel
    msg, pa, _, _, data = N.fold_pair("c3x3", False, True, True)
    txt = P.dumps(msg) + N.bn_layer("tail_bn", "c", top="y") + N.scale_layer("y_sc", "y", bias=False)
    msg = P.parse(txt)
    pa = N.synth_norm_params(msg, data, seed=3)
    types = {"c_bn": "BatchNorm", "tail_bn": "BatchNorm", "c_sc": "Scale", "y_sc": "Scale"}
    assert [b.shape for b in pa["tail_bn"]] == [(64,), (64,), (1,)] and len(pa["y_sc"]) == 1
    path = caffemodel.write_caffemodel(str(tmp_path / "n.caffemodel"), pa, layer_types=types)
    loaded = caffe.Net(None, path, caffe.TEST, prototxt_text=txt)
    byhand = caffe.Net(None, prototxt_text=txt)
    H.load_params(byhand, pa)
    for name, blobs in pa.items():
        for i, arr in enumerate(blobs):
            _same(np.array(loaded.params[name][i].data), arr, (name, i))
    oa, ob = _forward(loaded, data), _forward(byhand, data)
    _same(np.array(oa["y"]), np.array(ob["y"]), "forward")
    assert H.rel_err(oa["y"], _oracle(msg, pa, data).blobs["y"].data) < ACT_TOL
    bad = dict(pa, c_bn=pa["c_bn"][:2])
    caffemodel.write_caffemodel(str(tmp_path / "count.caffemodel"), bad, layer_types=types)
    with pytest.raises(Exception, match=r"Incompatible number of blobs for layer c_bn"):
        caffe.Net(None, str(tmp_path / "count.caffemodel"), caffe.TEST, prototxt_text=txt)
    bad = dict(pa, c_sc=[np.ones(65, F32), pa["c_sc"][1]])
    caffemodel.write_caffemodel(str(tmp_path / "size.caffemodel"), bad, layer_types=types)
    with pytest.raises(Exception, match=r"Cannot copy param 0 weights from layer 'c_sc'; shape mismatch"):
        caffe.Net(None, str(tmp_path / "size.caffemodel"), caffe.TEST, prototxt_text=txt)


def test_fresh_blobs_are_caffes_fillers():
    """BatchNorm's three blobs start at zero, Scale's gamma at one and beta at zero; shared by `param { name: }` and by lanes."""
    from smallhardface_amd import caffe
    txt = H.single_layer_net(_bottoms(8, [("b0", 0)]) + N.bn_layer("n", "b0", top="n", pnames=["m", "v", "f"]) +
                             N.bn_layer("n2", "b0", top="n2", pnames=["m", "v", "f"]) + N.scale_layer("s", "b0", top="s"), 16, 3, 5)
    net = caffe.Net(None, prototxt_text=txt)
    assert [tuple(b.data.shape) for b in net.params["n"]] == [(8,), (8,), (1,)]
    assert all((np.array(b.data) == 0).all() for b in net.params["n"])
    assert (np.array(net.params["s"][0].data) == 1).all() and (np.array(net.params["s"][1].data) == 0).all()
    x = _data(3, 5)
    blobs = [np.full(8, 0.5, F32), np.full(8, 4.0, F32), np.array([2.0], F32)]
    for i, arr in enumerate(blobs):
        net.params["n"][i].data[...] = arr
    net.commit_params()
    lane = net.clone()
    _forward(lane, x)
    want = N.batch_norm(_blob(lane, "b0"), blobs)
    _same(_blob(lane, "n"), want, "lane")
    _same(_blob(lane, "n2"), want, "shared by name")
    _same(_blob(lane, "s"), _blob(lane, "b0"), "gamma 1, beta 0")


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------
RESHAPE_3D = 'layer { name: "rs" type: "Reshape" bottom: "b0" top: "rs" reshape_param { shape { dim: 1 dim: -1 dim: 5 } } }\n'
TWO_TOPS = 'layer { name: "%s" type: "%s" bottom: "b0" top: "t1" top: "t2" }\n'

REFUSALS = [
    (N.bn_layer("n_in", "data", top="y"), r"BatchNorm 'n_in'.*'data' is a net input"),
    (N.scale_layer("s_in", "data", top="y"), r"Scale 's_in'.*'data' is a net input"),
    (N.bn_layer("n_flat", "im_info", top="y"), r"BatchNorm 'n_flat'.*'im_info'"),
    (N.scale_layer("s_flat", "im_info", top="y"), r"Scale 's_flat'.*'im_info'"),
    (N.bn_layer("n_3d", "rs", top="y"), r"BatchNorm 'n_3d'.*'rs' is not 4-D"),
    (N.scale_layer("s_3d", "rs", top="y"), r"Scale 's_3d'.*'rs' is not 4-D"),
    (TWO_TOPS % ("n_tops", "BatchNorm"), r"BatchNorm 'n_tops'.*exactly one bottom and one top"),
    (TWO_TOPS % ("s_tops", "Scale"), r"Scale 's_tops'.*exactly one bottom and one top"),
    ('layer { name: "n_bots" type: "BatchNorm" bottom: "b0" bottom: "b1" top: "y" }\n', r"BatchNorm 'n_bots'.*exactly one bottom and one top"),
    (N.scale_layer("s_two", None, top="y", bottoms=["b0", "b1"]), r"Scale 's_two'.*two-bottom form"),
    (N.scale_layer("s_axis", "b0", top="y", extra=" axis: 0"), r"Scale 's_axis'.*axis 0"),
    (N.scale_layer("s_axes", "b0", top="y", extra=" num_axes: 2"), r"Scale 's_axes'.*num_axes 2"),
    (N.scale_layer("s_all", "b0", top="y", extra=" axis: 1 num_axes: -1"), r"Scale 's_all'.*num_axes -1"),
    (N.bn_layer("n_train", "b0", top="y", extra=" use_global_stats: false"), r"BatchNorm 'n_train'.*use_global_stats: false.*training"),
    (N.bn_layer("n_nan", "b0", top="y", eps="nan"), r"BatchNorm 'n_nan'.*eps"),
    (N.bn_layer("n_inf", "b0", top="y", eps="inf"), r"BatchNorm 'n_inf'.*eps"),
    (N.bn_layer("n_huge", "b0", top="y", eps="1e39"), r"BatchNorm 'n_huge'.*eps"),
    (N.bn_layer("n_neg", "b0", top="y", eps=-1e-5), r"BatchNorm 'n_neg'.*eps"),
    (F.concat_layer("cc", ["b0", "b1"]) + N.bn_layer("n_member", "b0"), r"BatchNorm 'n_member'.*in place after Concat 'cc'"),
    (F.concat_layer("cc", ["b0", "b1"]) + N.scale_layer("s_member", "b1"), r"Scale 's_member'.*in place after Concat 'cc'"),
]


@pytest.mark.parametrize("layers,match", REFUSALS, ids=[m.split("'")[1] for _, m in REFUSALS])
def test_graphs_refused_at_construction_by_layer_name(layers, match):
    from smallhardface_amd import caffe
    txt = H.single_layer_net(_bottoms(8, [("b0", 0), ("b1", 0)]) + RESHAPE_3D + layers, 16, 3, 5)
    with pytest.raises(Exception, match=match):
        caffe.Net(None, prototxt_text=txt)


@pytest.mark.parametrize("kind", ["BatchNorm", "Scale"])
def test_a_bottom_of_a_proposal_tail_is_refused(kind):
    from smallhardface_amd import caffe
    layer = N.bn_layer("n_tail", "cls_score_output", top="y") if kind == "BatchNorm" else N.scale_layer("n_tail", "cls_score_output", top="y")
    txt = H.mini_detector(F.conv_layer("c0", "data", 128, 3, True), "c0", 8, 3, 8, 8) + layer
    with pytest.raises(Exception, match=r"%s 'n_tail'.*'cls_score_output'.*proposal tail" % kind):
        caffe.Net(None, prototxt_text=txt)


def test_an_in_place_layer_before_the_concat_is_accepted():
    """The refused case is the layer placed AFTER the Concat; in front of it the member is rewritten before the view is read.
    The Scale directly on the convolution `b1` is folded; the BatchNorm behind it is not (the fold's order is BatchNorm, then
    Scale) and runs in place on the member's channel window of the Concat's buffer."""
    C, h, w = 8, 3, 5
    x = _data(h, w, 4)
    txt = H.single_layer_net(_bottoms(C, [("b0", 0), ("b1", 0)]) + N.scale_layer("b1_sc", "b1") + N.bn_layer("b1_bn", "b1") +
                             F.concat_layer("cc", ["b0", "b1"]), 16, h, w)
    net, msg, p = _net(txt, x, seed=2)
    onet = _oracle(msg, p, x)
    _, prof = _profiled(net, lambda: _forward(net, x))
    assert prof[KERNEL] == 1, prof[KERNEL]
    assert H.rel_err(_blob(net, "cc"), onet.blobs["cc"].data) < ACT_TOL
    _same(_blob(net, "cc")[:, C:], _blob(net, "b1"), "the member is the view")
