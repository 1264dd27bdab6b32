"""The Normalize layer (csrc/l2norm.hip: channel_l2norm) through caffe.Net, Net.forward and Net.forward_group (run on an
MI355X: ``pytest -m gpu``).  Cases, graphs and references: tests/l2norm_cases.py; the references on their own:
tests/test_l2norm_host.py.

Without the layer every test here fails at ``caffe.Net(...)`` ("Unsupported layer type 'Normalize'"), the refusals for want of
their texts.

1. Every layer case on integer grids, per-channel and shared scale, default eps and 0.001, out of place and in place: in conv
   modes fp32, f16x3 and bf16 equal to ``normalize32`` (the kernel's fp32 order; the sum of squares is exact), in f64 mode
   within one fp32 ulp of fp32(``normalize``).  "Equal" compares values: a zero's sign is the feeding convolution's.
2. Every layer case on random grids against binary64, fp32 and f64 mode: |got - ref| <= (C / 2 + 4) 2^-24 |ref| + 2^-126 per
   element (derived in ``l2norm_cases.bound``; no margin).
3. Concat members: `n1` reads the view at channel 12 of 24 (vector form) / 6 of 12 (scalar form) of one Concat and writes the
   same view of another; exact on integer grids.
4. Neighbours on the fused path in f16x3: convolution -> Normalize (scale 10) -> convolution within ACT_TOL of
   ``L2NormOracleNet``; the blob the Normalize reads stays plain fp32 (its other reader runs the family kernel's fp32-input
   class, as tests/test_gpu_fused_forms.py observes the format); the Normalize top as a ProposalLayer's head blob.
5. A scale that lifts the output beyond 65504 in f16x3 redoes the forward in fp32.
6. An S3FD-shaped detector with Normalize on `f8` and `f16` against the oracle, forward_group over three lanes bit for bit,
   the profiler's count per pass.
7. Refusals by layer name, a refused reshape, caffemodel blobs, fillers, shared blobs, commits.
"""
import numpy as np
import pytest

from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import depthwise_cases as D
from tests import fusion_cases as F
from tests import general_conv_cases as G
from tests import helpers as H
from tests import l2norm_cases as L
from tests import modules_cases as MC

pytestmark = pytest.mark.gpu

F32 = np.float32
F64 = np.float64
ACT_TOL = 2e-5          # tests/test_gpu_parity.py
SCORE_TOL = 1e-4
BOX_TOL = 1e-3
FP32_FORM_MODES = ["fp32", "f16x3", "bf16"]
KERNEL = "channel_l2norm"
FUSE1 = "conv_mfma_f16x3_kernel<64, true, 1, 3, 3, false>"          # tests/test_gpu_fused_forms.py


def W4(split, mt, nt):
    return "conv_mfma_f16x3_w4d_kernel<%s, %d, %d, 3, false, 1>" % ("true" if split else "false", mt, nt)


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


def _equal(got, want, what):
    """Value for value (bit for bit but for the sign of a zero), and no NaN on either side."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    np.testing.assert_array_equal(got, want, err_msg=str(what))


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
VARIANTS = [(False, None, False), (True, 0.001, True), (False, 0.001, True), (True, None, False)]     # (shared, eps, in place)


@pytest.mark.parametrize("shared,eps,in_place", VARIANTS, ids=["vec_out", "shared_eps_inplace", "vec_eps_inplace", "shared_out"])
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_integer_grids_are_exact_in_every_mode(case, shared, eps, in_place):
    C, h, w = case
    data, sc = L.int_inputs(case, shared)
    params, perm = L.n_params(case, sc)
    net = _net(L.layer_net_text(case, shared, eps, in_place), params)
    x = data[:, perm]
    e = L.EPS if eps is None else eps
    want32, want64 = L.normalize32(x, sc, e, shared), L.normalize(x, sc, e, shared).astype(F32)
    assert (h * w == 1 or (want32[:, :, 0, 0] == 0).all()) and np.abs(want32).max() > 0.01
    out = L.out_blob(case, in_place)
    for mode in FP32_FORM_MODES:
        net.set_conv_mode(mode)
        _forward(net, data)
        assert tuple(net.blobs[out].shape) == (1, C, h, w), mode
        _equal(_blob(net, out), want32, (mode, L.case_id(case)))
        if not in_place:
            _equal(_blob(net, D.feeder_txt(C)[1]), x, (mode, "the feeder"))
    net.set_conv_mode("f64")
    _forward(net, data)
    got = _blob(net, out)
    near = (got == want64) | (got == np.nextafter(want64, F32(np.inf))) | (got == np.nextafter(want64, F32(-np.inf)))
    print("%s f64: %d of %d not equal to fp32(binary64)" % (L.case_id(case), int((got != want64).sum()), got.size))
    assert np.isfinite(got).all() and near.all(), int((~near).sum())


# ---- 2. random grids against binary64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["per_channel", "shared"])
@pytest.mark.parametrize("case", L.LAYER_CASES, ids=L.case_id)
def test_random_grids_against_binary64(case, shared):
    C, h, w = case
    data, sc = L.random_inputs(case, shared)
    params, perm = L.n_params(case, sc)
    net = _net(L.layer_net_text(case, shared), params)
    x = data[:, perm]
    ref = L.normalize(x, sc, L.EPS, shared)
    bnd = L.bound(ref, C)
    for mode in ("fp32", "f64"):
        net.set_conv_mode(mode)
        _forward(net, data)
        _same(_blob(net, D.feeder_txt(C)[1]), x, (mode, "the feeder"))     # (x * 1 + 0 * ... is x in fp32 and in binary64)
        got = _blob(net, "n")
        err = np.abs(got.astype(F64) - ref)
        worst = int(np.argmax(err - bnd))
        print("%s %s: max err / bound %.3g, max |ref| %.3g" % (L.case_id(case), mode, float((err / bnd).max()), float(np.abs(ref).max())))
        assert got.shape == ref.shape and np.isfinite(got).all()
        assert (err <= bnd).all(), (mode, float(err.flat[worst]), float(bnd.flat[worst]))
    # ... and fp32 mode is the stated order, bit for bit wherever the fused multiply-add's model is exact (module docstring
    # of l2norm_cases: all but ties of a double rounding) -- reported, not asserted
    net.set_conv_mode("fp32")
    _forward(net, data)
    print("%s: %d of %d differ from normalize32" % (L.case_id(case), int((_blob(net, "n") != L.normalize32(x, sc, L.EPS, shared)).sum()), ref.size))


# ---- 3. Concat members ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [12, 6])
def test_concat_members_are_exact(C):
    rng = np.random.default_rng(12 + C)
    data = rng.integers(-4, 5, (1, 16, 7, 9)).astype(F32)
    data[:, :, 0, 0] = 0
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    sc0, sc1 = rng.integers(-3, 4, C).astype(F32), rng.integers(-3, 4, C).astype(F32)
    params = {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)],
              "n0": [sc0], "n1": [sc1]}
    net = _net(L.concat_net_text(C), params)
    wa, wb = L.normalize32(data[:, p0], sc0), L.normalize32(data[:, p1], sc1, 0.001)
    assert np.abs(wb).max() > 0.1
    for mode in FP32_FORM_MODES + ["f64"]:
        net.set_conv_mode(mode)
        _forward(net, data)
        _equal(_blob(net, "cin"), np.concatenate([data[:, p0], data[:, p1]], axis=1), (mode, "cin"))
        if mode == "f64":
            wa, wb = L.normalize(data[:, p0], sc0).astype(F32), L.normalize(data[:, p1], sc1, 0.001).astype(F32)
            for name, want in (("a", wa), ("b", wb)):
                assert (np.abs(_blob(net, name) - want) <= np.spacing(np.abs(want))).all(), name
            continue
        _equal(_blob(net, "b"), wb, (mode, "b"))            # read at coff C of cstride 2 C, written at coff C of cstride 2 C
        _equal(_blob(net, "a"), wa, (mode, "a"))
        _equal(_blob(net, "cat"), np.concatenate([wa, wb], axis=1), (mode, "cat"))


def test_in_place_on_a_member_before_the_concat():
    """The member is rewritten before the Concat's view is read: accepted, and the Concat holds the normalised values."""
    C, h, w = 8, 3, 5
    rng = np.random.default_rng(4)
    data = rng.integers(-4, 5, (1, 16, h, w)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    sc = rng.integers(1, 4, C).astype(F32)
    txt = H.single_layer_net(G.conv_txt("pre", "data", 16, 1) + G.conv_txt("s0", "pre", C, 1) + G.conv_txt("s1", "pre", C, 1) +
                             L.norm_layer("n", "s1") + F.concat_layer("cc", ["s0", "s1"]), 16, h, w)
    net = _net(txt, {"pre": G.feeder_params(16, False)[0]["pre"], "s0": [s0, np.zeros(C, F32)], "s1": [s1, np.zeros(C, F32)], "n": [sc]})
    (_, prof) = _profiled(net, lambda: _forward(net, data))
    assert prof[KERNEL] == 1
    _equal(_blob(net, "cc"), np.concatenate([data[:, p0], L.normalize32(data[:, p1], sc)], axis=1), "cc")
    _same(_blob(net, "cc")[:, C:], _blob(net, "s1"), "the member is the view")


# ---- 4. neighbours on the fused path --------------------------------------------------------------------------------------------
NB_HW = (13, 19)


def _copy(params):
    return {k: [np.array(v) for v in blobs] for k, blobs in params.items()}


def _neighbours(text_fn=L.neighbours_text, **kw):
    msg = P.parse(text_fn(*NB_HW, **kw))
    return msg, L.graph_params(msg, seed=5), H.synth_image_blob(*NB_HW, seed=3), np.array([[NB_HW[0], NB_HW[1], 1.0]], F32)


def test_split_fp16_neighbours_on_the_fused_path():
    msg, params, data, info = _neighbours()
    onet = L.L2NormOracleNet(msg, params=_copy(params))
    gnet = _net(P.dumps(msg), params)
    assert tuple(gnet.params["n"][0].data.shape) == (128,) and (np.array(gnet.params["n"][0].data) == 10).all()
    gnet.set_conv_mode("f16x3")
    redos = gnet.range_fallbacks
    _, prof = _profiled(gnet, lambda: H.run_both(gnet, onet, data, info))
    assert gnet.range_fallbacks == redos
    # the fused path ran (the first pair is one kernel); the Normalize is one launch; `c1`, which it reads, is plain fp32: both
    # family convolutions -- `c2` on the Normalize top and `c2b` on `c1` -- run the fp32-input class, none the split-input one
    split_in = sum(prof.get(W4(True, mt, nt), 0) for mt in (2, 4) for nt in (1, 2))
    plain_in = sum(prof.get(W4(False, mt, nt), 0) for mt in (2, 4) for nt in (1, 2))
    assert prof[FUSE1] == 1 and prof[KERNEL] == 1 and (split_in, plain_in) == (0, 2), (prof[FUSE1], prof[KERNEL], split_in, plain_in)
    assert tuple(gnet.blobs["n"].shape) == (1, 128) + NB_HW == onet.blobs["n"].data.shape
    for name in L.NB_BLOBS:
        e = H.rel_err(_blob(gnet, name), onet.blobs[name].data)
        print("neighbours %s: max %.3g, rel err %.3g" % (name, float(np.abs(onet.blobs[name].data).max()), e))
        assert e < ACT_TOL, (name, e)
    norms = np.sqrt((onet.blobs["n"].data.astype(F64) ** 2).sum(axis=1))
    assert np.abs(norms - 10).max() < 1e-4                  # every pixel of the top has norm 10
    # what the FUSED pass itself left in the last maps (the blobs above are re-run layer by layer when read)
    want = [onet.blobs[k].data[0].copy() for k in ("c2", "c2b")]
    fused = H.read_fused_blob(gnet, onet, data, info, mode="f16x3")
    for k, f, wnt in zip(("c2", "c2b"), fused, want):
        e = H.rel_err(f, wnt)
        print("neighbours %s of the fused pass: rel err %.3g" % (k, e))
        assert e < ACT_TOL, (k, e)
    assert gnet.range_fallbacks == redos


@pytest.fixture
def det_cfg():
    old = (cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE)
    cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE, cfg.TEST.N_DETS_PER_MODULE = G.S3FD_THRESH, G.S3FD_MIN_SIZE, 10000
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


def _check_rows(what, gb, gs, ob, os_):
    assert gb.shape == ob.shape and gs.shape == os_.shape and len(os_) > 1, (what, gb.shape, ob.shape)
    ds = float(np.abs(np.sort(gs[:, 1])[::-1] - np.sort(os_[:, 1])[::-1]).max())
    db = _match_rows(gb, gs, ob, os_)
    print("%s: %d rows, max |dscore| %.3g, max |dbox| %.3g px" % (what, len(gs), ds, db))
    assert ds < SCORE_TOL and db < BOX_TOL, (what, ds, db)


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_normalize_top_as_a_proposal_head_blob(det_cfg, mode):
    from oracle import oracle as O
    msg, params, data, info = _neighbours(L.head_text)
    onet = L.forwarded(L.L2NormOracleNet(msg, params=_copy(params), proposal_cfg=O.ProposalParams(
        pre_nms_topN=10000, score_thresh=G.S3FD_THRESH, min_size=G.S3FD_MIN_SIZE)), data, info)
    gnet = _net(P.dumps(msg), params)
    gnet.set_conv_mode(mode)
    go, prof = _profiled(gnet, lambda: _forward(gnet, data, info))
    assert prof[KERNEL] == 1 and prof["detect_tail"] >= 1
    _check_rows("head %s" % mode, go["boxes"], go["cls_prob"], onet.blobs["boxes"].data, onet.blobs["cls_prob"].data)
    e = H.rel_err(_blob(gnet, "n"), onet.blobs["n"].data)
    assert e < ACT_TOL, e


# ---- 5. the range guard -----------------------------------------------------------------------------------------------------------
def test_a_scale_beyond_the_fp16_range_redoes_the_forward_in_fp32():
    """The scale is 1e6: `c1` is of order 1, the Normalize top reaches 1e5 and more.  Its launch raises the range flag, the
    forward is redone on the fp32 kernels: outputs and blobs equal fp32 mode's."""
    msg, params, data, info = _neighbours(fill=1.0e6)
    params["c2"][0] = (params["c2"][0] * F32(2.0 ** -14)).astype(F32)
    onet = L.forwarded(L.L2NormOracleNet(msg, params=_copy(params)), data, info)
    m = {k: float(np.abs(onet.blobs[k].data).max()) for k in L.NB_BLOBS}
    print(m)
    assert m["n"] > 65504 * 1.5 and m["c1"] < 1000 and m["c2"] < 1000 and m["c2b"] < 1000
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
    for name in L.NB_BLOBS:
        _same(_blob(gnet, name), _blob(fnet, name), name)
        assert H.rel_err(_blob(gnet, name), onet.blobs[name].data) < ACT_TOL, name


# ---- 6. the S3FD-shaped detector ----------------------------------------------------------------------------------------------------
S3FD_BLOBS = ("stem", "c2", "p2", "c3", "f8", "f8_norm", "e1a", "f16", "f16_norm", "e2a", "f32")


@pytest.fixture(scope="module")
def s3fd():
    """The net, three lanes of it, and per group size the unit and the oracle's forwarded net (computed once)."""
    root = _net(L.s3fd_norm_text(*G.S3FD_SIZE), L.s3fd_norm_params())
    lanes = [root.clone() for _ in range(3)]
    units, oracles = [], []
    for h, w in G.S3FD_GROUP_SIZES:
        data, info = G.s3fd_unit(h, w)
        units.append((data, info))
        oracles.append(L.forwarded(L.s3fd_norm_oracle(h, w), data, info))
    return root, lanes, units, oracles


def _stage_group(lanes, units):
    ins = []
    for lane, (x, info) in zip(lanes, units):
        lane.blobs["data"].reshape(*x.shape)
        lane.blobs["im_info"].reshape(1, 3)
        ins.append({"data": x, "im_info": info})
    return ins


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_s3fd_with_normalize_against_the_oracle(s3fd, det_cfg, mode):
    root, lanes, units, oracles = s3fd
    data, info = units[0]
    onet = oracles[0]
    root.set_conv_mode(mode)
    try:
        redos = root.range_fallbacks
        go, prof = _profiled(root, lambda: _forward(root, data, info))
        assert root.range_fallbacks == redos
        assert prof[KERNEL] == len(L.S3FD_NORMS) == 2, prof[KERNEL]
        assert list(root.blobs.keys()) == list(onet.blobs.keys()) and MC.levels_of(root) == ["8", "16", "32"]
        assert [float(np.array(root.params[n][0].data)[0]) for n in L.S3FD_NORMS] == [10.0, 8.0]
        for m in L.S3FD_MODULES:
            _check_rows("s3fd %s module %s" % (mode, m), go["boxes_" + m], go["cls_prob_" + m], onet.blobs["boxes_" + m].data,
                        onet.blobs["cls_prob_" + m].data)
        for name in S3FD_BLOBS:
            e = H.rel_err(_blob(root, name), onet.blobs[name].data)
            print("s3fd %s %s: rel err %.3g" % (mode, name, e))
            assert e < ACT_TOL, (name, e)
        for name, (bottom, fill) in L.S3FD_NORMS.items():      # the shallow level no longer dwarfs the deep ones
            assert tuple(root.blobs[name].shape) == tuple(root.blobs[bottom].shape)
            norms = np.sqrt((_blob(root, name).astype(F64) ** 2).sum(axis=1))
            assert np.abs(norms - fill).max() < 1e-3 * fill, name
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_s3fd_forward_group_equals_the_units_one_at_a_time(s3fd, det_cfg, mode):
    root, lanes, units, oracles = s3fd
    root.set_conv_mode(mode)
    try:
        single = [_forward(root, x, info) for x, info in units]
        assert all(len(s) == 6 and len(s["cls_prob_8"]) > 1 for s in single)
        outs = root.forward_group(lanes, _stage_group(lanes, units))
        for k, (lane, out) in enumerate(zip(lanes, outs)):
            assert sorted(out.keys()) == sorted(single[k].keys())
            for key in out:
                _same(np.array(out[key]), single[k][key], "unit %d %s" % (k, key))
            for m in L.S3FD_MODULES:
                assert out["cls_prob_" + m].shape == oracles[k].blobs["cls_prob_" + m].data.shape, (k, m)
            for name in L.S3FD_NORMS:
                e = H.rel_err(_blob(lane, name), oracles[k].blobs[name].data)
                assert e < ACT_TOL, (k, name, e)
    finally:
        root.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", ["fp32", "f16x3", "f64"])
def test_profiler_books_one_launch_per_layer_and_pass_for_a_group(s3fd, det_cfg, mode):
    root, lanes, units, oracles = s3fd
    ins = _stage_group(lanes, units)
    root.set_conv_mode(mode)
    try:
        root.forward_group(lanes, ins)
        redos = root.range_fallbacks
        root.prof_enable(True)
        root.prof_reset()
        root.forward_group(lanes, ins)
        rec = root.prof_read()[KERNEL]
        assert root.range_fallbacks == redos
        assert int(rec["launches"]) == len(L.S3FD_NORMS) == 2, rec
        assert rec["flops"] > 0 and rec["bytes"] > 0
    finally:
        root.prof_enable(False)
        root.set_conv_mode("fp32")


def test_profiler_books_none_for_the_graph_without_the_layers():
    net = _net(G.s3fd_text(*G.S3FD_SIZE), G.s3fd_params())
    data, info = G.s3fd_unit(*G.S3FD_SIZE)
    _forward(net, data, info)
    _, prof = _profiled(net, lambda: _forward(net, data, info))
    assert KERNEL in prof and prof[KERNEL] == 0
    assert prof["conv_mfma_gen_kernel"] == len(G.S3FD_GENERAL_LAYERS)


# ---- 7. refusals and survival -------------------------------------------------------------------------------------------------------
def _bottoms():
    return G.conv_txt("pre", "data", 16, 1) + G.conv_txt("b0", "pre", 8, 1) + G.conv_txt("b1", "pre", 8, 1)


RESHAPE_3D = 'layer { name: "rs" type: "Reshape" bottom: "b0" top: "rs" reshape_param { shape { dim: 1 dim: -1 dim: 5 } } }\n'
BARE = 'layer { name: "%s" type: "Normalize" %s }\n'

REFUSALS = [
    (L.norm_layer("n_as", "b0", "y", across=True), r"Normalize 'n_as'.*across_spatial: true.*write across_spatial: false"),
    (L.norm_layer("n_default", "b0", "y", across=None), r"Normalize 'n_default'.*across_spatial: true.*write across_spatial: false"),
    (BARE % ("n_bare", 'bottom: "b0" top: "y"'), r"Normalize 'n_bare'.*write across_spatial: false"),
    (BARE % ("n_tops", 'bottom: "b0" top: "t1" top: "t2" norm_param { across_spatial: false }'), r"Normalize 'n_tops'.*exactly one bottom and one top"),
    (BARE % ("n_bots", 'bottom: "b0" bottom: "b1" top: "y" norm_param { across_spatial: false }'), r"Normalize 'n_bots'.*exactly one bottom and one top"),
    (L.norm_layer("n_in", "data", "y"), r"Normalize 'n_in'.*'data' is a net input"),
    (L.norm_layer("n_flat", "im_info", "y"), r"Normalize 'n_flat'.*'im_info'"),
    (L.norm_layer("n_3d", "rs", "y"), r"Normalize 'n_3d'.*'rs' is not 4-D"),
    (L.norm_layer("n_neg", "b0", "y", eps=-1e-10), r"Normalize 'n_neg'.*eps"),
    (L.norm_layer("n_nan", "b0", "y", eps="nan"), r"Normalize 'n_nan'.*eps"),
    (L.norm_layer("n_inf", "b0", "y", eps="inf"), r"Normalize 'n_inf'.*eps"),
    (L.norm_layer("n_huge", "b0", "y", eps="1e39"), r"Normalize 'n_huge'.*eps"),
    (F.concat_layer("cc", ["b0", "b1"]) + L.norm_layer("n_member", "b1"), r"Normalize 'n_member'.*in place after Concat 'cc'"),
]


@pytest.mark.parametrize("layers,match", REFUSALS, ids=[m.split("'")[1] for _, m in REFUSALS])
def test_graphs_refused_at_construction_by_layer_name(layers, match):
    from smallhardface_amd import caffe
    txt = H.single_layer_net(_bottoms() + RESHAPE_3D + layers, 16, 3, 5)
    with pytest.raises(Exception, match=match):
        caffe.Net(None, prototxt_text=txt)


def test_a_bottom_of_a_proposal_tail_is_refused():
    from smallhardface_amd import caffe
    txt = H.mini_detector(F.conv_layer("c0", "data", 128, 3, True), "c0", 8, 3, 8, 8) + L.norm_layer("n_tail", "cls_score_output", "y")
    with pytest.raises(Exception, match=r"Normalize 'n_tail'.*'cls_score_output'.*proposal tail"):
        caffe.Net(None, prototxt_text=txt)


def test_a_concat_whose_top_is_rewritten_copies():
    """An in-place Normalize on a Concat's top: the Concat copies (Caffe's bottoms keep their values)."""
    C, h, w = 8, 3, 5
    rng = np.random.default_rng(9)
    data = rng.integers(-4, 5, (1, 16, h, w)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    sc = rng.integers(1, 4, 2 * C).astype(F32)
    txt = H.single_layer_net(_bottoms() + F.concat_layer("cc", ["b0", "b1"]) + L.norm_layer("n", "cc"), 16, h, w)
    net = _net(txt, {"pre": G.feeder_params(16, False)[0]["pre"], "b0": [s0, np.zeros(C, F32)], "b1": [s1, np.zeros(C, F32)], "n": [sc]})
    _, prof = _profiled(net, lambda: _forward(net, data))
    assert prof[KERNEL] == 1 and prof["eltwise_combine"] == 2          # one copy per member
    cat = np.concatenate([data[:, p0], data[:, p1]], axis=1)
    _equal(_blob(net, "cc"), L.normalize32(cat, sc), "cc")
    _equal(_blob(net, "b0"), data[:, p0], "b0 keeps its values")
    _equal(_blob(net, "b1"), data[:, p1], "b1 keeps its values")


def _valid_net_text(h, w, C=16):
    return H.single_layer_net(G.conv_txt("pre", "data", C, 1) + G.conv_txt("g", "pre", C, 3, 1, 0, 1) + L.norm_layer("n", "g", "n", fill=2), C, h, w)


def test_a_refused_reshape_leaves_the_net_usable():
    C = 16
    rng = np.random.default_rng(5)
    wt = rng.integers(-2, 3, (C, C, 3, 3)).astype(F32)
    params = {"pre": G.feeder_params(C, False)[0]["pre"], "g": [wt, np.zeros(C, F32)]}
    net = _net(_valid_net_text(5, 6), params)

    def want(x):
        from oracle import oracle as O
        return L.normalize32(O.convolution(x, wt, None, pad=0), np.full(C, 2, F32))
    data = rng.integers(-4, 5, (1, C, 5, 6)).astype(F32)
    _equal(_forward(net, data)["n"], want(data), "first")
    small = np.zeros((1, C, 2, 6), F32)
    for _ in range(2):
        with pytest.raises(RuntimeError, match=r"Convolution 'g': kernel extent 3 .*padded input 2 x 6"):
            _forward(net, small)
    _equal(_forward(net, data)["n"], want(data), "back at the last good size")
    assert tuple(net.blobs["n"].shape) == (1, C, 3, 4)
    big = rng.integers(-4, 5, (1, C, 7, 9)).astype(F32)
    _equal(_forward(net, big)["n"], want(big), "a new size")
    assert tuple(net.blobs["n"].shape) == (1, C, 5, 7)


def test_caffemodel_blobs(tmp_path):
    from smallhardface_amd import caffe, caffemodel
    case = (12, 3, 5)
    data, sc = L.int_inputs(case)
    params, perm = L.n_params(case, sc)
    types = {"n": "Normalize"}
    for shared in (False, True):
        txt = L.layer_net_text(case, shared)
        p = dict(params, n=[np.array(-3.0, F32)]) if shared else params
        path = caffemodel.write_caffemodel(str(tmp_path / ("n%d.caffemodel" % shared)), p, layer_types=types)
        assert caffemodel.read_blob(path, "n", 0).shape == (() if shared else (12,))
        loaded = caffe.Net(None, path, caffe.TEST, prototxt_text=txt)
        assert tuple(loaded.params["n"][0].data.shape) == (() if shared else (12,)) and len(loaded.params["n"]) == 1
        _same(np.array(loaded.params["n"][0].data), p["n"][0], "the blob")
        _equal(_forward(loaded, data)["n"], L.normalize32(data[:, perm], p["n"][0], L.EPS, shared), "the forward")
    # a (1,) blob for the per-channel layer, a (12,) blob for the shared one, two blobs
    txt = L.layer_net_text(case, False)
    caffemodel.write_caffemodel(str(tmp_path / "one.caffemodel"), dict(params, n=[np.ones(1, F32)]), layer_types=types)
    with pytest.raises(Exception, match=r"Cannot copy param 0 weights from layer 'n'; shape mismatch"):
        caffe.Net(None, str(tmp_path / "one.caffemodel"), caffe.TEST, prototxt_text=txt)
    with pytest.raises(Exception, match=r"Cannot copy param 0 weights from layer 'n'; shape mismatch"):
        caffe.Net(None, str(tmp_path / "n0.caffemodel"), caffe.TEST, prototxt_text=L.layer_net_text(case, True))
    caffemodel.write_caffemodel(str(tmp_path / "two.caffemodel"), dict(params, n=[sc, sc]), layer_types=types)
    with pytest.raises(Exception, match=r"Incompatible number of blobs for layer n"):
        caffe.Net(None, str(tmp_path / "two.caffemodel"), caffe.TEST, prototxt_text=txt)


def test_fresh_blobs_are_the_fillers_and_commits_are_followed():
    """The filler's value is in Net.params before any load; blobs shared by `param { name: }` and by lanes; a commit is
    followed by the next forward."""
    from smallhardface_amd import caffe
    C, h, w = 8, 3, 5
    txt = H.single_layer_net(_bottoms() + L.norm_layer("a", "b0", "a", fill=10, pnames=["sc"]) + L.norm_layer("b", "b1", "b", pnames=["sc"]) +
                             L.norm_layer("plain", "b0", "plain") + L.norm_layer("sh", "b0", "sh", shared=True, fill=20) +
                             L.norm_layer("zero", "b0", "zero", filler='type: "constant"') +
                             L.norm_layer("gauss", "b0", "gauss", filler='type: "gaussian" std: 3'), 16, h, w)
    net = caffe.Net(None, prototxt_text=txt)
    shapes = {k: tuple(net.params[k][0].data.shape) for k in ("a", "b", "plain", "sh", "zero", "gauss")}
    assert shapes == {"a": (C,), "b": (C,), "plain": (C,), "sh": (), "zero": (C,), "gauss": (C,)}, shapes
    first = {k: np.array(net.params[k][0].data).reshape(-1) for k in shapes}
    assert (first["a"] == 10).all() and (first["b"] == 10).all() and (first["plain"] == 1).all() and (first["sh"] == 20).all()
    assert (first["zero"] == 0).all() and (first["gauss"] == 1).all()
    rng = np.random.default_rng(6)
    data = rng.integers(-4, 5, (1, 16, h, w)).astype(F32)
    s0, p0 = G.selection(C, 16, seed=5)
    s1, p1 = G.selection(C, 16, seed=6)
    H.load_params(net, {"pre": G.feeder_params(16, False)[0]["pre"], "b0": [s0, np.zeros(C, F32)], "b1": [s1, np.zeros(C, F32)]})
    lane = net.clone()
    _forward(lane, data)
    x0, x1 = data[:, p0], data[:, p1]
    _equal(_blob(lane, "a"), L.normalize32(x0, np.full(C, 10, F32)), "a")
    _equal(_blob(lane, "b"), L.normalize32(x1, np.full(C, 10, F32)), "b shares a's blob")
    _equal(_blob(lane, "plain"), L.normalize32(x0, np.ones(C, F32)), "plain")
    _equal(_blob(lane, "sh"), L.normalize32(x0, np.array(20, F32), L.EPS, True), "sh")
    assert (_blob(lane, "zero") == 0).all()
    new = rng.integers(1, 4, C).astype(F32)
    net.params["b"][0].data[...] = new              # the shared blob, through the second layer
    net.params["sh"][0].data[...] = -2
    net.commit_params()
    _forward(lane, data)
    _equal(_blob(lane, "a"), L.normalize32(x0, new), "a follows the commit")
    _equal(_blob(lane, "b"), L.normalize32(x1, new), "b follows the commit")
    _equal(_blob(lane, "sh"), L.normalize32(x0, np.array(-2, F32), L.EPS, True), "sh follows the commit")
