"""The detection tail (csrc/tail.hip: logits -> decode -> select -> sort -> gather -> append) beyond the templates' anchors and
beyond `synth_params` (run on an MI355X: ``pytest -m gpu``).

1. Decode / select / gather under four ProposalLayer param strings the templates never use (two and three ratios, shifts,
   unequal strides, base sizes 8 and 12, 'subsampled': False) on the vectors of tests/golden/proposal_geometry.npz, which
   the reference's own ProposalLayer produced and tests/test_oracle_golden.py holds the oracle to.  The assertions are those
   of tests/test_gpu_golden.py: probabilities bit-equal, boxes within BOX_TOL, the overflow flag, boxes inside the image.
   The same nets then run forward() with dense predictors, stage parity on identical inputs as in test_detector_end_to_end.

2. The fp32 logits kernel `tail_logits_kernel<false>` per element against float64.  The graph is data (C, h, w) -> one-hot
   1x1 convolutions (x * 1 + 0 * ... is exact in every conv mode: each head blob is a channel permutation of `data`, bit for
   bit, asserted) -> the predictors.  The reference is formed from `data` alone; the predictors' tops are the logits
   workspace re-ordered by the read-back path.  Weights are N(0, 1/sqrt(Cf)), every one of the 6A biases a distinct
   non-zero number.

   The bound is derived from the kernel, not measured.  A lane forms x.x*w.x + x.y*w.y + x.z*w.z + x.w*w.w (the file is
   built with -ffp-contract=off: four rounded products, three rounded additions), adds that to its partial sum once per
   128-channel chunk (Cf/128 additions), the 32 partial sums of a pixel meet in a 5-step butterfly (5 additions), and
   the bias is added (1).  A product therefore passes through at most 1 + 3 + Cf/128 + 5 + 1 = Cf/128 + 10 roundings, the
   bias through one, and with gamma_n = n u / (1 - n u) <= 1.01 n u for u = 2^-24 and these n

       |got - ref| <= 1.01 (Cf/128 + 10) 2^-24 (sum |x w| + |b|)        for every element.

   The count is read off the kernel (csrc/tail.hip, tail_logits_kernel).  A wrong row, anchor, channel or bias is O(1)
   against it; on an MI355X the largest |got - ref| / bound seen was 0.09 (Cf 128), 0.06 (256), 0.04 (512).  (The float64 reference's own error, about Cf 2^-53 of the same sum, is far below the 0.01 slack.)

3. One grouped pass whose members end differently -- candidates above the threshold, candidates cut by pre_nms_topN, none
   above the threshold (the single best valid anchor), none valid (the dummy roi and no score rows) -- through
   forward_group and through detect_add_levels / detect_export, in both member orders, against the members run alone.

4. Two graphs the reference cannot run are refused at construction with the proposal layer's name.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd.config import cfg
from tests import helpers as H
from tests.test_oracle_golden import GEOMETRIES, GEOMETRY_CASES, GEOMETRY_FACTS, geometry_case, proposal_params, rows_sorted

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4        # tests/test_gpu_parity.py
BOX_TOL = 1e-3          # px: device expf vs numpy's float32 exp differ in the last ulp; everything else is op for op
U32 = 2.0 ** -24        # unit roundoff of fp32
MODES = ["fp32", "f16x3"]


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _conv1(name, bottom, nout):
    return ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
            'kernel_size: 1 pad: 0 } }\n' % (name, bottom, name, nout))


def _perm(C, i):
    """Head i reads channel (c + 17 i) mod C of the input as its channel c."""
    return (np.arange(C) + 17 * i) % C


def _net(C, h, w, heads=0, A=8, param_str=None):
    """data (1, C, h, w) -> `heads` one-hot 1x1 convolutions c0, c1, ... (head i: the channel permutation `_perm(C, i)`)
    -> a mini-detector tail: the single-blob one on c0 (heads 0, 2A / 4A predictor outputs) or the per-blob one."""
    from smallhardface_amd import caffe
    n = max(heads, 1)
    layers = "".join(_conv1("c%d" % i, "data", C) for i in range(n))
    probe = "c0" if heads == 0 else ["c%d" % i for i in range(n)]
    net = caffe.Net(None, prototxt_text=H.mini_detector(layers, probe, 8, C, h, w, param_str=None if param_str is None
                                                        else (A, param_str)))
    for i in range(n):
        wt = np.zeros((C, C, 1, 1), np.float32)
        wt[np.arange(C), _perm(C, i), 0, 0] = 1.0
        net.params["c%d" % i][0].data[...] = wt
        net.params["c%d" % i][1].data[...] = 0
    return net


def _forward(net, data, info):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {k: np.array(v) for k, v in net.forward(data=data, im_info=info).items()}


def _dense_predictors(net, rng):
    """N(0, 1/sqrt(Cf)) predictor weights and N(0, 0.5) biases, no two of the 6A biases equal and none zero."""
    names = [n for n in net.params if n.startswith(("cls_score", "bbox_pred"))]
    biases = []
    for name in names:
        wb, bb = net.params[name]
        wb.data[...] = rng.normal(0, 1.0 / np.sqrt(wb.shape[1]), wb.shape).astype(np.float32)
        bb.data[...] = rng.normal(0, 0.5, bb.shape).astype(np.float32)
        biases.append(np.array(bb.data).ravel())
    b = np.concatenate(biases)
    assert len(np.unique(b)) == len(b) and np.all(b != 0)
    return names


def _blob(net, name):
    return np.array(net.blobs[name].data)


# ---- 1. decode / select / gather under other param strings --------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry_nets(golden):
    g = golden("proposal_geometry.npz")
    nets = {}
    for name in GEOMETRIES:
        sc = g[name + "_ms0_scores"]
        nets[name] = _net(128, sc.shape[2], sc.shape[3], A=GEOMETRY_FACTS[name][0], param_str=str(g[name + "_ms0_param_str"]))
    return nets


def _geometry_of(case):
    return [n for n in GEOMETRIES if case.startswith(n)][0]


def _all_sides(sc, dl, ii, pstr):
    """ws, hs of every box the min-size filter judges (after the anchor subsampling), by the oracle."""
    b, _ = O.proposal_forward(sc, dl, ii, proposal_params(pstr, min_size=0, score_thresh=-1.0, pre_nms_topN=0))
    return np.concatenate([b[:, 3] - b[:, 1] + 1, b[:, 4] - b[:, 2] + 1])


@pytest.mark.parametrize("case", GEOMETRY_CASES)
def test_hip_tail_on_reference_vectors_of_other_geometries(golden, geometry_nets, case):
    g = golden("proposal_geometry.npz")
    net = geometry_nets[_geometry_of(case)]
    sc, dl, ii, pp, gb, gp = geometry_case(g, case)
    if pp.min_size:
        # device expf and numpy's exp may differ in the last ulp: no side lies within 0.01 px of the cut, so the kept sets
        # must be equal
        assert np.abs(_all_sides(sc, dl, ii, g[case + "_param_str"]) - pp.min_size * ii[0, 2]).min() > 0.01
    try:
        net.set_proposal_cfg(10000, 0.002, pp.min_size)
        boxes, probs, overflow = net.debug_proposal(sc, dl, ii)
    finally:
        net._apply_cfg()
    assert boxes.shape == gb.shape and probs.shape == gp.shape
    assert overflow == ("overflow" in case)           # np.seterr(over='raise') -> clamp branch, bbox_transform.py:52-65
    ties = len(np.unique(gp[:, 1])) != gp.shape[0]
    np.testing.assert_array_equal(probs[:, 1], gp[:, 1])
    assert np.all(boxes[:, 0] == 0)
    if not ties:
        np.testing.assert_array_equal(probs, gp)
        assert np.abs(boxes - gb).max() < BOX_TOL
    ob, op = O.proposal_forward(sc, dl, ii, pp)
    np.testing.assert_array_equal(probs, op)
    assert np.abs(boxes - ob).max() < BOX_TOL
    a = rows_sorted(np.hstack([probs, np.round(boxes, 2)]))
    b = rows_sorted(np.hstack([gp, np.round(gb, 2)]))
    assert np.abs(a - b).max() < 0.011
    assert boxes[:, [1, 3]].max() <= ii[0, 1] - 1 and boxes[:, [2, 4]].max() <= ii[0, 0] - 1 and boxes[:, 1:].min() >= 0


# seeds under which, by float64 logits on the host, no box side lies within 0.05 px of the min-size cut of 9 px (the test
# asserts 0.01 px on what the GPU produced)
DENSE_SEEDS = {"two_ratios_mixed_strides": 27, "shifts_two_strides": 12, "three_ratios_dense": 21, "strides_4_8_16": 14}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("min_size", [0, 6])
@pytest.mark.parametrize("name", GEOMETRIES)
def test_forward_on_other_geometries_with_dense_predictors(golden, geometry_nets, name, min_size, mode):
    """forward() of the same nets: dense predictors with distinct biases feed the decode, which is held to the oracle on
    the probabilities and deltas the GPU itself produced (stage parity on identical inputs)."""
    g = golden("proposal_geometry.npz")
    net = geometry_nets[name]
    pstr, ii = g[name + "_ms0_param_str"], g[name + "_ms0_im_info"]
    A = GEOMETRY_FACTS[name][0]
    h, w = g[name + "_ms0_scores"].shape[2:]
    rng = np.random.default_rng(DENSE_SEEDS[name])
    _dense_predictors(net, rng)
    data = rng.normal(0, 1, (1, 128, h, w)).astype(np.float32)
    cfg.TEST.ANCHOR_MIN_SIZE = min_size
    net.set_conv_mode(mode)
    try:
        out = _forward(net, data, ii)
        gp, gd = _blob(net, "cls_prob_reshape_output"), _blob(net, "bbox_pred_output")
    finally:
        net.set_conv_mode("fp32")
    assert gp.shape == (1, 2 * A, h, w) and gd.shape == (1, 4 * A, h, w)
    np.testing.assert_array_equal(_blob(net, "c0"), data)
    if min_size:
        assert np.abs(_all_sides(gp, gd, ii, pstr) - min_size * ii[0, 2]).min() > 0.01
    pb, ps = O.proposal_forward(gp, gd, ii, proposal_params(pstr, min_size=min_size))
    gb, gs = out["boxes"], out["cls_prob"]
    print("%s min_size %d %s: %d rows of %d anchors" % (name, min_size, mode, len(ps), h * w * A))
    assert len(ps) > 1
    assert gb.shape == pb.shape and gs.shape == ps.shape
    np.testing.assert_array_equal(gs, ps)
    assert np.abs(gb - pb).max() < BOX_TOL
    assert gb[:, [1, 3]].max() <= ii[0, 1] - 1 and gb[:, [2, 4]].max() <= ii[0, 0] - 1 and gb[:, 1:].min() >= 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("row,clamped", [(2, True), (3, False)], ids=["dw", "dh"])
def test_forward_overflow_flag_on_a_non_square_anchor(golden, geometry_nets, row, clamped, mode):
    """The flag the logits kernel itself raises.  Anchor 0 of `two_ratios_mixed_strides` is 22 wide and 12 high: a delta of
    85.9 overflows fp32 as exp(dw) * 22 (85.9 + ln 22 = 88.99 > ln FLT_MAX = 88.72) but not as exp(dh) * 12 (88.38), so dw
    clamps every delta above 50 to 5 (bbox_transform.py:52-65) and dh clamps nothing.  A zero weight row and a bias make
    the delta exact; under an im_info of 6000 x 8000 a clamped box ends inside the image, an unclamped one at its border."""
    g = golden("proposal_geometry.npz")
    name = "two_ratios_mixed_strides"
    net, A = geometry_nets[name], GEOMETRY_FACTS[name][0]
    pstr = g[name + "_ms0_param_str"]
    h, w = g[name + "_ms0_scores"].shape[2:]
    rng = np.random.default_rng(31)
    _dense_predictors(net, rng)
    for r, v in ((row, 85.9), (4 * 2 + 3, 60.0)):        # anchor 0's dw or dh; dh of anchor 2 (24 high)
        net.params["bbox_pred"][0].data[r] = 0
        net.params["bbox_pred"][1].data[r] = v
    data = rng.normal(0, 1, (1, 128, h, w)).astype(np.float32)
    ii = np.array([[6000, 8000, 1.5]], np.float32)
    net.set_conv_mode(mode)
    try:
        out = _forward(net, data, ii)
        gp, gd = _blob(net, "cls_prob_reshape_output"), _blob(net, "bbox_pred_output")
    finally:
        net.set_conv_mode("fp32")
    np.testing.assert_array_equal(gd[0, row], np.float32(85.9))
    np.testing.assert_array_equal(gd[0, 11], np.float32(60.0))
    assert np.abs(np.delete(gd[0], [row, 11], axis=0)).max() < 20
    pb, ps = O.proposal_forward(gp, gd, ii, proposal_params(pstr))
    gb, gs = out["boxes"], out["cls_prob"]
    assert gb.shape == pb.shape and len(ps) > 20
    np.testing.assert_array_equal(gs, ps)
    assert np.abs(gb - pb).max() < BOX_TOL
    at_border = int((gb[:, 4] == ii[0, 0] - 1).sum()) + int((gb[:, 3] == ii[0, 1] - 1).sum())
    assert (at_border == 0) == clamped, at_border


# ---- 2. the fp32 logits kernel per element ------------------------------------------------------------------------------------
# (heads, A, Cf): heads 0 = the single-blob layout (rows cls*A + a / a*4 + j of two predictors), else one predictor pair per blob
LOGIT_NETS = [(0, 8, 128), (0, 8, 256), (0, 8, 512), (2, 2, 512), (3, 3, 256), (8, 8, 128)]
LOGIT_SIZES = [(5, 7), (1, 1), (6, 8)]     # K odd (the last wave's second pixel is empty), one pixel, K even
_logit_nets = {}


def _logit_net(heads, A, Cf):
    """One net per layout, built at 6 x 8 and reshaped per case; dense predictors loaded once."""
    key = (heads, A, Cf)
    if key not in _logit_nets:
        net = _net(Cf, 6, 8, heads=heads, A=A)
        _dense_predictors(net, np.random.default_rng(1000 + 10 * heads + Cf))
        _logit_nets[key] = net
    return _logit_nets[key]


def _conv1_ref(x, wt, bs):
    """(w x + b, |w| |x| + |b|) in float64; x (C, h, w), wt (N, C, 1, 1), bs (N,) -> (N, h, w) each."""
    C, h, w = x.shape
    xd = x.astype(np.float64).reshape(C, -1)
    wd = wt.astype(np.float64).reshape(wt.shape[0], C)
    bd = bs.astype(np.float64)[:, None]
    return (wd @ xd + bd).reshape(-1, h, w), (np.abs(wd) @ np.abs(xd) + np.abs(bd)).reshape(-1, h, w)


def _check_logits(net, heads, A, Cf, data, what):
    """Every predictor top of `net` (forwarded on `data`) within the derived bound of its float64 value; the softmax blob
    within SCORE_TOL of the float64 softmax; the delta blob the proposal layer reads bit-equal to the predictors' tops."""
    h, w = data.shape[2:]
    pairs = [("cls_score", "bbox_pred", 0)] if heads == 0 else [("cls_score_%d" % i, "bbox_pred_%d" % i, i) for i in range(heads)]
    worst = 0.0
    cls_ref, box_got = [], []
    for cn, bn, i in pairs:
        x = data[0][_perm(Cf, i)]
        for name in (cn, bn):
            wt, bs = np.array(net.params[name][0].data), np.array(net.params[name][1].data)
            ref, mag = _conv1_ref(x, wt, bs)
            got = _blob(net, name + "_output")[0]
            assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
            assert np.isfinite(got).all()
            bound = 1.01 * (Cf // 128 + 10) * U32 * mag
            err = np.abs(got.astype(np.float64) - ref)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert (err <= bound).all(), (what, name, ratio, float(err.max()))
            if name == cn:
                cls_ref.append(ref)
            else:
                box_got.append(got)
                assert np.abs(ref[2::4]).max() < 20 and np.abs(ref[3::4]).max() < 20      # dw, dh far below overflow
    print("LOGITS %s Cf %d: worst |got - ref| / bound %.3f" % (what, Cf, worst))
    # softmax over (bg, fg) per anchor; channel cls * A + a of the blob the proposal layer reads
    lg = np.concatenate(cls_ref) if heads else cls_ref[0]
    lg = lg.reshape(A, 2, h, w).transpose(1, 0, 2, 3) if heads else lg.reshape(2, A, h, w)
    e = np.exp(lg - lg.max(axis=0, keepdims=True))
    prob = (e / e.sum(axis=0, keepdims=True)).reshape(2 * A, h, w)
    gp = _blob(net, "cls_prob_reshape_output")
    assert gp.shape == (1, 2 * A, h, w)
    assert np.abs(gp[0] - prob).max() < SCORE_TOL
    np.testing.assert_array_equal(_blob(net, "bbox_pred_output")[0], np.concatenate(box_got))
    for i in range(max(heads, 1)):
        np.testing.assert_array_equal(_blob(net, "c%d" % i)[0], data[0][_perm(Cf, i)])
    return worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", LOGIT_SIZES)
@pytest.mark.parametrize("heads,A,Cf", LOGIT_NETS)
def test_fp32_logits_kernel_per_element(heads, A, Cf, h, w, mode):
    net = _logit_net(heads, A, Cf)
    data = np.random.default_rng(Cf + 10 * h + w).normal(0, 1, (1, Cf, h, w)).astype(np.float32)
    net.set_conv_mode(mode)
    try:
        _forward(net, data, np.array([[8 * h, 8 * w, 1]], np.float32))
        _check_logits(net, heads, A, Cf, data, "%s heads %d A %d %dx%d" % (mode, heads, A, h, w))
    finally:
        net.set_conv_mode("fp32")


@pytest.mark.parametrize("mode", MODES)
def test_fp32_logits_kernel_per_element_in_a_group(mode):
    """Three members of different sizes in one launch: each against the reference of its own input."""
    heads, A, Cf = 0, 8, 256
    root = _logit_net(heads, A, Cf)
    members = [root, root.clone(), root.clone()]
    datas = [np.random.default_rng(70 + k).normal(0, 1, (1, Cf, h, w)).astype(np.float32) for k, (h, w) in enumerate(LOGIT_SIZES)]
    inputs = []
    for m, d in zip(members, datas):
        m.blobs["data"].reshape(*d.shape)
        m.blobs["im_info"].reshape(1, 3)
        inputs.append({"data": d, "im_info": np.array([[8 * d.shape[2], 8 * d.shape[3], 1]], np.float32)})
    root.set_conv_mode(mode)
    try:
        root.forward_group(members, inputs)
        for k, (m, d) in enumerate(zip(members, datas)):
            _check_logits(m, heads, A, Cf, d, "%s group member %d %dx%d" % (mode, k, d.shape[2], d.shape[3]))
    finally:
        root.set_conv_mode("fp32")


# ---- 3. members of one group that end differently -----------------------------------------------------------------------------
END_A, END_C = 8, 128
END_TOPN, END_MIN_SIZE, END_THRESH = 100, 2.0, 0.05
# name -> (h, w, im_info scale): `many` stays below pre_nms_topN (96 anchors), `cut` is cut by it (504 anchors), `best` has
# nothing above SCORE_THRESH, `none` has nothing valid (min size 2 px x scale 1000)
ENDINGS = {"many": (3, 4, 1.0), "cut": (7, 9, 1.0), "best": (5, 7, 1.0), "none": (4, 4, 1000.0)}
END_PARAMS = dict(feat_stride=[8] * END_A, scales=list(range(1, END_A + 1)), ratios=[1], pre_nms_topN=END_TOPN,
                  min_size=END_MIN_SIZE)


def _ending_net():
    """Single-blob tail on the identity head c0 with one-hot predictor rows and zero biases: per anchor a the logits are
    channels 4a (bg), 4a + 1 (fg), 4a + 2 (dx), 4a + 3 (dy), 32 + 2a (dw), 33 + 2a (dh) of the input, exactly."""
    net = _net(END_C, 7, 9, A=END_A)
    A = END_A
    wc = np.zeros((2 * A, END_C, 1, 1), np.float32)
    wb = np.zeros((4 * A, END_C, 1, 1), np.float32)
    for a in range(A):
        wc[a, 4 * a] = wc[A + a, 4 * a + 1] = 1.0
        wb[4 * a, 4 * a + 2] = wb[4 * a + 1, 4 * a + 3] = 1.0
        wb[4 * a + 2, 32 + 2 * a] = wb[4 * a + 3, 33 + 2 * a] = 1.0
    for name, wt in (("cls_score", wc), ("bbox_pred", wb)):
        net.params[name][0].data[...] = wt
        net.params[name][1].data[...] = 0
    return net


def _ending_input(name):
    h, w, scale = ENDINGS[name]
    rng = np.random.default_rng(sorted(ENDINGS).index(name) + 40)
    x = rng.normal(0, 0.3, (1, END_C, h, w)).astype(np.float32)
    fg = slice(1, 4 * END_A, 4)
    bg = slice(0, 4 * END_A, 4)
    x[0, bg] = 0
    x[0, fg] = rng.normal(0, 2.0, (END_A, h, w))
    if name == "best":
        x[0, bg] = 10
        x[0, fg] = -10 + rng.normal(0, 0.5, (END_A, h, w))
    return x, np.array([[8 * h - 3, 8 * w - 5, scale]], np.float32)


def _ending_oracle(net, info):
    """The oracle's proposal layer on the probabilities and deltas this net's last pass left."""
    gp, gd = _blob(net, "cls_prob_reshape_output"), _blob(net, "bbox_pred_output")
    sides = _all_sides(gp, gd, info, repr({k: END_PARAMS[k] for k in ("feat_stride", "scales", "ratios")}))
    assert np.abs(sides - END_MIN_SIZE * info[0, 2]).min() > 0.01      # the kept set does not hinge on exp()'s last ulp
    return O.proposal_forward(gp, gd, info, O.ProposalParams(**END_PARAMS))


@pytest.fixture(scope="module")
def ending_lanes():
    root = _ending_net()
    return [root] + [root.clone() for _ in range(len(ENDINGS))]


@pytest.mark.parametrize("mode", MODES)
def test_three_endings_in_one_group(ending_lanes, mode):
    import torch
    root, lanes = ending_lanes[0], ending_lanes[1:]
    cfg.TEST.N_DETS_PER_MODULE = END_TOPN
    cfg.TEST.ANCHOR_MIN_SIZE = END_MIN_SIZE
    inputs = {name: _ending_input(name) for name in ENDINGS}
    buf = torch.zeros((4096, 5), dtype=torch.float32, device="cuda")
    root.set_conv_mode(mode)
    try:
        # every unit alone on the root net: forward(), and the fused per-image path
        single, single_rows = {}, {}
        for name, (x, info) in inputs.items():
            h, w, scale = ENDINGS[name]
            out = _forward(root, x, info)
            np.testing.assert_array_equal(_blob(root, "bbox_pred_output")[0, 2::4], x[0, 32:32 + 2 * END_A:2])   # dw: the input itself
            ob, op = _ending_oracle(root, info)
            assert out["boxes"].shape == ob.shape and out["cls_prob"].shape == op.shape, name
            np.testing.assert_array_equal(out["cls_prob"], op)
            assert np.abs(out["boxes"] - ob).max() < BOX_TOL
            single[name] = out
            root.detect_begin()
            root.detect_add_level(x, h, w, int(info[0, 0]), int(info[0, 1]), scale, name == "cut", END_THRESH)
            n = root.detect_export(buf.data_ptr(), buf.shape[0])
            single_rows[name] = buf[:n].cpu().numpy()
        assert len(single["many"]["cls_prob"]) > 20 and single["many"]["cls_prob"][-1, 1] >= cfg.TEST.SCORE_THRESH
        assert len(single["many"]["cls_prob"]) < END_TOPN == len(single["cut"]["cls_prob"])
        assert single["best"]["cls_prob"].shape == (1, 2) and single["best"]["cls_prob"][0, 1] < cfg.TEST.SCORE_THRESH
        np.testing.assert_array_equal(single["none"]["boxes"], [[0, 0, 0, 16, 16]])
        assert single["none"]["cls_prob"].shape == (0, 2)
        assert len(single_rows["many"]) > 0 and len(single_rows["cut"]) > 0
        assert len(single_rows["best"]) == 0 and len(single_rows["none"]) == 0
        for order in (["none", "many", "best", "cut"], ["cut", "best", "many", "none"]):
            members = lanes[:len(order)]
            ins = []
            for m, name in zip(members, order):
                x, info = inputs[name]
                m.blobs["data"].reshape(*x.shape)
                m.blobs["im_info"].reshape(1, 3)
                ins.append({"data": x, "im_info": info})
            outs = root.forward_group(members, ins)
            for m, name, out in zip(members, order, outs):
                for key in ("boxes", "cls_prob"):
                    assert out[key].shape == single[name][key].shape, (order, name, key)
                    np.testing.assert_array_equal(out[key], single[name][key], err_msg="%s %s" % (name, key))
                    np.testing.assert_array_equal(m.blobs[key].data, single[name][key])
                ob, op = _ending_oracle(m, inputs[name][1])
                assert out["boxes"].shape == ob.shape
                np.testing.assert_array_equal(out["cls_prob"], op)
                assert np.abs(out["boxes"] - ob).max() < BOX_TOL
            # the same units through the fused per-image path: one list, the members' rows in order
            units = [(inputs[name][0], ENDINGS[name][0], ENDINGS[name][1], int(inputs[name][1][0, 0]), int(inputs[name][1][0, 1]),
                      ENDINGS[name][2], name == "cut") for name in order]
            root.detect_begin()
            root.detect_add_levels(members, units, END_THRESH)
            n = root.detect_export(buf.data_ptr(), buf.shape[0])
            want = np.concatenate([single_rows[name] for name in order])
            assert n == len(want) == root.detect_count()
            np.testing.assert_array_equal(buf[:n].cpu().numpy(), want)
            # ... and each member's own list
            root.detect_add_levels(members, units, END_THRESH, per_member_lists=True)
            root.sync()
            for m, name in zip(members, order):
                n = m.detect_export(buf.data_ptr(), buf.shape[0])
                np.testing.assert_array_equal(buf[:n].cpu().numpy(), single_rows[name], err_msg=name)
    finally:
        root.set_conv_mode("fp32")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_too_few_feat_strides_are_refused_at_construction():
    """'subsampled' true indexes feat_stride[i // len(shifts)**2] for every anchor i (proposal_layer.py:160-165): the reference
    and the oracle raise IndexError on fewer entries (tests/test_oracle_golden.py); the runtime once clamped the index."""
    from smallhardface_amd import caffe, prototxt as P
    layers = _conv1("c0", "data", 128)
    bad = "{'feat_stride': [8,8], 'scales': [2,3], 'ratios': [0.5,2], 'base_size': 8}"
    with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal': feat_stride has 2 entries.*indexes 4"):
        caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9, param_str=(4, bad)))
    with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal': feat_stride has 1 entries.*indexes 2"):
        caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9, param_str=(
            8, "{'feat_stride': [8], 'scales': [1], 'ratios': [0.5,2], 'shifts': [0,0.5]}")))
    with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal': feat_stride entries must not be smaller"):
        caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9, param_str=(
            2, "{'feat_stride': [16,8], 'scales': [1,2], 'ratios': [1,]}")))
    with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal': feat_stride entries must be in"):
        caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9, param_str=(
            2, "{'feat_stride': [0,8], 'scales': [1,2], 'ratios': [1,]}")))
    # the process lives on; the same anchors are accepted without the subsampling map, with enough strides, and so are the
    # graphs every other test builds: both templates and the mini-detector, A equal entries each
    ok = "{'feat_stride': [8,8], 'scales': [2,3], 'ratios': [0.5,2], 'base_size': 8, 'subsampled': False}"
    caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9, param_str=(4, ok)))
    caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9, param_str=(4, bad.replace("[8,8]", "[8,8,8,8]"))))
    caffe.Net(None, prototxt_text=H.mini_detector(layers, "c0", 8, 128, 7, 9))
    caffe.Net(None, prototxt_text=H.mini_detector(_conv1("c0", "data", 128) + _conv1("c1", "data", 128), ["c0", "c1"], 8, 128, 7, 9))
    for dd in (True, False):
        net = caffe.Net(None, prototxt_text=P.dumps(H.detector_msg(dd)))
        assert "boxes" in net.blobs


def test_heads_of_different_widths_are_refused_at_construction():
    """The per-head tail packs Cf weights per row and reads Cf channels of every head blob, Cf taken from the first head:
    a second head of another width would be read (or its weights copied) out of bounds."""
    from smallhardface_amd import caffe
    for c0, c1 in ((128, 256), (256, 128)):
        layers = _conv1("c0", "data", c0) + _conv1("c1", "data", c1)
        with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal': head blobs 'c0' and 'c1' differ in channel count \(%d vs %d\)" % (c0, c1)):
            caffe.Net(None, prototxt_text=H.mini_detector(layers, ["c0", "c1"], 8, 128, 7, 9))
    layers = _conv1("c0", "data", 128) + _conv1("c1", "data", 128)
    net = caffe.Net(None, prototxt_text=H.mini_detector(layers, ["c0", "c1"], 8, 128, 7, 9))
    assert "boxes" in net.blobs
