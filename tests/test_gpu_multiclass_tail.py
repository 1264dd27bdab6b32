"""A class count C > 2 through the proposal tail on the Net.forward / Net.forward_group path (run on an MI355X:
``pytest -m gpu``): graph construction and its refusals, the tail on the reference's own multi-class vectors
(tests/golden/proposal_multiclass.npz), the logits kernel per element, whole forwards against the oracle net, grouped
forwards, the driver's class loop, and the refusal of the fused per-image path.

The logits bound is the one tests/test_gpu_tail_geometry.py derives from the kernel, and it carries over because the
reduction is the same for every one of the C + 4 rows of an anchor: a lane forms x.x*w.x + x.y*w.y + x.z*w.z + x.w*w.w
(-ffp-contract=off: four rounded products, three rounded additions), adds it to its partial sum once per 128-channel chunk
(Cf/128 additions), the 32 partial sums of a pixel meet in a 5-step butterfly, and the bias is added last: a product passes
through at most Cf/128 + 10 roundings, so |got - ref| <= 1.01 (Cf/128 + 10) 2^-24 (sum |x w| + |b|) per element.  Conv mode
"f64" forms the sum in binary64 and rounds once: it is far inside the same bound.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import helpers as H
from tests import multiclass_cases as M

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4        # tests/test_gpu_parity.py
BOX_TOL = 1e-3          # px, tests/test_gpu_tail_geometry.py: device expf vs numpy's float32 exp differ in the last ulp
U32 = 2.0 ** -24
MODES = ["fp32", "f16x3"]


def _perm(C, i):
    return (np.arange(C) + 17 * i) % C


def _one_hot_net(Cf, h, w, C, A, per_head):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=M.one_hot_net_txt(Cf, h, w, C, A, per_head))
    for i in range(A if per_head else 1):
        wt = np.zeros((Cf, Cf, 1, 1), np.float32)
        wt[np.arange(Cf), _perm(Cf, i), 0, 0] = 1.0
        net.params["c%d" % i][0].data[...] = wt
        net.params["c%d" % i][1].data[...] = 0
    return net


def _forward(net, data, info):
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    return {k: np.array(v) for k, v in net.forward(data=data, im_info=info).items()}


def _blob(net, name):
    return np.array(net.blobs[name].data)


# ---- 1. construction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_head", [True, False], ids=["per_head", "single_blob"])
def test_three_class_graphs_load_and_report_their_class_count(per_head):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 3, 3, per_head))
    assert net.num_classes == 3 and net.clone().num_classes == 3
    assert net.blobs["cls_prob"].shape[1] == 3
    two = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 2, 3, per_head))
    assert two.num_classes == 2
    for dd in (True, False):
        assert caffe.Net(None, prototxt_text=P.dumps(H.detector_msg(dd))).num_classes == 2
    plain = caffe.Net(None, prototxt_text=H.single_layer_net(M.conv1("c0", "data", 128), 128))
    assert plain.num_classes == 0


REFUSALS = [
    # (per_head, C, A, overrides, message)
    (False, 3, 8, dict(cls_nout=20, pre_dim=3, final_dim=24), r"'cls_score' has 20 outputs, not a multiple of the 8 anchors"),
    (True, 3, 3, dict(cls_nout=[3, 4, 3]), r"'cls_score_0' and 'cls_score_1' disagree on the class count \(3 vs 4\)"),
    (False, 3, 3, dict(pre_dim=2), r"Reshape 'cls_reshape' makes 2 class planes, the predictor has 3 classes"),
    (False, 3, 3, dict(final_dim=6), r"Reshape 'cls_prob_reshape' makes 6 channels, the predictors give 3 classes x 3 anchors"),
    (True, 3, 3, dict(final_dim=6), r"Reshape 'cls_prob_reshape' makes 6 channels, the predictors give 3 classes x 3 anchors"),
    (True, 1, 3, dict(), r"at least 2 classes .* the predictors have 1"),
    (False, 1, 3, dict(), r"at least 2 classes .* the predictors have 1"),
    (True, 9, 3, dict(), r"9 classes: the tail supports at most 8"),
    (False, 9, 3, dict(), r"9 classes: the tail supports at most 8"),
]


@pytest.mark.parametrize("per_head,C,A,kw,message", REFUSALS)
def test_inconsistent_class_counts_are_refused_at_construction(per_head, C, A, kw, message):
    from smallhardface_amd import caffe
    with pytest.raises(RuntimeError, match=r"ProposalLayer 'proposal': .*" + message):
        caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, C, A, per_head, **kw))
    # the process lives on: the cap itself is accepted
    assert caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 8, A, per_head)).num_classes == 8


def test_refinement_bottoms_and_num_feats_stay_refused():
    from smallhardface_amd import caffe
    txt = M.one_hot_net_txt(128, 7, 9, 3, 3, False)
    with pytest.raises(RuntimeError, match="num_feats != 1 unsupported"):
        caffe.Net(None, prototxt_text=txt.replace("'ratios':[1,]}", "'ratios':[1,], 'num_feats': 2}"))
    with pytest.raises(RuntimeError, match=r"expected bottoms \(cls_prob, bbox_pred, im_info\)"):
        caffe.Net(None, prototxt_text=txt.replace('bottom: "cls_prob_reshape_output" bottom: "bbox_pred_output"',
                                                  'bottom: "bbox_pred_output" bottom: "cls_prob_reshape_output" bottom: "bbox_pred_output"'))


# ---- 2. the tail on the reference's vectors --------------------------------------------------------------------------------------
_fixture_nets = {}


def _fixture_net(C, A):
    if (C, A) not in _fixture_nets:
        _fixture_nets[(C, A)] = _one_hot_net(128, 7, 9, C, A, False)
    return _fixture_nets[(C, A)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", M.CASES)
def test_hip_tail_on_reference_multiclass_vectors(golden, case, mode):
    g = golden("proposal_multiclass.npz")
    sc, dl, ii, pp, (topn, thresh, min_size), gb, gp = M.fixture_case(g, case)
    C, A = (int(v) for v in g[case + "_classes"])
    net = _fixture_net(C, A)
    net.set_conv_mode(mode)
    try:
        net.set_proposal_cfg(topn, thresh, min_size)
        boxes, probs, overflow = net.debug_proposal(sc, dl, ii)
    finally:
        net._apply_cfg()
        net.set_conv_mode("fp32")
    assert not overflow
    assert boxes.shape == gb.shape and probs.shape == gp.shape == (len(gp), C)        # row count
    assert net.blobs["cls_prob"].shape == gp.shape
    if case == "none_valid":
        np.testing.assert_array_equal(boxes, [[0, 0, 0, 16, 16]])                     # the dummy roi
        assert probs.shape == (0, C)
        return
    ob, op = O.proposal_forward(sc, dl, ii, pp)
    np.testing.assert_array_equal(probs, op)            # the oracle's canonical order: ties by anchor index
    assert np.abs(boxes - ob).max() < BOX_TOL
    if case == "tie_classes":
        # argsort()[::-1] leaves the two tied rows' order to numpy: the pair as a set, the rest row for row
        assert probs[0].tolist() == [0.125, 0.75, 0.125] and probs[1].tolist() == [0.125, 0.125, 0.75]
        np.testing.assert_array_equal(M.rows_sorted(probs[:2]), M.rows_sorted(gp[:2]))
        a, b = M.rows_sorted(np.hstack([probs[:2], np.round(boxes[:2], 2)])), M.rows_sorted(np.hstack([gp[:2], np.round(gb[:2], 2)]))
        assert np.abs(a - b).max() < 0.011
        probs, gp, boxes, gb = probs[2:], gp[2:], boxes[2:], gb[2:]
    np.testing.assert_array_equal(probs, gp)            # scores bit-equal
    assert np.abs(boxes - gb).max() < BOX_TOL
    assert np.all(boxes[:, 0] == 0)


# ---- 3. the logits kernel per element --------------------------------------------------------------------------------------------
LOGIT_SIZES = [(5, 7), (6, 8)]      # K odd (the last wave's second pixel is empty), K even
_logit_nets = {}


def _logit_net(per_head, C, A, Cf):
    key = (per_head, C, A, Cf)
    if key not in _logit_nets:
        net = _one_hot_net(Cf, 6, 8, C, A, per_head)
        rng = np.random.default_rng(2000 + 100 * C + 10 * A + Cf + int(per_head))
        biases = []
        for name in [n for n in net.params if n.startswith(("cls_score", "bbox_pred"))]:
            wb, bb = net.params[name]
            wb.data[...] = rng.normal(0, 1.0 / np.sqrt(wb.shape[1]), wb.shape).astype(np.float32)
            bb.data[...] = rng.normal(0, 0.5, bb.shape).astype(np.float32)
            biases.append(np.array(bb.data).ravel())
        b = np.concatenate(biases)
        assert len(b) == (C + 4) * A and len(np.unique(b)) == len(b) and np.all(b != 0)
        _logit_nets[key] = net
    return _logit_nets[key]


def _conv1_ref(x, wt, bs):
    Cf, h, w = x.shape
    xd = x.astype(np.float64).reshape(Cf, -1)
    wd = wt.astype(np.float64).reshape(wt.shape[0], Cf)
    bd = bs.astype(np.float64)[:, None]
    return (wd @ xd + bd).reshape(-1, h, w), (np.abs(wd) @ np.abs(xd) + np.abs(bd)).reshape(-1, h, w)


@pytest.mark.parametrize("mode", MODES + ["f64"])
@pytest.mark.parametrize("Cf", [128, 256])
@pytest.mark.parametrize("A", [1, 8])
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("per_head", [True, False], ids=["per_head", "single_blob"])
def test_logits_kernel_per_element_with_more_classes(per_head, C, A, Cf, mode):
    net = _logit_net(per_head, C, A, Cf)
    assert net.num_classes == C
    pairs = ([("cls_score_%d" % i, "bbox_pred_%d" % i, i) for i in range(A)] if per_head else [("cls_score", "bbox_pred", 0)])
    net.set_conv_mode(mode)
    try:
        for h, w in LOGIT_SIZES:
            data = np.random.default_rng(Cf + 10 * h + w + C).normal(0, 1, (1, Cf, h, w)).astype(np.float32)
            _forward(net, data, np.array([[8 * h, 8 * w, 1]], np.float32))
            worst, cls_ref, box_got = 0.0, [], []
            for cn, bn, i in pairs:
                x = data[0][_perm(Cf, i)]
                np.testing.assert_array_equal(_blob(net, "c%d" % i)[0], x)
                for name in (cn, bn):
                    ref, mag = _conv1_ref(x, np.array(net.params[name][0].data), np.array(net.params[name][1].data))
                    got = _blob(net, name + "_output")[0]
                    assert got.shape == ref.shape and np.isfinite(got).all(), (name, got.shape, ref.shape)
                    bound = 1.01 * (Cf // 128 + 10) * U32 * mag
                    err = np.abs(got.astype(np.float64) - ref)
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (name, h, w, float((err / bound).max()))
                    (cls_ref if name == cn else box_got).append(ref if name == cn else got)
            print("LOGITS %s %s C %d A %d Cf %d %dx%d: worst |got - ref| / bound %.3f"
                  % (mode, "per-head" if per_head else "single-blob", C, A, Cf, h, w, worst))
            # the softmax over the C classes of an anchor; channel c * A + a of the blob the proposal layer reads
            lg = np.stack(cls_ref, axis=1) if per_head else cls_ref[0].reshape(C, A, h, w)       # (C, A, h, w)
            e = np.exp(lg - lg.max(axis=0, keepdims=True))
            prob = (e / e.sum(axis=0, keepdims=True)).reshape(C * A, h, w)
            gp = _blob(net, "cls_prob_reshape_output")
            assert gp.shape == (1, C * A, h, w)
            assert np.abs(gp[0] - prob).max() < SCORE_TOL
            np.testing.assert_array_equal(_blob(net, "cls_prob_output").reshape(gp.shape), gp)
            np.testing.assert_array_equal(_blob(net, "bbox_pred_output")[0], np.concatenate(box_got))
            # the pre-softmax (1, C, A*h, w) planes are the same logits, re-ordered
            pre = _blob(net, "cls_score_reshape_output")
            assert pre.shape == (1, C, A * h, w)
            got_lg = (np.stack([_blob(net, cn + "_output")[0] for cn, _, _ in pairs], axis=1) if per_head
                      else _blob(net, "cls_score_output")[0].reshape(C, A, h, w))
            np.testing.assert_array_equal(pre[0], got_lg.reshape(C, A * h, w))
    finally:
        net.set_conv_mode("fp32")


# ---- 4. whole forwards against the oracle net --------------------------------------------------------------------------------------
WHOLE_CFG = dict(pre_nms_topN=40, score_thresh=0.3)


def _whole_pair(C, per_head):
    from smallhardface_amd import caffe
    msg = P.parse(M.whole_net_txt(C, per_head))
    params = M.whole_params(msg)
    onet = O.OracleNet(msg, params=params, proposal_cfg=O.ProposalParams(**WHOLE_CFG))
    gnet = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(gnet, params)
    return gnet, onet


@pytest.fixture(scope="module")
def whole_oracle():
    """The oracle's forward of the four graphs, computed once."""
    out = {}
    data, info = M.whole_input()
    for C in (3, 4):
        for per_head in (True, False):
            msg = P.parse(M.whole_net_txt(C, per_head))
            onet = O.OracleNet(msg, params=M.whole_params(msg), proposal_cfg=O.ProposalParams(**WHOLE_CFG))
            oo = onet.forward(data=data, im_info=info)
            out[(C, per_head)] = (onet, {k: np.array(v) for k, v in oo.items()})
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("per_head", [True, False], ids=["per_head", "single_blob"])
@pytest.mark.parametrize("C", [3, 4])
def test_whole_forward_against_the_oracle_net(whole_oracle, C, per_head, mode):
    from smallhardface_amd import caffe
    onet, oo = whole_oracle[(C, per_head)]
    data, info = M.whole_input()
    ob, os_ = oo["boxes"], oo["cls_prob"]
    # the oracle alone: 40 rows, every foreground class is the best class of some row
    assert os_.shape == (40, C) and (np.bincount(os_[:, 1:].argmax(axis=1), minlength=C - 1) > 0).all()
    gnet = caffe.Net(None, prototxt_text=P.dumps(onet.msg))
    H.load_params(gnet, onet.params)
    cfg.TEST.N_DETS_PER_MODULE = WHOLE_CFG["pre_nms_topN"]
    cfg.TEST.SCORE_THRESH = WHOLE_CFG["score_thresh"]
    gnet.set_conv_mode(mode)
    go = _forward(gnet, data, info)
    gb, gs = go["boxes"], go["cls_prob"]
    assert gnet.num_classes == C and gs.shape == os_.shape and gb.shape == ob.shape
    # every blob of the graph is readable, has the oracle's shape and its values
    assert list(gnet.blobs.keys()) == list(onet.blobs.keys())
    for name in gnet.blobs.keys():
        if name in ("boxes", "cls_prob", "data", "im_info"):
            continue
        a, b = _blob(gnet, name), onet.blobs[name].data
        assert a.shape == b.shape, name
        assert np.abs(a - b).max() < SCORE_TOL * max(1.0, float(np.abs(b).max())), name
    gp, gd = _blob(gnet, "cls_prob_reshape_output"), _blob(gnet, "bbox_pred_output")
    assert gp.shape == (1, 3 * C, 9, 13) and np.abs(gp - onet.blobs["cls_prob_reshape_output"].data).max() < SCORE_TOL
    # stage parity on identical inputs: the oracle's proposal layer on the probabilities and deltas the GPU produced
    pb, ps = O.proposal_forward(gp, gd, info, O.ProposalParams(**WHOLE_CFG))
    assert gb.shape == pb.shape and gs.shape == ps.shape            # equal row count
    np.testing.assert_array_equal(gs, ps)
    assert np.abs(gb - pb).max() < BOX_TOL
    # end to end against the oracle net: rows matched by box.  The candidates lie close together around the 40th (the 41st
    # best score is within SCORE_TOL of it), so a row may change sides of the pre_nms_topN cut: the rows are matched against
    # the oracle's proposal layer on the oracle net's own blobs WITHOUT the cut, whose first 40 rows are the net's output, and
    # a matched row beyond them must score within 2 SCORE_TOL of the 40th (its score and the cut both moved by at most one)
    ub, us = O.proposal_forward(onet.blobs["cls_prob_reshape_output"].data, onet.blobs["bbox_pred_output"].data, info,
                                O.ProposalParams(pre_nms_topN=0, score_thresh=WHOLE_CFG["score_thresh"]))
    np.testing.assert_array_equal(us[:40], os_)
    np.testing.assert_array_equal(ub[:40], ob)
    matched = set()
    for r in range(len(gb)):
        d = np.abs(ub[:, 1:] - gb[r, 1:]).max(axis=1)
        j = int(d.argmin())
        assert d[j] < 0.05, (r, float(d[j]))
        assert np.abs(gs[r] - us[j]).max() < SCORE_TOL, (r, j)
        assert j < 40 or us[j, 1:].max() >= us[39, 1:].max() - 2 * SCORE_TOL, (r, j)
        matched.add(j)
    assert len(matched) == len(gb)


# ---- 5. grouped forwards -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("per_head", [True, False], ids=["per_head", "single_blob"])
def test_forward_group_of_a_three_class_net_equals_the_single_forwards(per_head, mode):
    root, _ = _whole_pair(3, per_head)
    cfg.TEST.N_DETS_PER_MODULE = WHOLE_CFG["pre_nms_topN"]
    cfg.TEST.SCORE_THRESH = WHOLE_CFG["score_thresh"]
    sizes = [(9, 13), (7, 9), (12, 10)]
    inputs = [dict(zip(("data", "im_info"), M.whole_input(h, w))) for h, w in sizes]
    names = ["boxes", "cls_prob", "cls_prob_reshape_output", "bbox_pred_output", "cls_score_reshape_output"]
    root.set_conv_mode(mode)
    single = []
    for inp in inputs:
        _forward(root, inp["data"], inp["im_info"])
        single.append({n: _blob(root, n) for n in names})
    assert all(s["cls_prob"].shape[1] == 3 and len(s["cls_prob"]) > 1 for s in single)
    members = [root, root.clone(), root.clone()]
    for m, inp in zip(members, inputs):
        m.blobs["data"].reshape(*inp["data"].shape)
        m.blobs["im_info"].reshape(1, 3)
    outs = root.forward_group(members, inputs)
    for m, out, want in zip(members, outs, single):
        for key in ("boxes", "cls_prob"):
            np.testing.assert_array_equal(out[key], want[key])
        for n in names:
            np.testing.assert_array_equal(_blob(m, n), want[n], err_msg=n)


# ---- 6. the driver's class loop -----------------------------------------------------------------------------------------------------
class _Canned(object):
    """What forward_net reads of a forwarded net: the proposal layer's two tops."""

    def __init__(self, boxes, probs):
        self.blobs = {"boxes": O.OBlob(boxes.shape), "cls_prob": O.OBlob(probs.shape)}
        self.blobs["boxes"].data[...] = boxes
        self.blobs["cls_prob"].data[...] = probs


@pytest.mark.parametrize("method", ["BBOX_VOTE", "NMS"])
def test_class_loop_reproduces_the_reference_detect_with_three_classes(golden, method):
    from smallhardface_amd import test as T
    g = golden("proposal_multiclass.npz")
    all_probs, all_boxes = [], []
    for u in (0, 1):
        net = _Canned(g["detect_u%d_boxes" % u], g["detect_u%d_probs" % u])
        info = g["detect_u%d_im_info" % u]
        out = {"boxes": net.blobs["boxes"].data, "cls_prob": net.blobs["cls_prob"].data}
        probs, boxes = T._unit_results(net, out, int(g["detect_u%d_width" % u][0]), float(info[0, 2]), bool(g["detect_u%d_flip" % u][0]))
        assert boxes[0].shape == (len(probs[0]), 12)          # tiled per class
        all_probs.append(probs[0].copy())
        all_boxes.append(boxes[0][:, 0:4])
    cfg.TEST.NMS_METHOD = method
    cfg.TEST.NMS_THRESH = float(g["detect_nms_thresh"][0])
    cls_dets = T._merge_class_dets(np.concatenate(all_probs), np.concatenate(all_boxes), float(g["detect_thresh"][0]))
    assert len(cls_dets) == 2
    for c in range(2):
        want = g["detect_%s_dets%d" % (method, c)]
        got = np.asarray(cls_dets[c], dtype=np.float64)
        assert got.shape == want.shape, (method, c)
        np.testing.assert_array_equal(got, want)              # as tests/test_gpu_golden.py holds the two-class detect.npz


# ---- 7. the fused per-image path refuses more than two classes -------------------------------------------------------------------------
def test_fused_path_refuses_a_three_class_net_and_leaves_others_alone():
    import torch
    from smallhardface_amd import _lib
    two = _one_hot_net(128, 7, 9, 2, 3, False)
    three = _one_hot_net(128, 7, 9, 3, 3, False)
    rng = np.random.default_rng(5)
    for net in (two, three):
        for name in [n for n in net.params if n.startswith(("cls_score", "bbox_pred"))]:
            wb, bb = net.params[name]
            wb.data[...] = rng.normal(0, 1.0 / np.sqrt(128), wb.shape).astype(np.float32)
            bb.data[...] = 0
    x = rng.normal(0, 1, (1, 128, 7, 9)).astype(np.float32)
    unit = (x, 7, 9, 53, 67, 1.0, False)
    buf = torch.zeros((1024, 5), dtype=torch.float32, device="cuda")

    def two_class_pass():
        two.detect_begin()
        two.detect_add_levels([two], [unit], 0.05)
        n = two.detect_export(buf.data_ptr(), buf.shape[0])
        return buf[:n].cpu().numpy()

    before = two_class_pass()
    assert len(before) > 3
    with pytest.raises(_lib.ShfError, match=r"detect_add_levels: the net has 3 classes"):
        three.detect_add_levels([three], [unit], 0.05)
    with pytest.raises(_lib.ShfError, match=r"detect_add_level: the net has 3 classes"):
        three.detect_add_level(*unit, 0.05)
    with pytest.raises(_lib.ShfError, match=r"debug_append: the net has 3 classes"):
        three.debug_append(np.zeros((1, 5), np.float32), np.zeros((1, 2), np.float32), 67, 1.0, False, 0.05)
    np.testing.assert_array_equal(two_class_pass(), before)
    # the refused net still forwards
    out = _forward(three, x, np.array([[53, 67, 1.0]], np.float32))
    assert out["cls_prob"].shape[1] == 3 and len(out["cls_prob"]) > 3
