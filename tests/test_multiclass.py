"""More than two classes through the proposal layer, the parts that need no GPU.

tests/golden/proposal_multiclass.npz holds what the reference's own ProposalLayer.forward and detect() produced with three
and four classes (tests/golden/make_multiclass_golden.py); the oracle is held to it here, the HIP tail in
tests/test_gpu_multiclass_tail.py."""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import multiclass_cases as M


def test_fixture_is_what_it_claims(golden):
    g = golden("proposal_multiclass.npz")
    assert sorted(g["cases"]) == sorted(M.CASES)
    seen = set()
    for case in M.CASES:
        sc, dl, ii, pp, _, gb, gp = M.fixture_case(g, case)
        C, A = (int(v) for v in g[case + "_classes"])
        seen.add((C, A))
        assert sc.shape == (1, C * A, 7, 9) and dl.shape == (1, 4 * A, 7, 9) and gp.shape[1] == C
        assert O.generate_anchors(pp.base_size, pp.ratios, pp.scales, pp.shifts, pp.feat_stride).shape == (A, 4)
    assert {(3, 3), (3, 8), (4, 8), (4, 3)} <= seen
    p = g["tie_classes_probs"]          # the same best foreground score in class 1 of one anchor and class 2 of another
    assert p[0, 1:].max() == p[1, 1:].max() == 0.75 and {int(p[0, 1:].argmax()), int(p[1, 1:].argmax())} == {0, 1}
    p = g["class2_wins_probs"]
    assert ((p[:, 1] < 0.3) & (p[:, 2] >= 0.3)).any() and (p[:, 1:].max(axis=1) >= 0.3).all()
    assert len(g["topn_cut_probs"]) == 40
    assert g["none_at_thresh_probs"].shape == (1, 4) and g["none_at_thresh_probs"][0, 1:].max() < 0.6
    assert g["none_valid_probs"].shape == (0, 3) and g["none_valid_boxes"].tolist() == [[0, 0, 0, 16, 16]]
    for u in (0, 1):
        assert g["detect_u%d_probs" % u].shape[1] == 3 and int(g["detect_u%d_flip" % u][0]) == u


@pytest.mark.parametrize("case", M.CASES)
def test_oracle_proposal_forward_reproduces_the_reference_with_more_classes(golden, case):
    g = golden("proposal_multiclass.npz")
    sc, dl, ii, pp, _, gb, gp = M.fixture_case(g, case)
    ob, op = O.proposal_forward(sc, dl, ii, pp)
    assert ob.shape == gb.shape and op.shape == gp.shape and ob.dtype == gb.dtype and op.dtype == gp.dtype
    if case == "tie_classes":
        # argsort()[::-1] leaves the order of the two tied rows to numpy; the oracle's is canonical: the lower anchor index
        # (class 1 wins there) first.  Everything else row for row; the tied pair as a set.
        assert op[0].tolist() == [0.125, 0.75, 0.125] and op[1].tolist() == [0.125, 0.125, 0.75]
        np.testing.assert_array_equal(op[2:], gp[2:])
        np.testing.assert_array_equal(ob[2:], gb[2:])
        np.testing.assert_array_equal(M.rows_sorted(np.hstack([op[:2], ob[:2]])), M.rows_sorted(np.hstack([gp[:2], gb[:2]])))
    else:
        np.testing.assert_array_equal(op, gp)
        np.testing.assert_array_equal(ob, gb)


@pytest.mark.parametrize("per_head", [True, False], ids=["per_head", "single_blob"])
@pytest.mark.parametrize("C", [3, 4])
def test_whole_graph_oracle_has_every_class_winning_rows(C, per_head):
    """The whole-forward GPU test's inputs judged on the CPU: with `synth_params` seed 7, pre_nms_topN 40 and SCORE_THRESH
    0.3 the oracle returns 40 rows and every foreground class is the best class of some row (3 / 37 and 8 / 4 / 28 rows
    with the per-head tail, 19 / 21 and 16 / 17 / 7 with the single-blob one)."""
    msg = P.parse(M.whole_net_txt(C, per_head))
    onet = O.OracleNet(msg, params=M.whole_params(msg), proposal_cfg=O.ProposalParams(pre_nms_topN=40, score_thresh=0.3))
    data, info = M.whole_input()
    out = onet.forward(data=data, im_info=info)
    probs = out["cls_prob"]
    hits = np.bincount(probs[:, 1:].argmax(axis=1), minlength=C - 1)
    print("C %d %s: %d rows, hits per foreground class %s" % (C, "per-head" if per_head else "single-blob", len(probs), hits.tolist()))
    assert probs.shape == (40, C) and (hits > 0).all()
    assert onet.blobs["cls_prob_reshape_output"].data.shape == (1, 3 * C, 9, 13)


def test_image_list_takes_class_names():
    from smallhardface_amd.datasets import ImageList
    assert ImageList("wider_val", ["a.jpg"]).num_classes == 2
    db = ImageList("wider_val", ["a.jpg"], classes=["bg", "face", "masked_face"])
    assert db.num_classes == 3 and len(db) == 1
    with pytest.raises(ValueError, match="at least one foreground class"):
        ImageList("wider_val", ["a.jpg"], classes=["bg"])


def test_num_classes_entry_point_is_declared_and_exported():
    from smallhardface_amd import _lib
    assert "shf_net_num_classes" in _lib.declared_symbols()
    lib = _lib.load(require_gpu=False)
    assert hasattr(lib, "shf_net_num_classes")
    assert lib.shf_net_num_classes.argtypes is not None and len(lib.shf_net_num_classes.argtypes) == 1


class _FakeNet(object):
    num_classes = 3

    def __init__(self, *a, **kw):
        pass

    def set_conv_mode(self, mode):
        pass


def test_inference_worker_checks_the_class_count_and_takes_the_class_loop(monkeypatch):
    """No GPU: the net and detect() are stand-ins.  A three-class net over a two-class imdb is refused naming both numbers;
    over a three-class imdb the worker takes the per-unit detect() loop (the fused per-image path serves two classes) and
    files every foreground class's detections."""
    from smallhardface_amd import test as T
    from smallhardface_amd.config import cfg
    from smallhardface_amd.datasets import ImageList
    monkeypatch.setattr(T.caffe, "Net", _FakeNet)
    monkeypatch.setattr(T.caffe, "set_mode_gpu", lambda: None)
    monkeypatch.setattr(T.caffe, "set_device", lambda i: None)
    monkeypatch.delenv("SHF_FUSED_DETECT", raising=False)
    cfg.TEST.MODEL = "some.caffemodel"
    cfg.TEST.GPU_ID = [0]
    assert len(cfg.TEST.SCALES) > 1 and len(cfg.TEST.LEVEL) == 0          # a two-class net would take the fused loop here
    with pytest.raises(ValueError, match=r"3 classes, the imdb 'wider_val' has 2"):
        T.inference_worker(0, ImageList("wider_val", ["a.jpg"]), "t.prototxt", 0, 1, 0.05)

    def no_fused(*a, **kw):
        raise AssertionError("the fused per-image loop was taken for a three-class net")

    c1, c2 = np.ones((2, 5)), np.zeros((1, 5))
    monkeypatch.setattr(T, "fused_image_loop", no_fused)
    monkeypatch.setattr(T, "detect", lambda net, path, thresh, timers=None, pyramid=False: ([c1, c2], timers))
    dets = T.inference_worker(0, ImageList("wider_val", ["a.jpg", "b.jpg"], classes=["bg", "face", "head"]), "t.prototxt", 0, 2, 0.05)
    assert len(dets) == 3 and dets[0] == [[], []] and dets[1] == [c1, c1] and dets[2] == [c2, c2]
