"""Pin the numpy oracle's Python half against vectors produced by the
reference's own code (tests/golden/make_golden.py)."""
import ast

import numpy as np
import pytest

from oracle import oracle as O


def rows_sorted(a):
    a = np.asarray(a)
    if a.shape[0] == 0:
        return a
    return a[np.lexsort(a.T[::-1])]


def test_anchors(golden):
    g = golden("anchors.npz")
    np.testing.assert_array_equal(
        O.generate_anchors(16, [1], [1, 2, 4], [0], [8, 8, 8]), g["default_param_str"])
    np.testing.assert_array_equal(g["default_param_str"],
                                  [[0, 0, 15, 15], [-8, -8, 23, 23], [-24, -24, 39, 39]])
    np.testing.assert_array_equal(
        O.generate_anchors(16, (0.5, 1, 2), (8, 16, 32), [0], [16] * 3), g["frcnn_defaults"])
    np.testing.assert_array_equal(
        O.generate_anchors(8, [0.5, 2], [2, 3], [0], [8, 8]), g["two_ratios_base8"])


def test_bbox_transform(golden):
    g = golden("bbox_transform.npz")
    p = O.bbox_transform_inv(g["boxes"], g["deltas"])
    np.testing.assert_array_equal(p, g["pred"])
    assert p.dtype == np.float32
    np.testing.assert_array_equal(O.clip_boxes(p.copy(), g["im_shape"]), g["clipped"])
    np.testing.assert_array_equal(O.bbox_transform_inv(g["boxes"], g["deltas_overflow"]), g["pred_overflow"])
    np.testing.assert_array_equal(O.bbox_transform_inv(g["boxes"], g["deltas_big"]), g["pred_big"])


@pytest.mark.parametrize("case", ["small", "unpadded", "wide", "all_below", "over_10000", "c1_512",
                                  "overflow", "ties"])
def test_proposal(golden, case):
    g = golden("proposal.npz")
    boxes, probs = O.proposal_forward(g[case + "_scores"], g[case + "_deltas"], g[case + "_im_info"])
    gb, gp = g[case + "_boxes"], g[case + "_probs"]
    assert boxes.shape == gb.shape and probs.shape == gp.shape
    if case == "over_10000":
        assert gb.shape[0] == 10000
    if case == "all_below":
        assert gb.shape[0] == 1  # nothing >= SCORE_THRESH: the best one is kept
    # scores are produced in descending order by both
    np.testing.assert_array_equal(probs[:, 1], gp[:, 1])
    # rows compared as a set of (score, box) records: tie order is implementation-defined
    a = rows_sorted(np.hstack([probs, boxes]))
    b = rows_sorted(np.hstack([gp, gb]))
    np.testing.assert_array_equal(a, b)
    if len(np.unique(gp[:, 1])) == gp.shape[0]:  # no tied scores: order is defined
        np.testing.assert_array_equal(boxes, gb)


GEOMETRIES = ["two_ratios_mixed_strides", "shifts_two_strides", "three_ratios_dense", "strides_4_8_16"]
GEOMETRY_CASES = ([g + m for g in GEOMETRIES for m in ("_ms0", "_ms6")] +
                  ["two_ratios_mixed_strides" + t for t in ("_overflow", "_overflow_product", "_big_finite")])
# what the issue's table says each param string reaches: (A, anchor widths, anchor heights, sub-strides)
GEOMETRY_FACTS = {
    "two_ratios_mixed_strides": (4, [22, 33, 12, 18], [12, 18, 24, 36], [1, 2, 2, 2]),
    "shifts_two_strides": (8, [16] * 4 + [32] * 4, [16] * 4 + [32] * 4, [1, 1, 1, 1, 2, 2, 2, 2]),
    "three_ratios_dense": (6, [23, 46, 16, 32, 11, 22], [12, 24, 16, 32, 22, 44], None),
    "strides_4_8_16": (3, [8, 16, 32], [16, 32, 64], [1, 2, 4]),
}


def proposal_params(param_str, **kw):
    """The oracle's ProposalParams of a ProposalLayer param string (a Python / YAML dict literal)."""
    return O.ProposalParams(**dict(ast.literal_eval(str(param_str)), **kw))


def geometry_case(g, case):
    """(scores, deltas, im_info, ProposalParams, reference boxes, reference probs) of a proposal_geometry.npz case."""
    pp = proposal_params(g[case + "_param_str"], min_size=float(g[case + "_min_size"][0]))
    return g[case + "_scores"], g[case + "_deltas"], g[case + "_im_info"], pp, g[case + "_boxes"], g[case + "_probs"]


def test_proposal_geometry_fixture_is_what_it_claims(golden):
    g = golden("proposal_geometry.npz")
    assert sorted(g["cases"]) == sorted(GEOMETRY_CASES)
    for name in GEOMETRIES:
        pp = proposal_params(g[name + "_ms0_param_str"])
        A, aw, ah, sub = GEOMETRY_FACTS[name]
        a = O.generate_anchors(pp.base_size, pp.ratios, pp.scales, pp.shifts, pp.feat_stride)
        assert a.shape == (A, 4) and g[name + "_ms0_scores"].shape[1] == 2 * A
        np.testing.assert_array_equal(a[:, 2] - a[:, 0] + 1, aw)
        np.testing.assert_array_equal(a[:, 3] - a[:, 1] + 1, ah)
        assert max(aw + ah) <= 64
        assert pp.subsampled == (sub is not None)
        if sub:
            assert [pp.feat_stride[i // len(pp.shifts) ** 2] // pp.feat_stride[0] for i in range(A)] == sub
        if len(pp.shifts) > 1:   # shifted copies: offsets of shift * stride in x fastest, then y
            np.testing.assert_array_equal(a[:4] - a[0], [[0, 0, 0, 0], [4, 0, 4, 0], [0, 4, 0, 4], [4, 4, 4, 4]])
            np.testing.assert_array_equal(a[4:] - a[4], [[0, 0, 0, 0], [8, 0, 8, 0], [0, 8, 0, 8], [8, 8, 8, 8]])
        ii = g[name + "_ms0_im_info"]
        h, w = g[name + "_ms0_scores"].shape[2:]
        assert 0 < h * pp.feat_stride[0] - ii[0, 0] < 8 and 0 < w * pp.feat_stride[0] - ii[0, 1] < 8   # unpadded < padded
        assert ii[0, 2] == 1.5
        # the min-size cut removes some rows but not all, on the same inputs
        np.testing.assert_array_equal(g[name + "_ms0_scores"], g[name + "_ms6_scores"])
        np.testing.assert_array_equal(g[name + "_ms0_deltas"], g[name + "_ms6_deltas"])
        assert g[name + "_ms0_min_size"][0] == 0 and g[name + "_ms6_min_size"][0] == 6
        assert 0 < len(g[name + "_ms6_boxes"]) < len(g[name + "_ms0_boxes"])


@pytest.mark.parametrize("case", GEOMETRY_CASES)
def test_proposal_geometry(golden, case):
    """ProposalLayer.forward under param strings the templates never use, held the way `test_proposal` holds the template's:
    this is what entitles tests/test_gpu_tail_geometry.py to the oracle as truth for these geometries."""
    g = golden("proposal_geometry.npz")
    sc, dl, ii, pp, gb, gp = geometry_case(g, case)
    boxes, probs = O.proposal_forward(sc, dl, ii, pp)
    assert boxes.shape == gb.shape and probs.shape == gp.shape and len(gb) > 1
    np.testing.assert_array_equal(probs[:, 1], gp[:, 1])
    a = rows_sorted(np.hstack([probs, boxes]))
    b = rows_sorted(np.hstack([gp, gb]))
    np.testing.assert_array_equal(a, b)
    if len(np.unique(gp[:, 1])) == gp.shape[0]:
        np.testing.assert_array_equal(probs, gp)
        np.testing.assert_array_equal(boxes, gb)
    assert gb[:, [1, 3]].max() <= ii[0, 1] - 1 and gb[:, [2, 4]].max() <= ii[0, 0] - 1 and gb[:, 1:].min() >= 0
    if case.endswith("_ms6"):
        # no side of any candidate box within 0.01 px of the cut: the kept set cannot hinge on exp()'s last ulp
        allb, _ = O.proposal_forward(sc, dl, ii, proposal_params(g[case + "_param_str"], min_size=0, score_thresh=-1.0,
                                                                 pre_nms_topN=0))
        sides = np.concatenate([allb[:, 3] - allb[:, 1] + 1, allb[:, 4] - allb[:, 2] + 1])
        assert np.abs(sides - pp.min_size * ii[0, 2]).min() > 0.01
    # the clamp of every dw, dh > 50 to 5 happens exactly when something overflows fp32 (bbox_transform.py:52-65).  Under
    # the 6000 px high im_info of these cases a clamped dh of 60 ends exp(5) * 24 / 2 px below its centre, an unclamped one
    # at the image border -- as does the unclamped dh of 85.9 itself
    if "overflow" in case or "big_finite" in case:
        assert dl[0, 11, 4, 2] == 60.0 and ii[0, 0] == 6000
        assert int((gb[:, 4] == ii[0, 0] - 1).sum()) == (2 if case.endswith("big_finite") else 0)


def test_too_few_strides_raise_like_the_reference():
    """With 'subsampled' true the reference indexes feat_stride[i // len(shifts)**2] for every anchor
    (proposal_layer.py:160-165): fewer entries raise IndexError.  The runtime refuses such a graph at construction."""
    with pytest.raises(IndexError):
        O.proposal_forward(np.zeros((1, 8, 3, 3), np.float32), np.zeros((1, 16, 3, 3), np.float32),
                           np.array([[24, 24, 1]], np.float32),
                           O.ProposalParams(ratios=(0.5, 2), scales=(2, 3), feat_stride=(8, 8), base_size=8))


VOTE_SETS = ["empty", "single", "two_overlap", "singletons", "last_singleton", "clusters_small",
             "clusters_mid", "clusters_big", "ties", "dense", "iou_exact_0p4"]


@pytest.mark.parametrize("name", VOTE_SETS)
def test_bbox_vote(golden, name):
    g = golden("vote_nms.npz")
    # replay the reference's own (tie-order-undefined) permutation -> exact equality
    out = O.bbox_vote(g[name + "_dets"], order=g[name + "_order"])
    ref = g[name + "_vote"]
    assert out.shape == ref.shape
    np.testing.assert_array_equal(np.asarray(out, dtype=np.float64), ref)
    if name != "ties":  # without tied scores the canonical order is the same order
        np.testing.assert_array_equal(np.asarray(O.bbox_vote(g[name + "_dets"]), dtype=np.float64), ref)


@pytest.mark.parametrize("name", VOTE_SETS)
@pytest.mark.parametrize("thr", [0.4, 0.3, 0.7])
def test_nms(golden, name, thr):
    g = golden("vote_nms.npz")
    d = g[name + "_dets"]
    keep = O.nms(d, thr, order=g[name + "_order"])
    ref = g[name + "_nms_%02d" % int(thr * 100)]
    np.testing.assert_array_equal(keep, ref)
    if name != "ties":
        np.testing.assert_array_equal(O.nms(d, thr), ref)
    if name == "iou_exact_0p4" and thr == 0.4:
        # IoU == thr is NOT suppressed by the canonical '>' predicate ...
        assert len(keep) == 4
        # ... but is by the Cython '>=' variant (cpu_nms.pyx:65)
        assert len(O.nms_ge(d, thr)) == 2
