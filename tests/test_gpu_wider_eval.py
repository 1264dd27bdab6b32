"""The device path of the WIDER evaluator (shf_wider_eval_counts, csrc/eval.hip) against the unchanged host functions.

The device returns integers (per-detection hits / proposal flags, summed counts per threshold), so every comparison is
``assert_array_equal`` against ``image_counts`` / ``image_pr_info``; the curves of ``evaluate(device=True)`` are held to the
reference's own output in tests/golden/wider_eval.npz like tests/test_wider_eval.py holds the host path.  Sizes cross the
64-detection tile of the match kernel and the 64-lane scan of the counts kernel; ground-truth counts cross 64 and 128."""
import ctypes as C
import logging

import numpy as np
import pytest

from smallhardface_amd import _lib
from smallhardface_amd import wider_eval as W
from tests import wider_eval_cases as K

pytestmark = pytest.mark.gpu

TH = W.sweep_thresholds()


def check(preds, boxes, keeps, iou=0.5, bug=True):
    """device == host on one batch: per-detection hits and proposal flags, and the summed counts per threshold"""
    flat = W.flatten_inputs(preds, boxes, keeps)
    totals, hits, prop = W.device_counts(flat, iou, bug, TH, diagnostics=True)
    want_t, want_h, want_p = K.host_counts(preds, boxes, keeps, iou, bug)
    np.testing.assert_array_equal(hits, want_h)
    np.testing.assert_array_equal(prop, want_p)
    np.testing.assert_array_equal(totals, want_t)
    np.testing.assert_array_equal(W.device_counts(flat, iou, bug, TH), want_t)     # (without the diagnostic outputs)
    return hits, prop, totals


def one(pred_rows, gt_rows, keeps, iou=0.5, bug=True):
    p = np.array(pred_rows, dtype=np.float64).reshape(-1, 5)
    return check([p], [np.array(gt_rows, dtype=np.float64).reshape(-1, 4)],
                 [[np.array(k, dtype=np.int64)] for k in keeps], iou, bug)


# ---- the reference's own output -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bug", [True, False])
def test_golden_fixture_through_the_device(bug):
    g, gts, preds = K.golden_case()
    ap, curves = W.evaluate(preds, gts, iou_thresh=0.5, mimic_eval_bug=bug, device=True)
    want_ap, want_pr = g["ap_bug%d" % int(bug)], g["pr_bug%d" % int(bug)]
    for s in range(3):
        np.testing.assert_array_equal(np.isnan(curves[s]), np.isnan(want_pr[s]))
        np.testing.assert_allclose(np.nan_to_num(curves[s]), np.nan_to_num(want_pr[s]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(ap, want_ap, rtol=0, atol=1e-14)
    ap_h, cur_h = W.evaluate(preds, gts, iou_thresh=0.5, mimic_eval_bug=bug)
    for a, b in zip(curves, cur_h):
        np.testing.assert_array_equal(a, b)            # bit for bit the host path
    assert ap == ap_h


# ---- per-image diagnostics across the lane / wave / tile boundaries -------------------------------------------------------
@pytest.mark.parametrize("iou", [0.5, 0.3])
@pytest.mark.parametrize("bug", [True, False])
@pytest.mark.parametrize("real", [False, True])
def test_hits_and_proposals_equal_image_counts(real, bug, iou):
    """ground-truth counts {1, 63, 64, 65, 129} x detection counts {1, 63, 64, 65, 257}, three settings (empty, partial,
    full subset)"""
    preds, boxes, keeps = K.boundary_batch(20 + int(real), real)
    _, prop, _ = check(preds, boxes, keeps, iou, bug)
    assert (~prop[0]).any() and (~prop[1]).any() and prop[2].all()     # hits outside the subset do occur


# ---- boundary arithmetic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bug", [True, False])
def test_iou_of_exactly_one_half_is_matched(bug):
    hits, prop, _ = one([[0, 0, 4, 9, 0.9]], [[0, 0, 9, 9]], [[0], []], 0.5, bug)     # 50 / 100
    np.testing.assert_array_equal(hits[:, 0], [1, 0])
    np.testing.assert_array_equal(prop[:, 0], [True, False])


@pytest.mark.parametrize("bug", [True, False])
def test_detection_identical_to_a_box(bug):
    hits, prop, _ = one([[3.25, 4.5, 10.75, 20.125, 0.5], [3.25, 4.5, 10.75, 20.125, 0.4]],
                        [[100, 100, 5, 5], [3.25, 4.5, 10.75, 20.125]], [[1], [0]], 0.5, bug)
    np.testing.assert_array_equal(hits, [[1, 1], [0, 0]])          # a box counts once
    np.testing.assert_array_equal(prop, [[True, True], [False, False]])


@pytest.mark.parametrize("bug", [True, False])
def test_identical_boxes_the_first_index_wins(bug):
    """two identical ground-truth boxes, one inside the subset: keep = [0] finds a face, keep = [1] turns the detection
    into a non-proposal, because the arg-max is box 0 either way"""
    hits, prop, _ = one([[10, 10, 20, 20, 0.7]], [[10, 10, 20, 20], [10, 10, 20, 20]], [[0], [1]], 0.5, bug)
    np.testing.assert_array_equal(hits[:, 0], [1, 0])
    np.testing.assert_array_equal(prop[:, 0], [True, False])


@pytest.mark.parametrize("bug", [True, False])
@pytest.mark.parametrize("iou", [0.5, 0.3])
def test_negative_sizes_and_zero_union(bug, iou):
    gt = [[0, 0, 9, 9], [0, 0, -1, 5], [20, 20, 9, 9]]             # box 1 has area 0
    pred = [[2, 2, -0.5, 5, 0.9],      # negative width: iw > 0, area_det < 0
            [5, 5, -3, -3, 0.8],       # negative width and height
            [0, 0, -1, 7, 0.7],        # area 0 on the area-0 box: union exactly 0
            [1, 1, 30, -0.25, 0.6],
            [20, 20, 9, 9, 0.5]]
    one(pred, gt, [[0, 1, 2], [2], []], iou, bug)


# ---- sweep ----------------------------------------------------------------------------------------------------------------
def test_scores_on_the_thresholds_and_ties():
    """scores taken from the threshold array itself pin the >= side; equal scores share a count"""
    sc = [TH[0], TH[10], TH[10], TH[10], TH[500], TH[998], TH[998], TH[999]]
    gt = [[10 * k, 0, 8, 8] for k in range(4)]
    pred = [[10 * (k % 4), 0, 8, 8, s] for k, s in enumerate(sc)]
    _, _, totals = one(pred, gt, [[0, 1, 2, 3], [1, 3], []])
    assert totals[0, 0, 0] == 1 and totals[0, 9, 0] == 1 and totals[0, 10, 0] == 4 and totals[0, 999, 0] == 8


def test_all_scores_below_the_lowest_threshold():
    _, _, totals = one([[0, 0, 8, 8, -0.25], [0, 0, 8, 8, -0.5]], [[0, 0, 8, 8]], [[0]])
    assert not totals.any()


def test_mixed_batch_with_empty_images():
    """an image without detections, one without ground truth and a missing prediction among ordinary ones: the totals are
    the host's summed image_pr_info"""
    rng = np.random.default_rng(5)
    imgs = [K.make_image(rng, g, n, True) for g, n in ((3, 70), (65, 5), (7, 129))]
    preds = [imgs[0][0], np.zeros((0, 5)), imgs[1][0], imgs[2][0], None, imgs[2][0][:9]]
    boxes = [imgs[0][1], imgs[1][1], imgs[1][1], np.zeros((0, 4)), imgs[0][1], imgs[2][1]]
    keeps = [[K.subsets(rng, len(b))[s] for b in boxes] for s in (1, 2, 0)]
    check(preds, boxes, keeps, 0.5, True)
    check(preds, boxes, keeps, 0.3, False)


def test_only_empty_images():
    check([None, np.zeros((0, 5))], [np.array([[0., 0., 5., 5.]]), np.zeros((0, 4))], [[np.arange(1), np.arange(0)]])


# ---- refusals: argument checks only -----------------------------------------------------------------------------------------
def raw_call(pred_off, gt_off, n_settings=1, iou=0.5, n_pred_rows=1, n_gt_rows=1):
    """the C entry point on dummy one-row arrays: a refused call reads no further than the offsets"""
    lib = _lib.load()
    pred5 = np.array([[0, 0, 8, 8, 0.5]] * n_pred_rows, dtype=np.float64)
    gt4 = np.array([[0, 0, 8, 8]] * n_gt_rows, dtype=np.float64)
    counted = np.ones((max(n_settings, 1), n_gt_rows), dtype=np.uint8)
    po, go = np.array(pred_off, dtype=np.int32), np.array(gt_off, dtype=np.int32)
    totals = np.full((max(n_settings, 1), len(TH), 2), -1, dtype=np.int64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = lib.shf_wider_eval_counts(pred5.ctypes.data_as(dp), po.ctypes.data_as(ip), gt4.ctypes.data_as(dp),
                                   go.ctypes.data_as(ip), counted.ctypes.data_as(C.POINTER(C.c_uint8)), len(po) - 1,
                                   n_settings, iou, 1, TH.ctypes.data_as(dp), len(TH),
                                   totals.ctypes.data_as(C.POINTER(C.c_longlong)), None, None)
    return rc, _lib.last_error(), totals


REFUSED = [
    ("negative offset", dict(pred_off=[0, -1], gt_off=[0, 1]), "negative offset in pred_off"),
    ("negative gt offset", dict(pred_off=[0, 1], gt_off=[-2, 1]), "negative offset in gt_off"),
    ("non-monotone", dict(pred_off=[0, 1, 0], gt_off=[0, 1, 1]), "non-monotone offsets in pred_off"),
    ("non-monotone gt", dict(pred_off=[0, 1, 1], gt_off=[0, 1, 0]), "non-monotone offsets in gt_off"),
    ("iou 0", dict(pred_off=[0, 1], gt_off=[0, 1], iou=0.0), "iou_thresh"),
    ("iou above 1", dict(pred_off=[0, 1], gt_off=[0, 1], iou=1.5), "iou_thresh"),
    ("iou nan", dict(pred_off=[0, 1], gt_off=[0, 1], iou=float("nan")), "iou_thresh"),
    ("no settings", dict(pred_off=[0, 1], gt_off=[0, 1], n_settings=0), "n_settings"),
    ("nine settings", dict(pred_off=[0, 1], gt_off=[0, 1], n_settings=9), "n_settings"),
    ("2^31 rows", dict(pred_off=[0, 2 ** 28], gt_off=[0, 1], n_settings=8), "2^31"),
    ("2^31 gt rows", dict(pred_off=[0, 1, 1], gt_off=[0, 4096, 2 ** 30], n_settings=2), "2^31"),
    ("gt cap", dict(pred_off=[0, 1], gt_off=[0, 65537]), "ground-truth boxes"),
]


@pytest.mark.parametrize("name,args,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_bad_arguments_are_refused_and_the_next_call_is_right(name, args, msg):
    rc, err, _ = raw_call(**args)
    assert rc != 0 and msg in err, (rc, err)
    rc, _, totals = raw_call([0, 1], [0, 1])        # score 0.5 on its box: a proposal and a face from threshold 0.5 down
    assert rc == 0
    want = np.repeat((TH <= 0.5).astype(np.int64)[None, :, None], 2, axis=2)
    np.testing.assert_array_equal(totals, want)


def test_the_cap_itself_is_accepted():
    """65 536 ground-truth boxes in one image (the stated cap) run; the detection sits on the LAST box"""
    g = 65536
    gt = np.zeros((g, 4))
    gt[:, 0] = 20.0 * np.arange(g)
    gt[:, 2:] = 8
    pred = np.array([[gt[-1, 0], 0, 8, 8, 0.75]])
    flat = W.flatten_inputs([pred], [gt], [[np.array([g - 1])], [np.array([0])]])
    totals, hits, prop = W.device_counts(flat, 0.5, True, TH, diagnostics=True)
    np.testing.assert_array_equal(hits[:, 0], [1, 0])
    np.testing.assert_array_equal(prop[:, 0], [True, False])
    assert totals[0, 249, 0] == 1 and totals[0, 248, 0] == 0 and totals[1].sum() == 0


# ---- fallback -------------------------------------------------------------------------------------------------------------
def test_nan_score_takes_the_host_path(caplog):
    _, gts, preds = K.golden_case()
    preds = [np.array(p, dtype=np.float64) for p in preds]
    preds[next(j for j, p in enumerate(preds) if len(p) > 1)][1, 4] = np.nan
    with np.errstate(invalid="ignore"), caplog.at_level(logging.WARNING):
        ap_d, cur_d = W.evaluate(preds, gts, device=True)
        ap_h, cur_h = W.evaluate(preds, gts)
    assert any("host" in r.getMessage() for r in caplog.records)
    for a, b in zip(cur_d, cur_h):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ap_d, ap_h)
