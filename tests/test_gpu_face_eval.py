"""The device path of the AFW / Pascal Faces evaluator (shf_face_eval_match, csrc/eval.hip) against the unchanged host
functions.

The device returns integers (per detection a code and the chosen box), so every comparison of a round is
``assert_array_equal`` against ``match_host``; ``evaluate(device=True)`` is held to the reference's own output in
tests/golden/face_eval.npz like tests/test_face_eval.py holds the host path, and to the host path bit for bit.  Box counts
cross the 64 lanes of the wave that walks an image (0, 1, 63, 64, 65, 130), detection counts run 0, 1, 64, 200, and one
call holds 1 image or 70."""
import ctypes as C
import logging

import numpy as np
import pytest

from smallhardface_amd import _lib
from smallhardface_amd import face_eval as F
from tests import face_eval_cases as K

pytestmark = pytest.mark.gpu


def check(dets, gt, ovr):
    """device == host on one round: codes and chosen indices"""
    _, want_code, want_index = K.one_round(dets, gt, ovr, F.match_host)
    _, code, index = K.one_round(dets, gt, ovr, F.match_device)
    np.testing.assert_array_equal(code, want_code)
    np.testing.assert_array_equal(index, want_index)
    return code, index


# ---- the reference's own output -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nit,ovr", K.COMBOS)
@pytest.mark.parametrize("ds", K.DATASETS)
def test_golden_fixture_through_the_device(ds, nit, ovr):
    g, dets, gt, _ = K.golden_case(ds)
    kept = F.filter_detections(dets, F.min_pixels(30, 30))
    ap, rec, prec, info = F.evaluate(kept, gt, ovr=ovr, iters=nit, device=True)
    K.assert_equals_fixture(g, K.tag(ds, nit, ovr), ap, rec, prec, info)
    ap_h, rec_h, prec_h, info_h = F.evaluate(kept, gt, ovr=ovr, iters=nit)
    # bit for bit the host path (NaN positions included)
    np.testing.assert_array_equal(rec, rec_h)
    np.testing.assert_array_equal(prec, prec_h)
    np.testing.assert_array_equal(info["boxes"], info_h["boxes"])
    assert ap == ap_h and np.array_equal(info["ap11"], info_h["ap11"], equal_nan=True)
    for a, b in zip(info["rounds"], info_h["rounds"]):
        np.testing.assert_array_equal(a["tp"], b["tp"])
        np.testing.assert_array_equal(a["fp"], b["fp"])
        np.testing.assert_array_equal(a["index"], b["index"])
        np.testing.assert_array_equal(np.array(a["means"]), np.array(b["means"]))


# ---- one round across the lane / wave boundaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("ovr", [0.5, 0.3])
@pytest.mark.parametrize("kw", [{}, {"equal_scores": True}, {"equal_ious": True}, {"all_difficult": True}],
                         ids=["plain", "equal_scores", "equal_ious", "all_difficult"])
def test_codes_and_indices_equal_the_host(kw, ovr):
    """box counts {0, 1, 63, 64, 65, 130} x detection counts {0, 1, 64, 200}: 24 images in one call"""
    dets, gt = K.batch(41, K.boundary_shapes(), **kw)
    code, index = check(dets, gt, ovr)
    if kw.get("all_difficult"):
        assert not (code == F.TRUE_POSITIVE).any() and (code == F.NEITHER).any()
    else:
        assert all((code == c).any() for c in (F.NEITHER, F.TRUE_POSITIVE, F.FALSE_POSITIVE))
    assert index.max() > 64 and (index == -1).any()          # boxes of the third lane round are chosen


@pytest.mark.parametrize("shape", [(0, 1), (1, 0), (1, 1), (65, 200), (130, 64)], ids=str)
def test_one_image_in_one_call(shape):
    dets, gt = K.batch(43, [shape])
    check(dets, gt, 0.5)


def test_seventy_images_in_one_call():
    dets, gt = K.batch(47, K.many_images_shapes(70))
    check(dets, gt, 0.5)
    check(dets, gt, 0.3)


def test_equal_maxima_take_the_last_box_across_lanes():
    """130 copies of one box, one exact detection: the walk ends on box 129 whichever lane holds it; with the last copy
    difficult the detection is neither, with any other copy difficult it counts"""
    box = [10., 10., 50., 50.]
    dets = F.Detections(["a", "a"], [[0.9] + box, [0.8] + box])
    for hard, want in ((129, [F.NEITHER, F.NEITHER]), (64, [F.TRUE_POSITIVE, F.FALSE_POSITIVE])):
        diff = np.zeros(130, bool)
        diff[hard] = True
        code, index = check(dets, F.FaceGT(["a.jpg"], [[box] * 130], [diff]), 0.5)
        assert code.tolist() == want and index.tolist() == [129, 129]


def test_iou_exactly_equal_to_ovr_is_a_false_positive():
    dets = F.Detections(["a"], [[0.9, 0, 0, 9, 4]])              # 50 of the 100 pixels of (0, 0, 9, 9)
    gt = F.FaceGT(["a.jpg"], [[[0, 0, 9, 9]]], [[False]])
    assert check(dets, gt, 0.5)[0].tolist() == [F.FALSE_POSITIVE]
    assert check(dets, gt, 0.4999)[0].tolist() == [F.TRUE_POSITIVE]


def test_inverted_and_degenerate_boxes():
    """abs() extents, negative intersections and zero-size boxes go through the same arithmetic"""
    dets = F.Detections(["a"] * 5, [[0.9, 30, 5, 2, 40], [0.8, 5, 5, 5, 5], [0.7, 0, 0, 60, 60], [0.6, 50, 50, 10, 10],
                                    [0.5, 10, 10, 50, 50]])
    gt = F.FaceGT(["a.jpg"], [[[0, 0, 60, 60], [5, 5, 5, 5], [50, 50, 10, 10], [10, 10, 50, 50]]], [[False] * 4])
    check(dets, gt, 0.5)
    check(dets, gt, 0.3)


# ---- refusals: argument checks only -----------------------------------------------------------------------------------------
def raw_call(det_off, gt_off, ovr=0.5):
    """the C entry point on dummy one-row arrays: a refused call reads no further than the offsets"""
    lib = _lib.load()
    det4 = np.array([[10., 10., 50., 50.]])
    gt4 = np.array([[10., 10., 50., 50.]])
    diff = np.zeros(1, dtype=np.uint8)
    do, go = np.array(det_off, dtype=np.int64), np.array(gt_off, dtype=np.int64)
    code, index = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int)
    rc = lib.shf_face_eval_match(det4.ctypes.data_as(dp), do.ctypes.data_as(lp), gt4.ctypes.data_as(dp),
                                 go.ctypes.data_as(lp), diff.ctypes.data_as(C.POINTER(C.c_uint8)), len(do) - 1, ovr,
                                 code.ctypes.data_as(ip), index.ctypes.data_as(ip))
    return rc, _lib.last_error(), code, index


REFUSED = [
    ("negative offset", dict(det_off=[0, -1], gt_off=[0, 1]), "negative offset in det_off"),
    ("negative gt offset", dict(det_off=[0, 1], gt_off=[-2, 1]), "negative offset in gt_off"),
    ("non-monotone", dict(det_off=[0, 1, 0], gt_off=[0, 1, 1]), "non-monotone offsets in det_off"),
    ("non-monotone gt", dict(det_off=[0, 1, 1], gt_off=[0, 1, 0]), "non-monotone offsets in gt_off"),
    ("ovr 0", dict(det_off=[0, 1], gt_off=[0, 1], ovr=0.0), "ovr must be in (0, 1]"),
    ("ovr above 1", dict(det_off=[0, 1], gt_off=[0, 1], ovr=1.5), "ovr must be in (0, 1]"),
    ("ovr nan", dict(det_off=[0, 1], gt_off=[0, 1], ovr=float("nan")), "ovr must be in (0, 1]"),
    ("2^31 rows", dict(det_off=[0, 2 ** 31], gt_off=[0, 1]), "2^31 rows or more"),
    ("2^31 gt rows", dict(det_off=[0, 1, 1], gt_off=[0, 4096, 2 ** 31]), "2^31 rows or more"),
]


@pytest.mark.parametrize("name,args,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_bad_arguments_are_refused_and_the_next_call_is_right(name, args, msg):
    rc, err, code, index = raw_call(**args)
    assert rc != 0 and msg in err, (rc, err)
    assert code.tolist() == [-7] and index.tolist() == [-7]           # nothing ran: the outputs are untouched
    rc, _, code, index = raw_call([0, 1], [0, 1])
    assert rc == 0 and code.tolist() == [F.TRUE_POSITIVE] and index.tolist() == [0]


def test_calls_without_work_return_at_once():
    rc, _, code, index = raw_call([0, 0], [0, 1])                    # no detections
    assert rc == 0 and code.tolist() == [-7]
    rc, _, code, index = raw_call([0, 1], [0, 0])                    # no ground truth at all: a false positive
    assert rc == 0 and code.tolist() == [F.FALSE_POSITIVE] and index.tolist() == [-1]


# ---- fallback -------------------------------------------------------------------------------------------------------------
def test_nan_boxes_take_the_host_path_with_a_warning(caplog):
    """a round without true positives leaves NaN boxes: from the second round on the matching runs on the host, and the
    result is the host path's"""
    dets = F.Detections(["a", "a"], [[0.9, 300, 300, 340, 340], [0.8, 400, 300, 440, 340]])
    gt = F.FaceGT(["a.jpg"], [[[10, 10, 50, 50]]], [[False]])
    with caplog.at_level(logging.WARNING):
        ap, rec, prec, info = F.evaluate(dets, gt, iters=3, device=True)
    assert sum("host" in r.getMessage() for r in caplog.records) == 2
    assert ap == 0.0 and np.isnan(info["boxes"]).all()
    ap_h, rec_h, prec_h, _ = F.evaluate(dets, gt, iters=3)
    np.testing.assert_array_equal(rec, rec_h)
    np.testing.assert_array_equal(prec, prec_h)


def test_a_nan_box_in_the_input_takes_the_host_path(caplog):
    _, dets, gt, _ = K.golden_case("afw")
    rows = dets.rows.copy()
    rows[5, 2] = np.nan
    bad = F.Detections(dets.names, rows)
    with caplog.at_level(logging.WARNING):
        ap, rec, prec, info = F.evaluate(bad, gt, iters=2, device=True)
    assert any("host" in r.getMessage() for r in caplog.records)
    ap_h, rec_h, prec_h, info_h = F.evaluate(bad, gt, iters=2)
    np.testing.assert_array_equal(prec, prec_h)
    np.testing.assert_array_equal(info["rounds"][-1]["tp"], info_h["rounds"][-1]["tp"])
    assert np.array_equal(ap, ap_h, equal_nan=True)
