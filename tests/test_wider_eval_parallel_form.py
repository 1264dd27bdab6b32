"""The parallel form of the WIDER evaluator (match -> per-setting counts -> threshold sweep) restated in numpy
(tests/wider_eval_cases.py: parallel_counts, the specification of csrc/eval.hip) equals the sequential host functions
``image_counts`` / ``image_pr_info``; the flattening helper round-trips; and ``evaluate(device=True)`` with the device call
replaced by that restatement gives the host's curves bit for bit.  No GPU."""
import logging

import numpy as np
import pytest

from smallhardface_amd import _lib
from smallhardface_amd import wider_eval as W
from tests import wider_eval_cases as K


def _check(preds, boxes, keeps, iou, bug):
    flat = W.flatten_inputs(preds, boxes, keeps)
    totals, hits, prop = K.parallel_counts(flat, iou, bug, W.sweep_thresholds())
    want_t, want_h, want_p = K.host_counts(preds, boxes, keeps, iou, bug)
    np.testing.assert_array_equal(hits, want_h)
    np.testing.assert_array_equal(prop, want_p)
    np.testing.assert_array_equal(totals, want_t)
    return want_p


@pytest.mark.parametrize("g", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("real", [False, True])
def test_parallel_form_equals_image_counts(g, real):
    rng = np.random.default_rng(1000 * g + int(real))
    off_subset = 0
    for n in (1, 5, 64, 65, 300):
        p, b = K.make_image(rng, g, n, real)
        keeps = [[k] for k in K.subsets(rng, g)]
        for bug in (True, False):
            for iou in (0.5, 0.3):
                want_p = _check([p], [b], keeps, iou, bug)
                off_subset += int((~want_p).sum())
    assert off_subset > 0      # the grid does contain hits on faces outside the subset


def test_batches_with_empty_images_and_shared_totals():
    preds, boxes, keeps = K.boundary_batch(7, real=True)
    # an image without detections, one without ground truth, a missing prediction
    preds += [np.zeros((0, 5)), K.make_image(np.random.default_rng(3), 4, 9, True)[0], None]
    boxes += [np.array([[1., 2., 30., 40.]]), np.zeros((0, 4)), np.array([[5., 5., 9., 9.]])]
    for s in range(3):
        keeps[s] += [np.arange(1), np.zeros(0, dtype=np.int64), np.arange(1)]
    _check(preds, boxes, keeps, 0.5, True)
    _check(preds, boxes, keeps, 0.3, False)


def test_flatten_round_trips():
    preds, boxes, keeps = K.boundary_batch(11, real=False)
    preds += [None, np.zeros((0, 5))]
    boxes += [np.array([[1., 2., 3., 4.]]), np.zeros((0, 4))]
    for s in range(3):
        keeps[s] += [np.arange(1), np.zeros(0, dtype=np.int64)]
    flat = W.flatten_inputs(preds, boxes, keeps)
    assert flat["pred5"].dtype == np.float64 and flat["gt4"].dtype == np.float64 and flat["counted"].dtype == np.uint8
    assert flat["pred_off"].dtype == np.int32 and flat["pred_off"][0] == 0 and flat["pred_off"][-1] == flat["pred5"].shape[0]
    assert flat["gt_off"][-1] == flat["gt4"].shape[0] == flat["counted"].shape[1] and flat["counted"].shape[0] == 3
    for got, want in zip(W.split_flat(flat["pred5"], flat["pred_off"]), preds):
        np.testing.assert_array_equal(got, np.zeros((0, 5)) if want is None else want)
    for got, want in zip(W.split_flat(flat["gt4"], flat["gt_off"]), boxes):
        np.testing.assert_array_equal(got, want)
    for s in range(3):
        for got, want, b in zip(W.split_flat(flat["counted"][s], flat["gt_off"]), keeps[s], boxes):
            np.testing.assert_array_equal(np.flatnonzero(got), np.sort(want) if len(b) else [])


def _model_device_counts(calls):
    def fake(flat, iou_thresh=0.5, mimic_eval_bug=True, thresh=None, diagnostics=False):
        calls.append(flat["counted"].shape[0])
        return K.parallel_counts(flat, iou_thresh, mimic_eval_bug, thresh)[0]
    return fake


@pytest.mark.parametrize("bug", [True, False])
def test_device_glue_gives_the_host_curves_bit_for_bit(monkeypatch, bug):
    """flatten -> counts -> divisions of the device path, with the counts from the numpy restatement: the curves and APs are
    the host path's to the last bit, in one call for the three settings."""
    _, gts, preds = K.golden_case()
    calls = []
    monkeypatch.setattr(W, "device_counts", _model_device_counts(calls))
    ap_d, cur_d = W.evaluate(preds, gts, 0.5, bug, device=True)
    ap_h, cur_h = W.evaluate(preds, gts, 0.5, bug)
    assert calls == [3]
    for a, b in zip(cur_d, cur_h):
        np.testing.assert_array_equal(a, b)            # (NaN == NaN under assert_array_equal)
    assert ap_d == ap_h


def test_settings_that_do_not_share_boxes_get_one_call_each(monkeypatch):
    _, gts, preds = K.golden_case()
    moved = [np.array(b, dtype=np.float64) for b in gts[1].boxes]
    moved[0] = moved[0] + 1.0
    gts = [gts[0], W.WiderGT(gts[1].events, gts[1].names, moved, gts[1].keep), gts[2]]
    calls = []
    monkeypatch.setattr(W, "device_counts", _model_device_counts(calls))
    _, cur_d = W.evaluate(preds, gts, 0.5, True, device=True)
    _, cur_h = W.evaluate(preds, gts, 0.5, True)
    assert calls == [1, 1, 1]
    for a, b in zip(cur_d, cur_h):
        np.testing.assert_array_equal(a, b)


def test_non_finite_input_takes_the_host_path_with_a_warning(monkeypatch, caplog):
    _, gts, preds = K.golden_case()
    preds = [np.array(p, dtype=np.float64) for p in preds]
    preds[next(j for j, p in enumerate(preds) if len(p))][0, 0] = np.inf

    def never(*a, **k):
        raise AssertionError("the device path must not be taken")
    monkeypatch.setattr(W, "device_counts", never)
    with np.errstate(invalid="ignore"), caplog.at_level(logging.WARNING):
        _, cur_d = W.evaluate(preds, gts, 0.5, True, device=True)
        _, cur_h = W.evaluate(preds, gts, 0.5, True)
    assert any("host" in r.getMessage() for r in caplog.records)
    for a, b in zip(cur_d, cur_h):
        np.testing.assert_array_equal(a, b)


def test_device_true_without_a_gpu_raises(monkeypatch):
    lib = _lib.load(require_gpu=False)
    monkeypatch.setattr(lib, "shf_device_count", lambda: 0)
    _, gts, preds = K.golden_case()
    with pytest.raises(_lib.ShfError):
        W.evaluate(preds, gts, device=True)


def test_default_stays_the_host_path(monkeypatch):
    def never(*a, **k):
        raise AssertionError("device_counts called without device=True")
    monkeypatch.setattr(W, "device_counts", never)
    _, gts, preds = K.golden_case()
    W.evaluate(preds, gts)
