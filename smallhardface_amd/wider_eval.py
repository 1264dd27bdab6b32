"""WIDER FACE evaluation (easy / medium / hard AP) of written detections.

What the reference runs after ``test_net`` for the WIDER imdb (lib/datasets/wider.py:169-195 ->
lib/wider_eval_tools/wider_eval.py:10-222, itself a port of the official MATLAB toolbox).  Semantics kept exactly,
because they decide the published AP numbers:

  * predictions are read back from the per-image text files (x, y, w, h, score), ordered by falling score, and the
    scores are min-max normalised over the WHOLE prediction set (wider_eval.py:42-59);
  * boxes become (x1, y1, x1 + w, y1 + h); IoU uses the +1 pixel convention with a zero-union guard (:62-79);
  * ``mimic_eval_bug`` (cfg.MISC.MIMIC_EVAL_BUG, default on): every IoU is ROUNDED to 0 / 1 before the arg-max, so
    a detection is attributed to the FIRST ground-truth box with IoU >= 0.5, not the best one (:92-95);
  * a detection matched to a ground-truth box outside the setting's subset is neither a hit nor a false positive
    (``proposal_list = -1``), a box of the subset counts once (:96-103);
  * 1000 thresholds ``1 - (t + 1) / 1000`` on the normalised score (:106-120), dataset curve = summed counts
    (:123-130), AP = VOC-style area under the monotone precision envelope (:133-139).

The implementation is organised around in-memory structures (``WiderGT`` / lists of (n, 5) arrays) with separate
readers for the toolbox's ``.mat`` ground truth and the detection text files, and the per-image threshold sweep is a
``searchsorted`` instead of a 1000-step loop.

The default path is host numpy.  ``evaluate(..., device=True)`` / ``wider_eval(..., device=True)`` run the matching and
the threshold sweep -- the loop over every detection of every image, three times -- on the GPU instead
(``shf_wider_eval_counts``, csrc/eval.hip): sorting, score normalisation, the final divisions and ``voc_ap`` stay on the
host, the device returns exact integer counts, and the curves come out bit for bit the host's.
"""
import ctypes as C
import logging
import os

import numpy as np

THRESH_NUM = 1000
SETTINGS = ('easy_val', 'medium_val', 'hard_val')


class WiderGT(object):
    """Ground truth of one setting, flattened over events: per image its name, event, (n, 4) x-y-w-h boxes and the
    0-based indices of the boxes that count in this setting."""

    def __init__(self, events, names, boxes, keep):
        self.events, self.names, self.boxes, self.keep = list(events), list(names), list(boxes), list(keep)

    def __len__(self):
        return len(self.names)


def load_gt_mat(path):
    """``wider_{easy,medium,hard}_val.mat`` / ``wider_face_val.mat`` of the official toolbox -> WiderGT (image order =
    event-major, the order the reference flattens with np.vstack / reduce, wider_eval.py:150-154)."""
    from scipy import io as sio
    m = sio.loadmat(path)
    events, names, boxes, keep = [], [], [], []
    for e in range(m['event_list'].shape[0]):
        ev = str(m['event_list'][e][0][0])
        files = m['file_list'][e][0]
        bbx = m['face_bbx_list'][e][0]
        sub = m['gt_list'][e][0] if 'gt_list' in m else None
        for j in range(files.shape[0]):
            events.append(ev)
            names.append(str(files[j][0][0]))
            b = np.asarray(bbx[j][0], dtype=np.float64).reshape(-1, 4)
            boxes.append(b)
            if sub is None:
                keep.append(np.arange(b.shape[0]))
            else:
                keep.append(np.asarray(sub[j][0], dtype=np.int64).reshape(-1) - 1)  # MATLAB indices are 1-based
    return WiderGT(events, names, boxes, keep)


def read_predictions(pred_dir, gt):
    """Per image of ``gt``: the (n, 5) x-y-w-h-score rows of ``<pred_dir>/<event>/<name>.txt`` (the files
    datasets.write_detections_wider produces), ordered by falling score; None when the file is missing or broken
    (the reference logs and carries on, wider_eval.py:33-37)."""
    out = []
    for ev, name in zip(gt.events, gt.names):
        try:
            with open(os.path.join(pred_dir, ev, name + '.txt')) as f:
                lines = [l.strip() for l in f.readlines()]
            n = int(lines[1])
            rows = np.array([[float(v) for v in lines[2 + k].split()] for k in range(n)], dtype=np.float64).reshape(n, 5)
            out.append(sort_by_score(rows))
        except Exception:
            out.append(None)
    return out


def sort_by_score(rows):
    """Falling score; equal scores keep their file order (the reference's ``argsort()[::-1]`` leaves ties undefined)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    return rows[np.argsort(-rows[:, 4], kind='stable')]


def normalise_scores(preds):
    """Min-max over every prediction of the set (wider_eval.py:42-59).  Returns new arrays."""
    allp = [p[:, 4] for p in preds if p is not None and len(p)]
    lo = min(float(s.min()) for s in allp)
    hi = max(max(float(s.max()) for s in allp), 0.0)   # the reference starts its running maximum at 0
    out = []
    for p in preds:
        if p is None:
            out.append(None)
            continue
        q = np.array(p, dtype=np.float64)
        q[:, 4] = (q[:, 4] - lo) / (hi - lo)
        out.append(q)
    return out


def _overlaps(gt_xyxy, box):
    iw = np.minimum(gt_xyxy[:, 2], box[2]) - np.maximum(gt_xyxy[:, 0], box[0]) + 1
    ih = np.minimum(gt_xyxy[:, 3], box[3]) - np.maximum(gt_xyxy[:, 1], box[1]) + 1
    inter = iw * ih
    union = (gt_xyxy[:, 2] - gt_xyxy[:, 0] + 1) * (gt_xyxy[:, 3] - gt_xyxy[:, 1] + 1) + \
        (box[2] - box[0] + 1) * (box[3] - box[1] + 1) - inter
    union = np.where(union == 0, np.inf, union)
    o = inter / union
    o[(iw <= 0) | (ih <= 0)] = 0
    return o


def image_counts(pred, gt_boxes, keep, iou_thresh=0.5, mimic_eval_bug=True):
    """One image: (hits[h], is_proposal[h]) after each of the score-ordered detections -- the number of distinct
    subset faces found so far, and whether detection h counts as a proposal (False when it sits on a face outside
    the subset)."""
    n, g = pred.shape[0], gt_boxes.shape[0]
    counted = np.zeros(g, dtype=bool)
    counted[keep] = True
    gxy = np.array(gt_boxes, dtype=np.float64)
    gxy[:, 2:4] += gxy[:, 0:2]
    pxy = np.array(pred[:, :4], dtype=np.float64)
    pxy[:, 2:4] += pxy[:, 0:2]
    state = np.zeros(g, dtype=np.int64)      # 0 untouched, 1 found, -1 hit although outside the subset
    hits = np.zeros(n, dtype=np.int64)
    proposal = np.ones(n, dtype=bool)
    for h in range(n):
        o = _overlaps(gxy, pxy[h])
        if mimic_eval_bug:
            o = np.floor(o + 0.5)             # Python 2 round(): halves away from zero
        idx = int(np.argmax(o))
        if o[idx] >= iou_thresh:
            if not counted[idx]:
                state[idx] = -1
                proposal[h] = False
            elif state[idx] == 0:
                state[idx] = 1
        hits[h] = int((state == 1).sum())
    return hits, proposal


def image_pr_info(pred, hits, proposal, thresh_num=THRESH_NUM):
    """(thresh_num, 2): [number of proposals, number of subset faces found] with score >= each threshold."""
    t = np.arange(thresh_num, dtype=np.float64)
    thresh = 1 - (t + 1.) / thresh_num
    # pred is score-descending: the last row with score >= thresh is (count of such rows) - 1
    cnt = np.searchsorted(-pred[:, 4], -thresh, side='right')
    cum_prop = np.concatenate([[0], np.cumsum(proposal.astype(np.int64))])
    info = np.zeros((thresh_num, 2))
    has = cnt > 0
    info[has, 0] = cum_prop[cnt[has]]
    info[has, 1] = hits[cnt[has] - 1]
    return info


def voc_ap(rec, prec):
    mrec = np.hstack([0, rec, 1])
    mpre = np.hstack([0, prec, 0])
    for i in range(mpre.shape[0] - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def evaluate_setting(norm_preds, gt, iou_thresh=0.5, mimic_eval_bug=True, thresh_num=THRESH_NUM):
    """PR curve (thresh_num, 2) = [precision, recall] of one setting (wider_eval.py:142-177)."""
    total = np.zeros((thresh_num, 2))
    count_face = 0
    for j in range(len(gt)):
        keep = np.asarray(gt.keep[j], dtype=np.int64).reshape(-1)
        count_face += keep.shape[0]
        p = norm_preds[j]
        if gt.boxes[j].size == 0 or p is None or p.size == 0:
            continue
        hits, proposal = image_counts(p, gt.boxes[j], keep, iou_thresh, mimic_eval_bug)
        total += image_pr_info(p, hits, proposal, thresh_num)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.stack([total[:, 1] / total[:, 0], total[:, 1] / count_face], axis=1)


# ---- device path ------------------------------------------------------------------------------------------------------
MAX_DEVICE_SETTINGS = 8      # shf_wider_eval_counts takes 1..8 subset masks over one set of boxes
_FINITE_BOUND = 1e150        # below it no product or sum of _overlaps() can overflow to inf (and inf / inf to NaN)


def flatten_inputs(norm_preds, boxes, keeps):
    """The flat arrays of ``shf_wider_eval_counts``: ``norm_preds`` per image (n, 5) score-descending rows (None or
    empty: no rows), ``boxes`` per image (g, 4), ``keeps`` per SETTING the per-image index arrays of its subset.
    Returns a dict: pred5 (N, 5), pred_off (I + 1), gt4 (G, 4), gt_off (I + 1), counted (S, G) uint8."""
    n_img = len(boxes)
    pl = [np.zeros((0, 5)) if p is None else np.asarray(p, dtype=np.float64).reshape(-1, 5) for p in norm_preds]
    bl = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes]
    pred_off = np.zeros(n_img + 1, dtype=np.int64)
    gt_off = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([p.shape[0] for p in pl], out=pred_off[1:])
    np.cumsum([b.shape[0] for b in bl], out=gt_off[1:])
    if max(int(pred_off[-1]), int(gt_off[-1])) >= 2 ** 31:
        raise ValueError('flatten_inputs: 2^31 rows or more')
    counted = np.zeros((len(keeps), int(gt_off[-1])), dtype=np.uint8)
    for s, keep in enumerate(keeps):
        for j in range(n_img):
            if bl[j].shape[0]:
                # (a view of the image's segment: counted[keep] = True of image_counts, out-of-range indices raise alike)
                counted[s, gt_off[j]:gt_off[j + 1]][np.asarray(keep[j], dtype=np.int64).reshape(-1)] = 1
    return dict(pred5=np.ascontiguousarray(np.concatenate(pl, axis=0) if pl else np.zeros((0, 5))),
                pred_off=pred_off.astype(np.int32),
                gt4=np.ascontiguousarray(np.concatenate(bl, axis=0) if bl else np.zeros((0, 4))),
                gt_off=gt_off.astype(np.int32), counted=counted)


def split_flat(flat, off):
    """Inverse of the flattening: the per-image blocks of rows ``off[i] .. off[i + 1]`` of ``flat`` (pred5, gt4, or one
    setting's row of ``counted``)."""
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def sweep_thresholds(thresh_num=THRESH_NUM):
    t = np.arange(thresh_num, dtype=np.float64)
    return 1 - (t + 1.) / thresh_num       # (the expression of image_pr_info; the device is handed these values)


def device_counts(flat, iou_thresh=0.5, mimic_eval_bug=True, thresh=None, diagnostics=False):
    """One ``shf_wider_eval_counts`` call on flattened inputs.  Returns totals (S, T, 2) int64 = summed [proposals,
    subset faces found] per setting and threshold; with ``diagnostics`` also hits (S, N) int32 and proposal (S, N) bool,
    the per-detection outputs of ``image_counts``."""
    from . import _lib
    lib = _lib.load()                       # raises ShfError when the library or a GPU is missing
    thresh = np.ascontiguousarray(sweep_thresholds() if thresh is None else thresh, dtype=np.float64)
    pred5 = np.ascontiguousarray(flat['pred5'], dtype=np.float64)
    gt4 = np.ascontiguousarray(flat['gt4'], dtype=np.float64)
    pred_off = np.ascontiguousarray(flat['pred_off'], dtype=np.int32)
    gt_off = np.ascontiguousarray(flat['gt_off'], dtype=np.int32)
    counted = np.ascontiguousarray(flat['counted'], dtype=np.uint8)
    n_set, n_rows = counted.shape[0], pred5.shape[0]
    totals = np.zeros((n_set, thresh.shape[0], 2), dtype=np.int64)
    hits = np.zeros((n_set, n_rows), dtype=np.int32) if diagnostics else None
    prop = np.zeros((n_set, n_rows), dtype=np.uint8) if diagnostics else None
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    _lib.check(lib.shf_wider_eval_counts(
        pred5.ctypes.data_as(dp), pred_off.ctypes.data_as(ip), gt4.ctypes.data_as(dp), gt_off.ctypes.data_as(ip),
        counted.ctypes.data_as(bp), len(pred_off) - 1, n_set, float(iou_thresh), int(bool(mimic_eval_bug)),
        thresh.ctypes.data_as(dp), thresh.shape[0], totals.ctypes.data_as(C.POINTER(C.c_longlong)),
        hits.ctypes.data_as(ip) if diagnostics else None, prop.ctypes.data_as(bp) if diagnostics else None),
        "wider_eval_counts")
    return (totals, hits, prop.astype(bool)) if diagnostics else totals


def _share_images(gts):
    """Do the settings list the same images with the same boxes (the toolbox's three .mat files do)?"""
    a = gts[0]
    for b in gts[1:]:
        if len(b) != len(a) or any(np.shape(x) != np.shape(y) or not np.array_equal(x, y)
                                   for x, y in zip(a.boxes, b.boxes)):
            return False
    return True


def _device_safe(norm_preds, gts):
    """Every box and score finite and far from overflow: only then is the device arithmetic numpy's bit for bit (the
    arg-max of a row holding NaN is numpy's own business)."""
    def ok(x):
        x = np.asarray(x, dtype=np.float64)
        return bool(np.all(np.abs(x) < _FINITE_BOUND))
    return all(ok(p) for p in norm_preds if p is not None) and all(ok(b) for g in gts for b in g.boxes)


def _device_curves(norm_preds, gts, iou_thresh, mimic_eval_bug, thresh_num=THRESH_NUM):
    """evaluate_setting for every gt of ``gts`` with the counting on the device: one call for all settings when they
    share images and boxes, else one call per setting."""
    share = len(gts) <= MAX_DEVICE_SETTINGS and _share_images(gts)
    groups = [list(range(len(gts)))] if share else [[s] for s in range(len(gts))]
    curves = [None] * len(gts)
    for grp in groups:
        flat = flatten_inputs(norm_preds, gts[grp[0]].boxes, [gts[s].keep for s in grp])
        totals = device_counts(flat, iou_thresh, mimic_eval_bug, sweep_thresholds(thresh_num))
        for k, s in enumerate(grp):
            count_face = sum(np.asarray(kp, dtype=np.int64).reshape(-1).shape[0] for kp in gts[s].keep)
            total = totals[k].astype(np.float64)       # (exact: the host sums the same integers as float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                curves[s] = np.stack([total[:, 1] / total[:, 0], total[:, 1] / count_face], axis=1)
    return curves


def evaluate(preds, gts, iou_thresh=0.5, mimic_eval_bug=True, device=False):
    """``preds``: per image (n, 5) x-y-w-h-score arrays (any order; None = missing) in the image order shared by the
    three ``gts`` (easy, medium, hard WiderGT).  Returns ([ap_easy, ap_medium, ap_hard], [pr_curves]).
    ``device=True``: matching and threshold sweep on the GPU (same curves, bit for bit; ShfError without a GPU)."""
    norm = normalise_scores([None if p is None else sort_by_score(p) for p in preds])
    if device and not _device_safe(norm, gts):
        logging.getLogger(__name__).warning('wider_eval: non-finite boxes or scores, evaluating on the host')
        device = False
    if device:
        curves = _device_curves(norm, gts, iou_thresh, mimic_eval_bug)
    else:
        curves = [evaluate_setting(norm, g, iou_thresh, mimic_eval_bug) for g in gts]
    return [voc_ap(c[:, 1], c[:, 0]) for c in curves], curves


def wider_eval(pred_dir, gt_dir_base, silent=True, parallel=False, mimic_eval_bug=True, IoU_thresh=0.5, device=False):
    """The reference's entry point (wider_eval.py:180-222): detection text files + the toolbox's ground_truth
    directory -> (ap[3], pr_curve[3])."""
    face = load_gt_mat(os.path.join(gt_dir_base, 'wider_face_val.mat'))
    preds = read_predictions(pred_dir, face)
    gts = [load_gt_mat(os.path.join(gt_dir_base, 'wider_%s.mat' % s)) for s in SETTINGS]
    return evaluate(preds, gts, IoU_thresh, mimic_eval_bug, device=device)
