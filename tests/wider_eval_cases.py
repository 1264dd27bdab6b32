"""Shared by test_wider_eval_parallel_form.py (CPU) and test_gpu_wider_eval.py: the numpy restatement of the evaluator's
parallel form (the specification of csrc/eval.hip), seeded cases that sit on its edges, and the host reference built from
the unchanged ``image_counts`` / ``image_pr_info``."""
import json
import os

import numpy as np

from smallhardface_amd import wider_eval as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_case():
    """tests/golden/wider_eval.npz (the reference's own run) -> (npz, [easy, medium, hard WiderGT], preds)."""
    def split(flat, counts):
        out, o = [], 0
        for c in counts:
            out.append(flat[o:o + c])
            o += c
        return out
    g = np.load(os.path.join(GOLDEN, "wider_eval.npz"))
    names = json.load(open(os.path.join(GOLDEN, "wider_eval_names.json")))
    n = int(g["n_images"][0])
    boxes = split(g["gt_boxes"], g["gt_count"])
    preds = split(g["preds"], g["pred_count"])
    events = [names["events"][i // 2] for i in range(n)]
    gts = [W.WiderGT(events, names["files"], boxes, [k - 1 for k in split(g["sub_%s" % s], g["sub_%s_count" % s])])
           for s in ("easy", "medium", "hard")]
    return g, gts, preds


# ---- the parallel form, in numpy ------------------------------------------------------------------------------------------
def parallel_counts(flat, iou_thresh, mimic_eval_bug, thresh):
    """What shf_wider_eval_counts computes, step for step: (totals (S, T, 2) int64, hits (S, N) int32, proposal (S, N) bool).
    1. match: per detection the first arg-max box of its (rounded) IoU row and whether that value reaches iou_thresh --
       no state, no setting;  2. per setting: first[g] = earliest detection matched to g, proposal / flag per detection,
       hits = inclusive prefix sum of flag within the image;  3. sweep: cnt = detections with score >= threshold by
       binary search, info = (prefix_sum(proposal)[cnt], hits[cnt - 1]) when cnt > 0, summed over images as integers."""
    pred5, po, gt4, go, counted = flat["pred5"], flat["pred_off"], flat["gt4"], flat["gt_off"], flat["counted"]
    n_img, n_set, n_rows, n_gt = len(po) - 1, counted.shape[0], pred5.shape[0], gt4.shape[0]
    match = np.full(n_rows, -1, dtype=np.int64)
    for i in range(n_img):
        p, g = pred5[po[i]:po[i + 1]], gt4[go[i]:go[i + 1]]
        if not len(p) or not len(g):
            continue
        gx = np.array(g, dtype=np.float64)
        gx[:, 2:4] += gx[:, 0:2]
        b = np.array(p[:, :4], dtype=np.float64)
        b[:, 2:4] += b[:, 0:2]
        iw = np.minimum(gx[None, :, 2], b[:, None, 2]) - np.maximum(gx[None, :, 0], b[:, None, 0]) + 1
        ih = np.minimum(gx[None, :, 3], b[:, None, 3]) - np.maximum(gx[None, :, 1], b[:, None, 1]) + 1
        inter = iw * ih
        union = ((gx[:, 2] - gx[:, 0] + 1) * (gx[:, 3] - gx[:, 1] + 1))[None, :] + \
            ((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1))[:, None] - inter
        union = np.where(union == 0, np.inf, union)
        key = inter / union
        key[(iw <= 0) | (ih <= 0)] = 0
        if mimic_eval_bug:
            key = np.floor(key + 0.5)
        idx = np.argmax(key, axis=1)                       # first index on ties
        matched = key[np.arange(len(p)), idx] >= iou_thresh
        match[po[i]:po[i + 1]] = np.where(matched, go[i] + idx, -1)
    h = np.arange(n_rows)
    m = match >= 0
    first = np.full(n_gt, np.iinfo(np.int32).max, dtype=np.int64)
    np.minimum.at(first, match[m], h[m])                   # (the kernel's atomic min)
    totals = np.zeros((n_set, len(thresh), 2), dtype=np.int64)
    hits = np.zeros((n_set, n_rows), dtype=np.int32)
    proposal = np.ones((n_set, n_rows), dtype=bool)
    for s in range(n_set):
        in_subset = np.zeros(n_rows, dtype=bool)
        in_subset[m] = counted[s][match[m]] != 0
        proposal[s] = ~(m & ~in_subset)
        flag = np.zeros(n_rows, dtype=bool)
        flag[m] = in_subset[m] & (first[match[m]] == h[m])
        for i in range(n_img):
            a, e = po[i], po[i + 1]
            hits[s, a:e] = np.cumsum(flag[a:e])
            if e == a or go[i + 1] == go[i]:
                continue
            cum_prop = np.cumsum(proposal[s, a:e])
            cnt = np.searchsorted(-pred5[a:e, 4], -thresh, side="right")
            has = cnt > 0
            totals[s, has, 0] += cum_prop[cnt[has] - 1]
            totals[s, has, 1] += hits[s, a:e][cnt[has] - 1]
    return totals, hits, proposal


# ---- the host reference ---------------------------------------------------------------------------------------------------
def host_counts(preds, boxes, keeps, iou_thresh, mimic_eval_bug, thresh_num=W.THRESH_NUM):
    """The unchanged host functions on per-image arrays: totals (S, thresh_num, 2) int64 as evaluate_setting sums them, and the
    concatenated per-detection hits (S, N) / proposal (S, N) of image_counts (images without boxes: no hit, all proposals)."""
    n_set = len(keeps)
    totals = np.zeros((n_set, thresh_num, 2))
    hits, prop = [[] for _ in keeps], [[] for _ in keeps]
    for s in range(n_set):
        for j, p in enumerate(preds):
            if p is None or p.size == 0:
                continue
            if boxes[j].size == 0:
                hits[s].append(np.zeros(len(p), dtype=np.int64))
                prop[s].append(np.ones(len(p), dtype=bool))
                continue
            keep = np.asarray(keeps[s][j], dtype=np.int64).reshape(-1)
            hh, pp = W.image_counts(p, boxes[j], keep, iou_thresh, mimic_eval_bug)
            totals[s] += W.image_pr_info(p, hh, pp, thresh_num)
            hits[s].append(hh)
            prop[s].append(pp)
    cat = lambda rows, dt: np.stack([np.concatenate(r) if r else np.zeros(0, dt) for r in rows]).astype(dt)
    assert np.array_equal(totals, np.rint(totals))
    return totals.astype(np.int64), cat(hits, np.int32), cat(prop, bool)


# ---- seeded cases ---------------------------------------------------------------------------------------------------------
def make_image(rng, g, n, real):
    """One image: g ground-truth boxes and n score-descending detections that sit on the evaluator's edges -- detections
    jittered around boxes (IoU on both sides of the threshold), exact copies of a box, duplicated boxes (arg-max ties),
    negative detection widths / heights (IoU outside [0, 1]), and scores quantised onto the sweep's thresholds with ties."""
    xy = rng.uniform(0, 300, (g, 2))
    wh = rng.uniform(4, 60, (g, 2))
    gt = np.hstack([xy, wh])
    if not real:
        gt = np.rint(gt)
    if g > 1:
        dup = rng.choice(g, max(1, g // 8), replace=False)
        gt[dup] = gt[rng.integers(0, g, len(dup))]        # identical boxes: the first index must win
    src = rng.integers(0, g, n)
    det = gt[src] + rng.uniform(-1, 1, (n, 4)) * gt[src][:, [2, 3, 2, 3]] * rng.choice([0.0, 0.1, 0.35, 1.5], (n, 1))
    if not real:
        det = np.rint(det)
    neg = rng.random(n) < 0.1
    det[neg, 2] = -np.abs(det[neg, 2]) - 2                # negative width
    neg = rng.random(n) < 0.05
    det[neg, 3] = -np.abs(det[neg, 3]) - 2
    th = W.sweep_thresholds()
    score = np.where(rng.random(n) < 0.5, th[rng.integers(0, len(th), n)], rng.random(n))   # on a threshold, bit for bit
    pred = W.sort_by_score(np.hstack([det, score[:, None]]))
    return pred, gt


def subsets(rng, g):
    """(empty, partial, full) keep-index arrays for an image with g boxes."""
    part = np.flatnonzero(rng.random(g) < 0.5)
    return [np.zeros(0, dtype=np.int64), part, np.arange(g)]


G_SIZES = (1, 63, 64, 65, 129)        # lane, wave and tile boundaries of the ground-truth walk ...
N_SIZES = (1, 63, 64, 65, 257)        # ... and of the 64-detection tiles and scans


def boundary_batch(seed, real):
    """Every (g, n) of G_SIZES x N_SIZES as one batch of 25 images with three settings (empty / partial / full subset):
    (preds, boxes, keeps)."""
    rng = np.random.default_rng(seed)
    preds, boxes, keeps = [], [], [[], [], []]
    for g in G_SIZES:
        for n in N_SIZES:
            p, b = make_image(rng, g, n, real)
            preds.append(p)
            boxes.append(b)
            for s, k in enumerate(subsets(rng, g)):
                keeps[s].append(k)
    return preds, boxes, keeps
