#!/usr/bin/env python3
"""Generate tests/golden/proposal_multiclass.npz from the REFERENCE's own Python: its ProposalLayer.forward (TEST phase)
and detect() with more than two classes.

Run in the authoring container only (needs the reference checkout make_golden.py names):

    python tests/golden/make_multiclass_golden.py [OUTDIR]

Like make_golden.py (whose conversion, stubs and FakeBlob it imports): the reference's lib/ is converted to py3 in a
scratch TEMP dir with lib2to3, with the same two integer-division patches in proposal_layer.py (:118, :163); nothing of
the reference is written into this repository, the fixture is DATA only.

Reference entry points exercised:
  lib/layers/proposal_layer.py:60   ProposalLayer.forward: num_classes = scores.shape[1] / A (:118), the (K A, C) regrouping
                                    (:138-140), the ranking by the best foreground class (:180), the (R, C) score top (:219)
  lib/test.py:21,109                forward_net / detect(): boxes tiled per class (:59-66), the per-class cut and merge
                                    (:161-175) under BBOX_VOTE and NMS

Proposal cases, all on a 7 x 9 map (an odd pixel count), `scores` laid out as the net lays them out: channel c * A + a.
  c3_a3, c3_a8, c4_a8          random class probabilities, C = 3 / 4, A = 3 (the template's param string) / 8
                               ('shifts': [0, 0.5] over two strides: sub-strides 1,1,1,1,2,2,2,2)
  tie_classes                  two anchors hold the same best foreground score, one in class 1 and one in class 2
                               (argsort()[::-1] leaves the order of ties to the implementation: consumers compare
                               canonically, as with proposal.npz `ties`)
  class2_wins                  SCORE_THRESH 0.3: rows are kept whose class 1 is below the threshold and class 2 is not
  topn_cut                     C = 4, A = 3: N_DETS_PER_MODULE 40 cuts the candidates
  none_at_thresh               C = 4, probabilities halved, SCORE_THRESH 0.6: nothing reaches it, the single best anchor by its best foreground class
  none_valid                   ANCHOR_MIN_SIZE 1000: nothing valid, the dummy roi and a (0, C) score top

detect(): one scale with TEST.FLIP (two units, the second flipped) over a canned net that returns (R, 3) scores; the
per-unit net outputs and both classes' merged boxes are stored, under BBOX_VOTE and under NMS.  lib/test.py calls
``nms`` without importing it (NameError under NMS_METHOD "NMS"); the generator binds the reference's own
nms/py_cpu_nms.py:py_cpu_nms to that name.  Scores are distinct, so no order is left to the sort's implementation.
"""
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FakeBlob, convert_reference, install_stubs  # noqa: E402

OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
MAP = (7, 9)
PSTR_A3 = "{'feat_stride': [8,8,8],'scales': [1,2,4], 'ratios':[1,]}"
PSTR_A8 = "{'feat_stride': [8,16], 'scales': [1,2], 'ratios': [1,], 'shifts': [0,0.5]}"


def class_probs(rng, C, A, h, w, spread=2.0, bg_bias=1.0):
    """(1, C*A, h, w) float32 probabilities, channel c * A + a; a float32 softmax over the classes of every anchor."""
    lg = rng.normal(0, spread, (C, A, h, w)).astype(np.float32)
    lg[0] += np.float32(bg_bias)
    e = np.exp(lg - lg.max(axis=0, keepdims=True)).astype(np.float32)
    p = (e / e.sum(axis=0, keepdims=True, dtype=np.float32)).astype(np.float32)
    return p.reshape(1, C * A, h, w)


def deltas(rng, A, h, w):
    """(1, 4A, h, w) box deltas, N(0, 0.3) on a 1/64 grid (exact in float32; the fixture compresses)."""
    return (np.round(rng.normal(0, 0.3, (1, 4 * A, h, w)) * 64) / 64).astype(np.float32)


class FakeNet3(object):
    """A canned 3-class net: (R, 5) boxes and (R, 3) scores per forward, rows ranked by the best foreground class."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.blobs = {"data": FakeBlob(np.zeros((1, 3, 16, 16))), "im_info": FakeBlob(np.zeros((1, 3))),
                      "boxes": FakeBlob(np.zeros((1, 5))), "cls_prob": FakeBlob(np.zeros((1, 3)))}
        self.outputs = []

    def forward(self, data=None, im_info=None):
        h, w, s = im_info[0]
        n = int(self.rng.integers(25, 40))
        # a handful of clusters, so that votes and suppressions happen
        cx, cy = self.rng.uniform(10, w - 10, 6), self.rng.uniform(10, h - 10, 6)
        k = self.rng.integers(0, 6, n)
        half = self.rng.uniform(4, 9, n)
        x1 = np.clip(cx[k] - half + self.rng.normal(0, 1, n), 0, w - 3)
        y1 = np.clip(cy[k] - half + self.rng.normal(0, 1, n), 0, h - 3)
        x2 = np.minimum(x1 + 2 * half, w - 1)
        y2 = np.minimum(y1 + 2 * half, h - 1)
        p = self.rng.dirichlet([1.0, 0.8, 0.8], n)
        p = p[np.argsort(-p[:, 1:].max(axis=1))]
        boxes = np.stack([np.zeros(n), x1, y1, x2, y2], 1).astype(np.float32)
        probs = p.astype(np.float32)
        self.outputs.append((boxes.copy(), probs.copy(), im_info.copy(), tuple(data.shape)))
        self.blobs["boxes"].data = boxes
        self.blobs["cls_prob"].data = probs
        return {"boxes": self.blobs["boxes"].data, "cls_prob": self.blobs["cls_prob"].data}


def main():
    import numpy.ma  # noqa: F401  (before the np.bool alias of install_stubs)
    import scipy.io  # noqa: F401
    tmp = tempfile.mkdtemp(prefix="shf_ref_py3_")
    convert_reference(tmp)
    fake_cv2 = types.ModuleType("cv2")
    fake_cv2.INTER_LINEAR = 1
    fake_cv2._images = {}
    fake_cv2.imread = lambda p: fake_cv2._images[p].copy()
    sys.path.insert(0, os.path.join(HERE, "..", ".."))

    def _resize(im, a, b, fx=None, fy=None, interpolation=None):
        from oracle.resize import cv_resize_linear_f64
        return cv_resize_linear_f64(im, fx, fy)

    fake_cv2.resize = _resize
    install_stubs(fake_cv2)
    os.chdir(tmp)
    sys.path.insert(0, tmp)
    sys.path.insert(0, os.path.join(tmp, "lib"))

    from utils.get_config import cfg, cfg_from_file, cfg_from_list
    cfg_from_file("configs/smallhardface.toml")
    cfg.TEST.NO_CACHE = True
    cfg_from_list(["TEST.MODEL", "dummy.caffemodel", "TEST.GPU_ID", "[0]"])
    from lib.layers.proposal_layer import ProposalLayer
    from nms.py_cpu_nms import py_cpu_nms
    import test as ref_test

    def run_proposal(scores, deltas, im_info, pstr, topn, thresh, min_size):
        old = (cfg.TEST.N_DETS_PER_MODULE, cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE)
        cfg.TEST.N_DETS_PER_MODULE, cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE = topn, thresh, min_size
        L = ProposalLayer()
        L.param_str = pstr
        L.phase = 1
        bottom = [FakeBlob(scores), FakeBlob(deltas), FakeBlob(im_info)]
        top = [FakeBlob(), FakeBlob()]
        L.setup(bottom, top)
        keep_out = sys.stdout
        sys.stdout = io.StringIO()
        try:
            L.forward(bottom, top)
        finally:
            sys.stdout = keep_out
            cfg.TEST.N_DETS_PER_MODULE, cfg.TEST.SCORE_THRESH, cfg.TEST.ANCHOR_MIN_SIZE = old
        return top[0].data.copy(), top[1].data.copy()

    h, w = MAP
    fx = {}
    names = []

    def record(name, C, A, pstr, sc, dl, topn=10000, thresh=0.002, min_size=0.0):
        ii = np.array([[8 * h - 3, 8 * w - 5, 1.5]], np.float32)
        assert sc.shape == (1, C * A, h, w) and dl.shape == (1, 4 * A, h, w)
        b, p = run_proposal(sc, dl, ii, pstr, topn, thresh, min_size)
        assert p.ndim == 2 and p.shape[1] == C, p.shape
        fx[name + "_scores"], fx[name + "_deltas"], fx[name + "_im_info"] = sc, dl, ii
        fx[name + "_cfg"] = np.array([topn, thresh, min_size], np.float64)
        fx[name + "_classes"] = np.array([C, A])
        fx[name + "_param_str"] = np.array(pstr)
        fx[name + "_boxes"], fx[name + "_probs"] = b, p
        names.append(name)
        print("proposal_multiclass %-16s C %d A %d: %d rows of %d anchors" % (name, C, A, len(p), h * w * A))
        return b, p

    for seed, (name, C, A, pstr) in enumerate([("c3_a3", 3, 3, PSTR_A3), ("c3_a8", 3, 8, PSTR_A8), ("c4_a8", 4, 8, PSTR_A8)]):
        r = np.random.default_rng(300 + seed)
        b, p = record(name, C, A, pstr, class_probs(r, C, A, h, w), deltas(r, A, h, w))
        assert len(p) > 20 and all((p[:, 1:].argmax(axis=1) == c - 1).any() for c in range(1, C))

    # two anchors with the same best foreground score in different classes, above everything else
    r = np.random.default_rng(310)
    C, A = 3, 3
    sc = class_probs(r, C, A, h, w).reshape(C, A, h, w)
    sc = sc * np.float32(0.5)      # (exact: no new ties; everything else stays below the pair's 0.75)
    sc[:, 1, 2, 3] = (0.125, 0.75, 0.125)
    sc[:, 0, 5, 6] = (0.125, 0.125, 0.75)
    b, p = record("tie_classes", C, A, PSTR_A3, sc.reshape(1, C * A, h, w).astype(np.float32),
                  deltas(r, A, h, w))
    assert sorted(map(tuple, p[:2].tolist())) == [(0.125, 0.125, 0.75), (0.125, 0.75, 0.125)]

    r = np.random.default_rng(311)
    b, p = record("class2_wins", 3, 3, PSTR_A3, class_probs(r, 3, 3, h, w), deltas(r, 3, h, w), thresh=0.3)
    assert ((p[:, 1] < 0.3) & (p[:, 2] >= 0.3)).sum() > 5 and ((p[:, 1] >= 0.3) & (p[:, 2] < 0.3)).sum() > 5

    r = np.random.default_rng(312)
    b, p = record("topn_cut", 4, 3, PSTR_A3, class_probs(r, 4, 3, h, w), deltas(r, 3, h, w), topn=40)
    assert len(p) == 40 and len(np.unique(p[:, 1:].max(axis=1))) == 40

    r = np.random.default_rng(313)
    b, p = record("none_at_thresh", 4, 3, PSTR_A3, class_probs(r, 4, 3, h, w) * np.float32(0.5),
                  deltas(r, 3, h, w), thresh=0.6)
    assert p.shape == (1, 4) and p[0, 1:].max() < 0.5
    best = np.sort(fx["none_at_thresh_scores"][0, 3:].reshape(3, -1).max(axis=0))
    assert best[-1] == p[0, 1:].max() > best[-2]          # one best anchor: no tie to order

    r = np.random.default_rng(314)
    b, p = record("none_valid", 3, 3, PSTR_A3, class_probs(r, 3, 3, h, w), deltas(r, 3, h, w), min_size=1000.0)
    assert p.shape == (0, 3) and b.tolist() == [[0, 0, 0, 16, 16]]
    fx["cases"] = np.array(names)

    # ---- detect(): two units (one flipped) of a canned 3-class net -------------------------------------------------------
    ref_test.nms = lambda dets, thresh: py_cpu_nms(dets, thresh) if dets.shape[0] else []
    im = np.random.default_rng(520).integers(0, 256, (90, 120, 3)).astype(np.uint8)
    fake_cv2._images["mc.jpg"] = im
    cfg.TEST.SCALES = [cfg.TEST.PYRAMID_BASE_SIZE[0]]
    cfg.TEST.FLIP = True
    for method in ("BBOX_VOTE", "NMS"):
        cfg.TEST.NMS_METHOD = method
        net = FakeNet3(930)
        cls_dets, _ = ref_test.detect(net, "mc.jpg", thresh=0.05, pyramid=True)
        assert len(cls_dets) == 2 and len(net.outputs) == 2
        for c in range(2):
            fx["detect_%s_dets%d" % (method, c)] = np.asarray(cls_dets[c], dtype=np.float64)
            assert len(cls_dets[c]) > 3
        if method == "BBOX_VOTE":
            for u, (boxes, probs, info, shape) in enumerate(net.outputs):
                assert len(np.unique(probs[:, 1:])) == probs[:, 1:].size
                fx["detect_u%d_boxes" % u], fx["detect_u%d_probs" % u] = boxes, probs
                fx["detect_u%d_im_info" % u] = info
                fx["detect_u%d_flip" % u] = np.array([u])
                fx["detect_u%d_width" % u] = np.array([int(info[0, 1])])
    fx["detect_thresh"] = np.array([0.05])
    fx["detect_nms_thresh"] = np.array([float(cfg.TEST.NMS_THRESH)])

    np.savez_compressed(os.path.join(OUT, "proposal_multiclass.npz"), **fx)
    shutil.rmtree(tmp, ignore_errors=True)
    print("proposal_multiclass.npz written to", OUT, os.path.getsize(os.path.join(OUT, "proposal_multiclass.npz")), "bytes")


if __name__ == "__main__":
    main()
