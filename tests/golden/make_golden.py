#!/usr/bin/env python3
"""Generate golden input/output vectors from the REFERENCE's own Python.

Run in the authoring container only (needs /root/reference):

    python tests/golden/make_golden.py [OUTDIR]

OUTDIR (default: this directory) receives every fixture; to add one fixture without touching the committed ones, write
to a scratch directory, compare the arrays of the others and copy only the new file over.

What it does (nothing from the reference is copied into this repo):
  * converts /root/reference/lib + configs to py3 in a scratch TEMP dir with
    lib2to3 (all fixers except fix_import), patches the two Py2 integer
    divisions in proposal_layer.py (:118, :163) to ``//`` and the Py2
    comprehension-variable leak in utils/blob.py:23;
  * installs tiny stub modules for things the container lacks (caffe, cv2,
    toml, easydict, requests, nms.cpu_nms/gpu_nms);
  * imports the reference modules and drives them on seeded inputs;
  * writes inputs + expected outputs as small .npz/.json fixtures next to
    this script.  The fixtures are DATA only.

Reference entry points exercised (file:line in /root/reference):
  lib/layers/generate_anchors.py:11   generate_anchors
  lib/layers/proposal_layer.py:60     ProposalLayer.forward (TEST phase), also under param strings with two / three
                                      ratios, shifts, unequal strides, base sizes 8 / 12 and 'subsampled': False
  lib/utils/bbox_transform.py:33,80   bbox_transform_inv / clip_boxes
  lib/test.py:181                     bbox_vote
  lib/nms/py_cpu_nms.py:10            py_cpu_nms
  lib/test.py:21                      forward_net (flip / unscale / tile)
  lib/test.py:109                     detect (pyramid orchestration, fake net)
  lib/utils/test_utils.py:8           _compute_scaling_factor (+ test.py:131-137)
  lib/utils/get_config.py:134,140     cfg_from_file / cfg_from_list
  lib/datasets/wider.py:143           write_detections line format
  lib/datasets/{wider,fddb,afw,pascalface}.py   write_detections of the four imdbs (files as text)
  lib/wider_eval_tools/wider_eval.py:180   wider_eval on a synthetic ground truth (.mat) + detection files
  models/test_*template.prototxt      structural digest of both inference templates
"""
import io
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE

# ProposalLayer param strings beyond the templates' (proposal_geometry.npz); every anchor stays <= 64 px
GEOMETRIES = [
    # anchors 22x12, 33x18, 12x24, 18x36; zip(scales, strides) drops two strides; sub-strides 1, 2, 2, 2
    ("two_ratios_mixed_strides", "{'feat_stride': [8,16,16,16], 'scales': [2,3], 'ratios': [0.5,2], 'base_size': 8}"),
    # four shifted copies per scale, A = 8; sub-strides 1,1,1,1,2,2,2,2
    ("shifts_two_strides", "{'feat_stride': [8,16], 'scales': [1,2], 'ratios': [1,], 'shifts': [0,0.5]}"),
    # the unfiltered map, A = 6, anchors from 11x22 to 46x24
    ("three_ratios_dense", "{'feat_stride': [8,8], 'scales': [1,2], 'ratios': [0.5,1,2], 'subsampled': False}"),
    # feat_stride[0] != 8; sub-strides 1, 2, 4 on an odd map: ragged last row and column
    ("strides_4_8_16", "{'feat_stride': [4,8,16], 'scales': [1,2,4], 'ratios': [2,], 'base_size': 12}"),
]
GEOMETRY_MAP = (7, 9)
GEOMETRY_SCALE = 1.5
GEOMETRY_MIN_SIZE = 6


# --------------------------------------------------------------------------
# scratch conversion
# --------------------------------------------------------------------------
def convert_reference(tmp):
    from lib2to3 import refactor
    fixers = [f for f in refactor.get_fixers_from_package("lib2to3.fixes")
              if not f.endswith("fix_import")]
    rt = refactor.RefactoringTool(fixers)
    for sub in ("lib", "configs"):
        shutil.copytree(os.path.join(REF, sub), os.path.join(tmp, sub))
    for root, _, files in os.walk(os.path.join(tmp, "lib")):
        for fn in files:
            if not fn.endswith(".py"):
                continue
            p = os.path.join(root, fn)
            src = open(p).read()
            if not src.endswith("\n"):
                src += "\n"
            try:
                out = str(rt.refactor_string(src, p))
            except Exception as e:  # pragma: no cover
                print("2to3 failed for", p, e)
                continue
            if fn == "proposal_layer.py":
                a = "num_classes = scores.shape[1] / (A * self._num_feats)"
                b = "stride = self._feat_stride[i / len(self._shifts)**"
                assert a in out and b in out
                out = out.replace(a, a.replace(" / ", " // "))
                out = out.replace(b, b.replace("[i / len", "[i // len"))
            if fn == "blob.py":
                # Py2 leaked the list-comprehension variable `im` (blob.py:21-23)
                a = "max_shape[1], im.shape[2])"
                assert a in out
                out = out.replace(a, "max_shape[1], ims[0].shape[2])")
            open(p, "w").write(out)


def install_stubs(fake_cv2):
    np.float = float  # noqa  (np 2.x removed the aliases the reference uses)
    np.int = int  # noqa
    np.bool = bool  # noqa
    import yaml
    _load = yaml.load
    yaml.load = lambda s, Loader=None: _load(s, Loader=yaml.SafeLoader)

    caffe = types.ModuleType("caffe")
    caffe.Layer = object
    caffe.TEST = 1
    caffe.TRAIN = 0
    sys.modules["caffe"] = caffe

    sys.modules["cv2"] = fake_cv2

    import tomli
    toml = types.ModuleType("toml")
    toml.load = lambda p: tomli.load(open(p, "rb"))
    toml.loads = tomli.loads
    toml.dumps = lambda d: repr(d)
    toml.dump = lambda d, f: f.write(repr(d))
    sys.modules["toml"] = toml

    ed = types.ModuleType("easydict")

    class EasyDict(dict):
        def __init__(self, d=None, **kw):
            super().__init__()
            d = dict(d or {}, **kw)
            for k, v in d.items():
                self[k] = v

        def __setitem__(self, k, v):
            if isinstance(v, dict) and not isinstance(v, EasyDict):
                v = EasyDict(v)
            super().__setitem__(k, v)

        __setattr__ = __setitem__

        def __getattr__(self, k):
            try:
                return self[k]
            except KeyError:
                raise AttributeError(k)

        def has_key(self, k):
            return k in self

        def iteritems(self):
            return self.items()

    ed.EasyDict = EasyDict
    sys.modules["easydict"] = ed

    sys.modules.setdefault("requests", types.ModuleType("requests"))
    for name in ("nms.cpu_nms", "nms.gpu_nms"):
        m = types.ModuleType(name)
        m.cpu_nms = None
        m.gpu_nms = None
        sys.modules[name] = m


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
class FakeBlob(object):
    def __init__(self, arr=None):
        self.data = None if arr is None else np.array(arr, dtype=np.float32)

    def reshape(self, *dims):
        if self.data is None or self.data.shape != tuple(dims):
            self.data = np.zeros(dims, dtype=np.float32)

    @property
    def shape(self):
        return self.data.shape


class FakeNet(object):
    """Returns canned proposal outputs; records what the driver fed it."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.blobs = {"data": FakeBlob(np.zeros((1, 3, 16, 16))),
                      "im_info": FakeBlob(np.zeros((1, 3))),
                      "boxes": FakeBlob(np.zeros((1, 5))),
                      "cls_prob": FakeBlob(np.zeros((1, 2)))}
        self.calls = []

    def forward(self, data=None, im_info=None):
        h, w, s = im_info[0]
        self.calls.append((tuple(data.shape), im_info.copy(),
                           float(data.sum()), float(data[0, 0, 0, 0])))
        n = int(self.rng.integers(3, 40))
        x1 = self.rng.uniform(0, w - 2, n)
        y1 = self.rng.uniform(0, h - 2, n)
        x2 = np.minimum(x1 + self.rng.uniform(1, w / 3 + 2, n), w - 1)
        y2 = np.minimum(y1 + self.rng.uniform(1, h / 3 + 2, n), h - 1)
        fg = np.sort(self.rng.uniform(0.002, 1, n))[::-1]
        self.blobs["boxes"].data = np.stack(
            [np.zeros(n), x1, y1, x2, y2], 1).astype(np.float32)
        self.blobs["cls_prob"].data = np.stack([1 - fg, fg], 1).astype(np.float32)
        return {"boxes": self.blobs["boxes"].data, "cls_prob": self.blobs["cls_prob"].data}


def softmax_blob(rng, h, w, bias):
    """(1,6,h,w) blob laid out as the net does: channel c*3+d, bg+fg = 1."""
    logit = rng.normal(0, 2.0, size=(3, h, w)).astype(np.float32) + np.float32(bias)
    fg = (1.0 / (1.0 + np.exp(-logit.astype(np.float64)))).astype(np.float32)
    bg = (np.float32(1.0) - fg).astype(np.float32)
    return np.concatenate([bg, fg], axis=0)[None].astype(np.float32)


def clustered_dets(rng, n_centers, per, jitter, size=(20, 120), extent=900.0, quant=None):
    rows = []
    for _ in range(n_centers):
        cx, cy = rng.uniform(50, extent, 2)
        s = rng.uniform(*size)
        for _ in range(int(rng.integers(1, per + 1))):
            j = rng.normal(0, jitter * s, 4)
            x1, y1 = cx - s / 2 + j[0], cy - s / 2 + j[1]
            # keep boxes non-degenerate: the reference's bbox_vote never
            # terminates on a box whose IoU with itself is < thresh
            x2 = max(cx + s / 2 + j[2], x1 + 2.0)
            y2 = max(cy + s / 2 + j[3], y1 + 2.0)
            sc = rng.uniform(0.05, 1.0)
            rows.append([x1, y1, x2, y2, sc])
    d = np.array(rows, dtype=np.float32).reshape(-1, 5)
    if quant:
        d[:, 4] = np.round(d[:, 4] * quant) / quant
    return d


def main():
    import numpy.ma  # noqa: F401  (before the np.bool alias below: numpy.ma's import trips over it)
    import scipy.io  # noqa: F401
    tmp = tempfile.mkdtemp(prefix="shf_ref_py3_")
    convert_reference(tmp)

    # --- fake cv2: registry-backed imread, resize delegated to the ORACLE's independent restatement of
    # cv2.resize (oracle/resize.py -- not the product's host mirror), so the detect() fixture pins orchestration
    # only (cv2 parity itself is unpinned: OpenCV is not installable here).
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

    from lib.layers.generate_anchors import generate_anchors
    from lib.layers.proposal_layer import ProposalLayer
    from utils.bbox_transform import bbox_transform_inv, clip_boxes
    from nms.py_cpu_nms import py_cpu_nms
    import test as ref_test
    from utils.test_utils import _compute_scaling_factor

    # ---------------- config -------------------------------------------
    cfg_dump = {
        "MAX_RESOLUTION": cfg.MAX_RESOLUTION,
        "PIXEL_MEANS": cfg.PIXEL_MEANS,
        "USE_GPU_NMS": cfg.USE_GPU_NMS,
        "MODEL.DIFFERENT_DILATION.ENABLE": cfg.MODEL.DIFFERENT_DILATION.ENABLE,
        "TEST": {k: cfg.TEST[k] for k in (
            "SCALES", "PYRAMID_BASE_SIZE", "FLIP", "MAX_SIZE", "ORIG_SIZE",
            "SCORE_THRESH", "N_DETS_PER_MODULE", "ANCHOR_MIN_SIZE", "NMS_THRESH",
            "NMS_METHOD", "LEVEL", "GPU_ID", "MODEL", "PROTOTXT", "NO_CACHE",
            "IOU_THRESH", "DB")},
    }
    json.dump(cfg_dump, open(os.path.join(OUT, "config_smallhardface.json"), "w"),
              indent=1, sort_keys=True)

    # ---------------- anchors ------------------------------------------
    anc = {}
    anc["default_param_str"] = generate_anchors(
        scales=np.array([1, 2, 4]), base_size=16, ratios=np.array([1, ]),
        shifts=np.array([0]), strides=np.array([8, 8, 8]))
    anc["frcnn_defaults"] = generate_anchors(
        scales=np.array((8, 16, 32)), base_size=16, ratios=np.array((0.5, 1, 2)),
        shifts=np.array([0]), strides=np.array([16] * 3))
    anc["two_ratios_base8"] = generate_anchors(
        scales=np.array([2, 3]), base_size=8, ratios=np.array([0.5, 2]),
        shifts=np.array([0]), strides=np.array([8, 8]))
    np.savez(os.path.join(OUT, "anchors.npz"), **anc)

    # ---------------- bbox_transform_inv / clip ------------------------
    rng = np.random.default_rng(11)
    boxes = np.stack([rng.uniform(0, 300, 64), rng.uniform(0, 300, 64)], 1)
    boxes = np.concatenate([boxes, boxes + rng.uniform(1, 200, (64, 2))], 1)  # f64
    deltas = rng.normal(0, 0.5, (64, 4)).astype(np.float32)
    out = bbox_transform_inv(boxes.copy(), deltas.copy())
    clipped = clip_boxes(out.copy(), np.array([240., 320.], dtype=np.float32))
    d_of = deltas.copy()
    d_of[3, 2] = 120.0   # exp overflow in fp32 -> FloatingPointError -> clamp branch
    d_of[7, 3] = 60.0    # >50 but no overflow by itself: clamped only because of [3,2]
    d_of[9, 2] = 55.0
    old = sys.stdout
    sys.stdout = io.StringIO()
    out_of = bbox_transform_inv(boxes.copy(), d_of.copy())
    sys.stdout = old
    d_big = deltas.copy()
    d_big[5, 2] = 60.0   # big but finite: NOT clamped
    out_big = bbox_transform_inv(boxes.copy(), d_big.copy())
    np.savez(os.path.join(OUT, "bbox_transform.npz"), boxes=boxes, deltas=deltas,
             pred=out, clipped=clipped, im_shape=np.array([240., 320.], np.float32),
             deltas_overflow=d_of, pred_overflow=out_of,
             deltas_big=d_big, pred_big=out_big)

    # ---------------- ProposalLayer.forward ----------------------------
    def run_proposal(scores, deltas, im_info, param_str=None):
        L = ProposalLayer()
        L.param_str = param_str or "{'feat_stride': [8,8,8],'scales': [1,2,4], 'ratios':[1,]}"
        L.phase = 1
        bottom = [FakeBlob(scores), FakeBlob(deltas), FakeBlob(im_info)]
        top = [FakeBlob(), FakeBlob()]
        L.setup(bottom, top)
        old = sys.stdout
        sys.stdout = io.StringIO()
        try:
            L.forward(bottom, top)
        finally:
            sys.stdout = old
        return top[0].data.copy(), top[1].data.copy()

    prop = {}
    cases = [
        # name, h, w, im_info(h,w,scale), bias, delta_std, seed
        ("small", 8, 10, (64, 80, 1.0), -2.0, 0.5, 1),
        ("unpadded", 14, 14, (100, 100, 0.09765625), -3.0, 0.4, 2),      # 112 padded, 100 real
        ("wide", 19, 38, (150, 300, 0.29296875), -4.0, 0.3, 3),
        ("all_below", 6, 7, (48, 56, 1.0), -12.0, 0.3, 4),               # nothing >= 0.002
        ("over_10000", 64, 64, (512, 512, 1.0), 2.0, 0.3, 5),            # 12288 anchors, ~all kept
        ("c1_512", 64, 64, (512, 512, 1.0), -5.0, 0.3, 6),
    ]
    for name, h, w, info, bias, dstd, seed in cases:
        r = np.random.default_rng(seed)
        sc = softmax_blob(r, h, w, bias)
        dl = r.normal(0, dstd, (1, 12, h, w)).astype(np.float32)
        ii = np.array([info], dtype=np.float32)
        b, p = run_proposal(sc, dl, ii)
        prop[name + "_scores"] = sc
        prop[name + "_deltas"] = dl
        prop[name + "_im_info"] = ii
        prop[name + "_boxes"] = b
        prop[name + "_probs"] = p
    # overflow/clamp branch inside the layer
    r = np.random.default_rng(7)
    sc = softmax_blob(r, 5, 6, 0.0)
    dl = r.normal(0, 0.3, (1, 12, 5, 6)).astype(np.float32)
    dl[0, 2, 1, 1] = 130.0
    dl[0, 7, 2, 3] = 70.0
    ii = np.array([[40, 48, 1.0]], dtype=np.float32)
    b, p = run_proposal(sc, dl, ii)
    prop.update(overflow_scores=sc, overflow_deltas=dl, overflow_im_info=ii,
                overflow_boxes=b, overflow_probs=p)
    # tie scores (order among ties is implementation-defined; consumers compare canonically)
    r = np.random.default_rng(8)
    sc = softmax_blob(r, 9, 9, -1.0)
    fg = np.round(sc[0, 3:6] * 8) / 8
    sc = np.concatenate([1 - fg, fg], 0)[None].astype(np.float32)
    dl = r.normal(0, 0.3, (1, 12, 9, 9)).astype(np.float32)
    ii = np.array([[72, 72, 1.0]], dtype=np.float32)
    b, p = run_proposal(sc, dl, ii)
    prop.update(ties_scores=sc, ties_deltas=dl, ties_im_info=ii, ties_boxes=b, ties_probs=p)
    np.savez_compressed(os.path.join(OUT, "proposal.npz"), **prop)

    # ---------------- ProposalLayer.forward under other param strings --------
    # per geometry: TEST.ANCHOR_MIN_SIZE 0 and GEOMETRY_MIN_SIZE on the same inputs, an unpadded image a few pixels below
    # h * feat_stride[0], im_info scale 1.5.  The seed is the first one for which no side of any box lies within 0.01 px
    # of min_size * scale (judged with the oracle's restatement, which the CPU test then holds to these vectors): the
    # kept set must not hinge on the last ulp of exp().
    import ast
    from oracle import oracle as O
    geo = {}
    gh, gw = GEOMETRY_MAP

    def geometry_inputs(pstr, seed, dstd):
        kw = ast.literal_eval(pstr)
        A = O.generate_anchors(kw.get("base_size", 16), kw["ratios"], kw["scales"], kw.get("shifts", [0]),
                               kw["feat_stride"]).shape[0]
        r = np.random.default_rng(seed)
        fg = r.uniform(0.001, 0.9, (A, gh, gw)).astype(np.float32)
        sc = np.concatenate([1 - fg, fg], 0)[None].astype(np.float32)
        dl = r.normal(0, dstd, (1, 4 * A, gh, gw)).astype(np.float32)
        s0 = kw["feat_stride"][0]
        ii = np.array([[gh * s0 - 3, gw * s0 - 5, GEOMETRY_SCALE]], dtype=np.float32)
        return kw, A, sc, dl, ii

    def sides_clear_of_cut(kw, sc, dl, ii):
        b, _ = O.proposal_forward(sc, dl, ii, O.ProposalParams(min_size=0, score_thresh=-1.0, pre_nms_topN=0, **kw))
        cut = GEOMETRY_MIN_SIZE * GEOMETRY_SCALE
        sides = np.concatenate([b[:, 3] - b[:, 1] + 1, b[:, 4] - b[:, 2] + 1])
        return np.abs(sides - cut).min() > 0.01

    def record(case, pstr, sc, dl, ii, min_size):
        old_ms = cfg.TEST.ANCHOR_MIN_SIZE
        cfg.TEST.ANCHOR_MIN_SIZE = min_size
        try:
            b, p = run_proposal(sc, dl, ii, pstr)
        finally:
            cfg.TEST.ANCHOR_MIN_SIZE = old_ms
        geo[case + "_scores"] = sc
        geo[case + "_deltas"] = dl
        geo[case + "_im_info"] = ii
        geo[case + "_min_size"] = np.array([min_size], np.float32)
        geo[case + "_boxes"] = b
        geo[case + "_probs"] = p
        geo[case + "_param_str"] = np.array(pstr)
        geo_cases.append(case)
        return b

    geo_cases = []
    for gi, (name, pstr) in enumerate(GEOMETRIES):
        seed = 100 * (gi + 1)
        while True:
            kw, A, sc, dl, ii = geometry_inputs(pstr, seed, 0.3 + 0.05 * gi)
            if sides_clear_of_cut(kw, sc, dl, ii):
                break
            seed += 1
        total = gh * gw * A
        n0 = len(record(name + "_ms0", pstr, sc, dl, ii, 0))
        n6 = len(record(name + "_ms%d" % GEOMETRY_MIN_SIZE, pstr, sc, dl, ii, GEOMETRY_MIN_SIZE))
        assert 0 < n6 < n0 <= total, (name, n6, n0, total)   # the cut removes some rows, not all
        print("proposal_geometry %s: seed %d, A %d, rows %d / %d of %d" % (name, seed, A, n0, n6, total))
    # the overflow / clamp branch on non-square anchors (np.seterr(over='raise'), bbox_transform.py:9,52-65):
    #   _overflow          dw = 130 on the 22x12 anchor: exp() itself overflows fp32
    #   _overflow_product  dw = 85.9 there: exp(85.9) is finite, times the WIDTH 22 it overflows, times the height 12 it
    #                      would not (ln FLT_MAX = 88.72 < 85.9 + ln 22 = 88.99, > 85.9 + ln 12 = 88.38)
    #   _big_finite        dh = 85.9 there: against the height 12 nothing overflows and nothing is clamped
    # each with a second delta above 50 that is clamped only when the flag is raised, under an im_info of 6000 x 8000 px:
    # a clamped side is exp(5) * 24 = 3562 px and ends inside that image, an unclamped one ends at its border
    name, pstr = GEOMETRIES[0]
    for tag, row, val in (("overflow", 2, 130.0), ("overflow_product", 2, 85.9), ("big_finite", 3, 85.9)):
        kw, A, sc, dl, ii = geometry_inputs(pstr, 77, 0.3)
        ii[0, :2] = (6000, 8000)
        dl[0, row, 2, 4] = val          # anchor 0 (22 wide, 12 high), rows 4 a + (dx, dy, dw, dh)
        dl[0, 4 * 2 + 3, 4, 2] = 60.0   # dh of anchor 2 at a cell its sub-stride 2 keeps
        record(name + "_" + tag, pstr, sc, dl, ii, 0)
    geo["cases"] = np.array(geo_cases)
    np.savez_compressed(os.path.join(OUT, "proposal_geometry.npz"), **geo)

    # ---------------- bbox_vote / py_cpu_nms ---------------------------
    vn = {}
    rng = np.random.default_rng(21)
    sets = {
        "empty": np.zeros((0, 5), np.float32),
        "single": np.array([[10, 20, 50, 80, 0.9]], np.float32),
        "two_overlap": np.array([[10, 10, 50, 50, 0.9], [12, 12, 52, 52, 0.8]], np.float32),
        "singletons": np.array([[i * 100, 0, i * 100 + 30, 30, 0.5 + 0.01 * i] for i in range(7)], np.float32),
        "last_singleton": np.array([[0, 0, 40, 40, 0.9], [1, 1, 41, 41, 0.8], [300, 300, 340, 340, 0.1]], np.float32),
        "clusters_small": clustered_dets(rng, 12, 6, 0.08),
        "clusters_mid": clustered_dets(rng, 120, 10, 0.10),
        "clusters_big": clustered_dets(rng, 400, 16, 0.12, extent=1400.0),
        "ties": clustered_dets(rng, 40, 8, 0.08, quant=16),
        "dense": clustered_dets(rng, 30, 40, 0.25, size=(60, 200), extent=400.0),
    }
    # IoU exactly == 0.4 : a=(0,0,9,9) area 100 ; b=(0,0,9,3)?? build exactly:
    # a = 10x10 (area 100), b = 10x4 inside a shifted: inter=40, union=100 -> 0.4
    sets["iou_exact_0p4"] = np.array([[0, 0, 9, 9, 0.9], [0, 0, 9, 3, 0.8],
                                      [100, 100, 109, 109, 0.7], [100, 100, 109, 103, 0.95]], np.float32)
    for k, d in sets.items():
        vn[k + "_dets"] = d
        # the permutation both bbox_vote (test.py:182) and py_cpu_nms (:18) start from;
        # tie order is implementation-defined, so it is recorded for exact replay
        vn[k + "_order"] = d[:, 4].ravel().argsort()[::-1].astype(np.int64)
        vn[k + "_vote"] = np.asarray(ref_test.bbox_vote(d.copy()), dtype=np.float64)
        for thr in (0.4, 0.3, 0.7):
            keep = py_cpu_nms(d.copy(), thr) if d.shape[0] else []
            vn[k + "_nms_%02d" % int(thr * 100)] = np.asarray(keep, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "vote_nms.npz"), **vn)

    # ---------------- forward_net (flip/unscale/tile) ------------------
    fw = {}
    for i, (h, w, s, flip) in enumerate([(100, 100, 0.09765625, False), (150, 301, 0.29296875, True),
                                         (64, 80, 1.0, True), (37, 53, 1.37, False)]):
        net = FakeNet(100 + i)
        blob = {"data": np.random.default_rng(i).normal(0, 50, (1, 3, h, w)).astype(np.float32)}
        probs, boxes = ref_test.forward_net(net, blob, s, pyramid=True, flip=flip)
        fw["c%d_args" % i] = np.array([h, w, s, float(flip)])
        fw["c%d_seed" % i] = np.array([100 + i])
        fw["c%d_probs" % i] = probs[0]
        fw["c%d_boxes" % i] = boxes[0]
        fw["c%d_fed_shape" % i] = np.array(net.calls[0][0])
        fw["c%d_fed_im_info" % i] = net.calls[0][1]
        fw["c%d_raw_boxes_after" % i] = net.blobs["boxes"].data.copy()
    np.savez_compressed(os.path.join(OUT, "forward_net.npz"), **fw)

    # ---------------- pyramid scales ------------------------------------
    ps = {}
    for shape in [(1024, 1024, 3), (768, 1024, 3), (2000, 300, 3), (50, 50, 3), (683, 1024, 3), (1365, 1024, 3)]:
        base = _compute_scaling_factor(shape, cfg.TEST.PYRAMID_BASE_SIZE[0], cfg.TEST.PYRAMID_BASE_SIZE[1])
        sc = [float(s) / cfg.TEST.PYRAMID_BASE_SIZE[0] * base for s in cfg.TEST.SCALES]
        ps["%dx%d" % shape[:2]] = np.array([base] + sc, dtype=np.float64)
    np.savez(os.path.join(OUT, "pyramid_scales.npz"), **ps)

    # ---------------- detect() orchestration with a fake net ------------
    det = {}
    for i, (H, W) in enumerate([(96, 128), (200, 150)]):
        im = np.random.default_rng(500 + i).integers(0, 256, (H, W, 3)).astype(np.uint8)
        fake_cv2._images["img%d.jpg" % i] = im
        net = FakeNet(900 + i)
        cls_dets, _ = ref_test.detect(net, "img%d.jpg" % i, thresh=0.05, pyramid=True)
        det["i%d_image" % i] = im
        det["i%d_seed" % i] = np.array([900 + i])
        det["i%d_dets" % i] = np.asarray(cls_dets[0], dtype=np.float64)
        det["i%d_fed_shapes" % i] = np.array([c[0] for c in net.calls])
        det["i%d_fed_im_info" % i] = np.concatenate([c[1] for c in net.calls])
        det["i%d_fed_sum" % i] = np.array([c[2] for c in net.calls])
        det["i%d_fed_first" % i] = np.array([c[3] for c in net.calls])
    np.savez_compressed(os.path.join(OUT, "detect.npz"), **det)

    # ---------------- write_detections line format ----------------------
    # lib/datasets/wider.py:160-167 -- the consumer that defines "0-pixel diff".
    rows = np.array([[10.9, 20.2, 50.99, 80.5, 0.987654321], [0.0, 0.4, 3.6, 2.2, 1e-4],
                     [123.5, 7.75, 400.25, 300.0, 0.05000001]], dtype=np.float64)
    lines = ['%d %d %d %d %g \n' % (int(d[0]), int(d[1]), int(d[2]) - int(d[0]),
                                    int(d[3]) - int(d[1]), d[4]) for d in rows]
    # produced with the same expression as the reference's writer; kept as a
    # format pin (the wider imdb class itself needs datasets on disk to construct)
    json.dump({"rows": rows.tolist(), "lines": lines},
              open(os.path.join(OUT, "write_detections.json"), "w"), indent=1)

    # ---------------- detection writers of the four imdbs ------------------
    # lib/datasets/{wider,fddb,afw,pascalface}.py write_detections, called unbound on a stand-in `self` (the
    # constructors need the datasets on disk); the files they write are stored as text.
    import datasets.wider as ref_wider
    import datasets.fddb as ref_fddb
    import datasets.afw as ref_afw
    import datasets.pascalface as ref_pascal
    rngw = np.random.default_rng(77)
    wpaths = ["0--Parade/0_Parade_marchingband_1_5.jpg", "1--Handshaking/1_Handshaking_Handshaking_1_35.jpg",
              "2--Demonstration/2_Demonstration_Political_Rally_2_9.jpg"]
    wboxes = []
    for n in (4, 0, 7):
        xy = rngw.uniform(0, 600, (n, 2))
        wh = rngw.uniform(3, 200, (n, 2))
        sc = rngw.uniform(0.05, 1.0, (n, 1))
        wboxes.append(np.hstack([xy, xy + wh, sc]))
    all_boxes = [[[] for _ in wpaths], wboxes]
    written = {}
    for key, mod, cls in (("wider", ref_wider, "wider"), ("fddb", ref_fddb, "fddb"), ("afw", ref_afw, "afw"),
                          ("pascal", ref_pascal, "pascalface")):
        outd = os.path.join(tmp, "written_" + key)
        os.makedirs(outd)
        fake_self = types.SimpleNamespace(_image_paths=list(wpaths))
        klass = getattr(mod, cls)
        (klass.write_detections_rect if key == "fddb" else klass.write_detections)(fake_self, all_boxes, outd)
        files = {}
        for root, _, fns in os.walk(outd):
            for fn in fns:
                files[os.path.relpath(os.path.join(root, fn), outd)] = open(os.path.join(root, fn)).read()
        written[key] = files
    json.dump({"image_paths": wpaths, "boxes": [b.tolist() for b in wboxes], "written": written},
              open(os.path.join(OUT, "writers.json"), "w"), indent=1, sort_keys=True)

    # ---------------- WIDER evaluator --------------------------------------
    # lib/wider_eval_tools/wider_eval.py on a synthetic ground truth in the official toolbox's .mat layout
    # (61 events -- the evaluator hard-codes that number -- two images each) and synthetic detection files.
    from scipy import io as sio
    import wider_eval_tools.wider_eval as ref_eval
    rnge = np.random.default_rng(2024)
    gt_dir = os.path.join(tmp, "ground_truth")
    pred_dir = os.path.join(tmp, "pred")
    os.makedirs(gt_dir)
    n_ev, per_ev = 61, 2
    ev_names, file_names, gt_boxes, subsets, preds = [], [], [], {"easy": [], "medium": [], "hard": []}, []
    for e in range(n_ev):
        ev = "%d--Event%d" % (e, e)
        ev_names.append(ev)
        os.makedirs(os.path.join(pred_dir, ev))
        for j in range(per_ev):
            name = "%d_Event%d_img_%d" % (e, e, j)
            file_names.append(name)
            g = int(rnge.integers(0, 6))
            xy = rnge.uniform(0, 400, (g, 2))
            wh = rnge.uniform(8, 120, (g, 2))
            gb = np.round(np.hstack([xy, wh]))
            gt_boxes.append(gb)
            big = np.where(wh.min(axis=1) > 60)[0] if g else np.zeros(0, int)
            mid = np.where(wh.min(axis=1) > 25)[0] if g else np.zeros(0, int)
            subsets["easy"].append(big + 1)
            subsets["medium"].append(mid + 1)
            subsets["hard"].append(np.arange(g) + 1)
            # detections: jittered copies of some faces (a few duplicates on one face), plus clutter
            rows = []
            for k in range(g):
                for _ in range(int(rnge.integers(0, 3))):
                    jit = rnge.normal(0, 0.12, 4) * np.array([gb[k, 2], gb[k, 3], gb[k, 2], gb[k, 3]])
                    rows.append(np.concatenate([gb[k] + jit, [rnge.uniform(0.3, 1.0)]]))
            for _ in range(int(rnge.integers(0, 4))):
                rows.append(np.concatenate([rnge.uniform(0, 400, 2), rnge.uniform(8, 120, 2), [rnge.uniform(0.05, 0.6)]]))
            if e == 7 and j == 1:
                rows = []      # an image without detections
            pr = np.array(rows, dtype=np.float64).reshape(-1, 5)
            pr[:, 2:4] = np.maximum(pr[:, 2:4], 2.0)
            pr[:, 4] = np.round(pr[:, 4], 4) + 1e-6 * np.arange(len(pr))     # distinct scores: no tie-order ambiguity
            with open(os.path.join(pred_dir, ev, name + ".txt"), "w") as f:
                f.write("%s/%s.jpg\n%d\n" % (ev, name, len(pr)))
                for r in pr:
                    f.write("%d %d %d %d %g \n" % (int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[4]))
            # what the evaluator parses back from that text
            preds.append(np.array([[float(v) for v in ("%d %d %d %d %g" % (int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[4])).split()]
                                   for r in pr], dtype=np.float64).reshape(-1, 5))

    def cell(rows):       # MATLAB cell column
        c = np.empty((len(rows), 1), dtype=object)
        for i, r in enumerate(rows):
            c[i, 0] = r
        return c

    def mat_for(subset):
        fl, bl, gl = [], [], []
        for e in range(n_ev):
            sl = slice(e * per_ev, (e + 1) * per_ev)
            fl.append(cell([np.array([nm], dtype=object).reshape(1, 1) if False else nm for nm in file_names[sl]]))
            bl.append(cell([gt_boxes[i] for i in range(sl.start, sl.stop)]))
            gl.append(cell([np.asarray(subset[i], dtype=np.int32).reshape(-1, 1) for i in range(sl.start, sl.stop)]))
        return {"event_list": cell(ev_names), "file_list": cell(fl), "face_bbx_list": cell(bl), "gt_list": cell(gl)}

    sio.savemat(os.path.join(gt_dir, "wider_face_val.mat"), mat_for(subsets["hard"]))
    for sname in ("easy", "medium", "hard"):
        sio.savemat(os.path.join(gt_dir, "wider_%s_val.mat" % sname), mat_for(subsets[sname]))
    ev_out = {}
    for bug in (True, False):
        ap, pr_curve = ref_eval.wider_eval(pred_dir, gt_dir, parallel=False, mimic_eval_bug=bug, IoU_thresh=0.5)
        ev_out["ap_bug%d" % int(bug)] = np.array(ap, dtype=np.float64)
        ev_out["pr_bug%d" % int(bug)] = np.array(pr_curve, dtype=np.float64)
    ev_out["n_images"] = np.array([len(file_names)])
    ev_out["gt_count"] = np.array([len(b) for b in gt_boxes])
    ev_out["gt_boxes"] = np.concatenate([b.reshape(-1, 4) for b in gt_boxes])
    for sname in ("easy", "medium", "hard"):
        ev_out["sub_%s_count" % sname] = np.array([len(v) for v in subsets[sname]])
        ev_out["sub_%s" % sname] = np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v in subsets[sname]])
    ev_out["pred_count"] = np.array([len(p_) for p_ in preds])
    ev_out["preds"] = np.concatenate([p_.reshape(-1, 5) for p_ in preds])
    np.savez_compressed(os.path.join(OUT, "wider_eval.npz"), **ev_out)
    json.dump({"events": ev_names, "files": file_names}, open(os.path.join(OUT, "wider_eval_names.json"), "w"))

    # ---------------- inference templates: structural digest -------------
    # models/test_template.prototxt and models/test_different_dilation_template.prototxt parsed with the
    # runtime's own text-format parser and reduced to a canonical dump; only its SHA-256 and a few counts
    # are committed (the product generates the templates itself, prototxt.build_test_template).
    import hashlib
    from smallhardface_amd import prototxt as P
    tdig = {}
    for key, fn in (("plain", "test_template.prototxt"), ("different_dilation", "test_different_dilation_template.prototxt")):
        msg = P.parse(open(os.path.join(REF, "models", fn)).read())
        canon = P.dumps(msg)
        layers = msg.getall("layer")
        tdig[key] = {"sha256": hashlib.sha256(canon.encode()).hexdigest(), "n_layers": len(layers),
                     "n_chars": len(canon)}
    json.dump(tdig, open(os.path.join(OUT, "template_digest.json"), "w"), indent=1, sort_keys=True)

    shutil.rmtree(tmp, ignore_errors=True)
    print("golden fixtures written to", OUT)


if __name__ == "__main__":
    main()
