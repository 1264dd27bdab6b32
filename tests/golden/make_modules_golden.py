#!/usr/bin/env python3
"""Generate tests/golden/forward_net_levels.npz from the REFERENCE's own forward_net(pyramid=True) over a net with several
proposal layers: the branch of lib/test.py:67-83 that collects ``boxes_<level>`` / ``cls_prob_<level>`` per level.

Run in the authoring container only (needs the reference checkout make_golden.py names):

    python tests/golden/make_modules_golden.py [OUTDIR]

Like make_golden.py (whose conversion, stubs and FakeBlob it imports unchanged): the reference's lib/ is converted to py3
in a scratch TEMP dir; nothing of the reference is written into this repository, the fixture is DATA only.

Reference entry point exercised:
  lib/test.py:21    forward_net: im_info and the pad to MAX_RESOLUTION (:30-38), the flip fix over every output whose name
                    starts with ``boxes`` (:52-54), the level list from the blob names or TEST.LEVEL (:67-75), per level the
                    unscale and the tiling per class (:76-83)

A stand-in net with the blobs data, im_info, boxes_1, cls_prob_1, boxes_2, cls_prob_2 (in this order) returns canned rows;
three calls on a (1, 3, 21, 30) level at scale 1.5: plain, flipped, and plain with TEST.LEVEL = ['2'].  Stored: the canned
rows, the level's shape and scale, the shape forward() was fed, and per call the probs / pred_boxes lists.
"""
import os
import shutil
import sys
import tempfile
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import FakeBlob, convert_reference, install_stubs  # noqa: E402

OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
LEVEL_SHAPE, SCALE, ROWS = (1, 3, 21, 30), 1.5, {"1": 7, "2": 4}


def canned_rows(seed=640):
    """Per level (R, 5) boxes inside the 21 x 30 level and (R, 2) scores, float32."""
    rng = np.random.default_rng(seed)
    out = {}
    for lv, n in ROWS.items():
        x1, y1 = rng.uniform(0, 18, n), rng.uniform(0, 12, n)
        b = np.stack([np.zeros(n), x1, y1, x1 + rng.uniform(2, 11, n), y1 + rng.uniform(2, 8, n)], 1).astype(np.float32)
        fg = np.sort(rng.uniform(0.01, 0.99, n))[::-1]
        out[lv] = (b, np.stack([1 - fg, fg], 1).astype(np.float32))
    return out


class LevelsNet(object):
    """The stand-in: canned rows per level, fresh copies at every forward (the driver's flip fix writes into them)."""

    def __init__(self, rows):
        self.rows = rows
        self.blobs = OrderedDict([("data", FakeBlob(np.zeros((1, 3, 16, 16)))), ("im_info", FakeBlob(np.zeros((1, 3))))])
        for lv in rows:
            self.blobs["boxes_" + lv] = FakeBlob(np.zeros((1, 5)))
            self.blobs["cls_prob_" + lv] = FakeBlob(np.zeros((1, 2)))
        self.fed = []

    def forward(self, data=None, im_info=None):
        self.fed.append((tuple(data.shape), np.array(im_info)))
        out = {}
        for lv, (b, p) in self.rows.items():
            self.blobs["boxes_" + lv].data = b.copy()
            self.blobs["cls_prob_" + lv].data = p.copy()
            out["boxes_" + lv] = self.blobs["boxes_" + lv].data
            out["cls_prob_" + lv] = self.blobs["cls_prob_" + lv].data
        return out


def main():
    import numpy.ma  # noqa: F401  (before the np.bool alias of install_stubs)
    import scipy.io  # noqa: F401
    tmp = tempfile.mkdtemp(prefix="shf_ref_py3_")
    convert_reference(tmp)
    fake_cv2 = types.ModuleType("cv2")
    fake_cv2.INTER_LINEAR = 1
    install_stubs(fake_cv2)
    os.chdir(tmp)
    sys.path.insert(0, tmp)
    sys.path.insert(0, os.path.join(tmp, "lib"))
    from utils.get_config import cfg, cfg_from_file, cfg_from_list
    cfg_from_file("configs/smallhardface.toml")
    cfg_from_list(["TEST.MODEL", "dummy.caffemodel", "TEST.GPU_ID", "[0]"])
    import test as ref_test

    rows = canned_rows()
    fx = {"level_shape": np.array(LEVEL_SHAPE), "scale": np.array([SCALE]), "max_resolution": np.array([int(cfg.MAX_RESOLUTION)]),
          "levels": np.array(list(rows))}
    for lv, (b, p) in rows.items():
        fx["rows_boxes_" + lv], fx["rows_probs_" + lv] = b, p
    level = np.random.default_rng(641).normal(0, 50, LEVEL_SHAPE).astype(np.float32)
    for case, flip, subset in (("plain", False, []), ("flip", True, []), ("level2", False, ["2"])):
        cfg.TEST.LEVEL = subset
        net = LevelsNet(rows)
        blob = {"data": level[..., ::-1] if flip else level}
        probs, boxes = ref_test.forward_net(net, blob, SCALE, pyramid=True, flip=flip)
        probs, boxes = list(probs), list(boxes)
        assert len(probs) == len(boxes) == (1 if subset else 2) and len(net.fed) == 1
        fx[case + "_n"] = np.array([len(probs)])
        fx[case + "_fed_shape"] = np.array(net.fed[0][0])
        fx[case + "_fed_im_info"] = net.fed[0][1]
        for j, (p, b) in enumerate(zip(probs, boxes)):
            fx["%s_probs%d" % (case, j)], fx["%s_boxes%d" % (case, j)] = np.array(p), np.array(b)
        print("forward_net_levels %-7s %d level(s), fed %s" % (case, len(probs), net.fed[0][0]))
    cfg.TEST.LEVEL = []
    path = os.path.join(OUT, "forward_net_levels.npz")
    np.savez_compressed(path, **fx)
    shutil.rmtree(tmp, ignore_errors=True)
    print("forward_net_levels.npz written to", OUT, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
