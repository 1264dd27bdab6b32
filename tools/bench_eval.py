"""Host against device WIDER evaluation on a seeded SYNTHETIC set of WIDER-val size.

    python tools/bench_eval.py [--images 3226] [--gt-max 23] [--dets 300] [--seed 0] [--out profiles/wider_eval_device.json]

Builds per image 1..gt-max ground-truth faces (easy within medium within hard subsets, by face size) and about --dets
detections (jittered copies of the faces plus background boxes, random scores), then runs on the SAME arrays
  host    evaluate_setting x 3 (smallhardface_amd/wider_eval.py, the unchanged numpy evaluator), and
  device  flatten + shf_wider_eval_counts (uploads, kernels, read-back) + the final divisions -- once cold (the first HIP
          call of the process, runtime start-up included) and five times warm (the median is reported),
asserts that the three PR curves are identical bit for bit, and writes one JSON with both times and the generator
parameters.  Sorting and score normalisation are common to both paths and timed apart.  Needs a GPU: there is no fallback.
The detection counts of a trained model on the real WIDER images are not known here; the set is synthetic.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from smallhardface_amd import wider_eval as W  # noqa: E402


def synthetic_set(n_images, gt_max, dets, seed):
    rng = np.random.default_rng(seed)
    preds, boxes, keeps = [], [], [[], [], []]
    for _ in range(n_images):
        g = int(rng.integers(1, gt_max + 1))
        wh = np.rint(rng.uniform(6, 200, (g, 2)))
        gt = np.hstack([np.rint(rng.uniform(0, 1000, (g, 2))), wh])
        size = wh.min(axis=1)
        for s, lim in enumerate((50, 25, 0)):        # easy: large faces, medium: + mid-sized, hard: all
            keeps[s].append(np.flatnonzero(size >= lim))
        n = int(rng.integers(max(dets // 2, 1), dets + dets // 2 + 1))
        n_fg = min(n, int(rng.integers(g, 4 * g + 1)))
        src = rng.integers(0, g, n_fg)
        fg = gt[src] + rng.normal(0, 0.12, (n_fg, 4)) * gt[src][:, [2, 3, 2, 3]]
        bg = np.hstack([rng.uniform(0, 1000, (n - n_fg, 2)), rng.uniform(4, 120, (n - n_fg, 2))])
        score = np.concatenate([rng.beta(4, 2, n_fg), rng.beta(1, 6, n - n_fg)])
        preds.append(np.hstack([np.vstack([fg, bg]), score[:, None]]))
        boxes.append(gt)
    ev = ["e"] * n_images
    names = ["%d" % i for i in range(n_images)]
    return preds, [W.WiderGT(ev, names, boxes, k) for k in keeps]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3226)
    ap.add_argument("--gt-max", type=int, default=23)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--iou", type=float, default=0.5)
    ap.add_argument("--no-mimic-eval-bug", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="time the device path alone and write no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wider_eval_device.json"))
    a = ap.parse_args()
    bug = not a.no_mimic_eval_bug

    from smallhardface_amd import _lib
    _lib.load()                                       # raises without a GPU, before the long host run
    preds, gts = synthetic_set(a.images, a.gt_max, a.dets, a.seed)
    t0 = time.perf_counter()
    norm = W.normalise_scores([W.sort_by_score(p) for p in preds])
    t_common = time.perf_counter() - t0

    t0 = time.perf_counter()
    dev_cold = W._device_curves(norm, gts, a.iou, bug)
    t_dev_cold = time.perf_counter() - t0
    t_warm = []
    for _ in range(5):
        t0 = time.perf_counter()
        dev = W._device_curves(norm, gts, a.iou, bug)
        t_warm.append(time.perf_counter() - t0)
    t_dev = sorted(t_warm)[len(t_warm) // 2]
    t0 = time.perf_counter()
    flat = W.flatten_inputs(norm, gts[0].boxes, [g.keep for g in gts])
    t_flatten = time.perf_counter() - t0
    t0 = time.perf_counter()
    W.device_counts(flat, a.iou, bug)
    t_call = time.perf_counter() - t0

    if a.device_only:                                 # (for a kernel trace: no host run, no file)
        print(json.dumps({"device_first_call_s": t_dev_cold, "device_warm_runs_s": t_warm, "flatten_s": t_flatten,
                          "shf_wider_eval_counts_s": t_call}))
        return
    t0 = time.perf_counter()
    host = [W.evaluate_setting(norm, g, a.iou, bug) for g in gts]
    t_host = time.perf_counter() - t0

    for s in range(3):
        assert np.array_equal(dev[s], host[s], equal_nan=True), "setting %d: device and host curves differ" % s
        assert np.array_equal(dev_cold[s], host[s], equal_nan=True), "setting %d: cold device curves differ" % s
    aps = [float(W.voc_ap(c[:, 1], c[:, 0])) for c in host]
    res = {
        "what": "WIDER evaluation (matching + threshold sweep, 3 settings) of a seeded synthetic set: host numpy against the "
                "device path on the same arrays, one process",
        "synthetic": True,
        "generator": {"images": a.images, "gt_per_image": [1, a.gt_max], "dets_per_image_mean": a.dets, "seed": a.seed,
                      "detections": int(sum(len(p) for p in preds)), "gt_boxes": int(sum(len(b) for b in gts[0].boxes)),
                      "iou_thresh": a.iou, "mimic_eval_bug": bug},
        "host_s": round(t_host, 3),
        "device_s": round(t_dev, 3),
        "device_warm_runs_s": [round(t, 4) for t in t_warm],
        "device_first_call_s": round(t_dev_cold, 3),
        "device_parts_s": {"flatten": round(t_flatten, 3), "shf_wider_eval_counts": round(t_call, 3)},
        "sort_and_normalise_s": round(t_common, 3),
        "curves_identical": True,
        "ap": aps,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
