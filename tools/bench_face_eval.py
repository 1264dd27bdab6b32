"""Host against device AFW / Pascal Faces evaluation: the two fixtures and one seeded SYNTHETIC set.

    python tools/bench_face_eval.py [--out profiles/face_eval_device.json]

Runs ``face_eval.evaluate`` (5 refinement rounds) on the SAME arrays with the matching on the host and on the device
(``shf_face_eval_match``), for the filtered detections of tests/golden/face_eval.npz (AFW, Pascal Faces) and for
``tests/face_eval_cases.large_set``: 38 412 rows over 851 images, the size of the reference's largest Pascal dump.  Per
set: the best and the median of five runs after one warm-up call, end to end and for one matching round alone; asserts that
AP and precision are identical bit for bit.  Needs a GPU: there is no fallback.
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

from smallhardface_amd import face_eval as F  # noqa: E402
from tests import face_eval_cases as K  # noqa: E402


def best(fn, n):
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return dict(min_ms=1e3 * min(ts), median_ms=1e3 * float(np.median(ts)), runs=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_eval_device.json"))
    args = ap.parse_args()
    cases = {}
    for ds in K.DATASETS:
        _, dets, gt, _ = K.golden_case(ds)
        cases["fixture_" + ds] = (F.filter_detections(dets, F.min_pixels(30, 30)), gt)
    cases["large_38412x851"] = K.large_set()
    out = {}
    for name, (dets, gt) in cases.items():
        rec = dict(rows=len(dets), images=len(gt), boxes=int(sum(len(b) for b in gt.boxes)))
        rec["host"] = best(lambda: F.evaluate(dets, gt, iters=5), 5)
        F.evaluate(dets, gt, iters=5, device=True)          # first call: library load, context
        rec["device"] = best(lambda: F.evaluate(dets, gt, iters=5, device=True), 5)
        ordered = dets.sorted_by_score()
        flat = F.group_by_image(ordered, gt)
        d4 = np.ascontiguousarray(ordered.rows[flat["perm"], 1:5])
        rec["host_match_call"] = best(lambda: F.match_host(d4, flat, 0.5), 5)
        rec["device_match_call"] = best(lambda: F.match_device(d4, flat, 0.5), 10)
        a, b = F.evaluate(dets, gt, iters=5, device=True), F.evaluate(dets, gt, iters=5)
        assert a[0] == b[0] and np.array_equal(a[2], b[2], equal_nan=True)
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
