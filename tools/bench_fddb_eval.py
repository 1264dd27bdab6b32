"""Host against device FDDB evaluation on one seeded SYNTHETIC set of FDDB's size.

    python tools/bench_fddb_eval.py [--out profiles/fddb_eval_device.json]

``tests/fddb_eval_cases.fddb_sized_set``: 2 845 images of 300..450 pixels a side, 5 171 ellipses, 20..89 detections per image
drawn around and away from them.  Runs ``fddb_eval.evaluate`` on the SAME structures with the pixel counts on the host and
on the device (``shf_fddb_pair_counts``): the device once cold (the first call of the process: library load, context) and
five times warm, the host once; then the parts of one warm device run -- shared geometry, the call (its uploads, kernels
and read-back from stream events), and the host remainder (scores, assignment, curves).  Asserts that every integer array
and every curve value is identical.  Needs a GPU: there is no fallback.
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

from smallhardface_amd import fddb_eval as F  # noqa: E402
from tests import fddb_eval_cases as K  # noqa: E402
from tools.kernel_hash import kernel_source_hash  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fddb_eval_device.json"))
    ap.add_argument("--images", type=int, default=2845)
    ap.add_argument("--faces", type=int, default=5171)
    ap.add_argument("--seed", type=int, default=2845)
    a = ap.parse_args()

    from smallhardface_amd import _lib
    _lib.load()                                       # raises without a GPU, before the host run
    dets, gt, sizes = K.fddb_sized_set(a.seed, a.images, a.faces)
    dev_cold, t_cold = timed(lambda: F.evaluate(dets, gt, sizes=sizes, device=True))
    warm = [timed(lambda: F.evaluate(dets, gt, sizes=sizes, device=True)) for _ in range(5)]
    t_warm = [t for _, t in warm]
    dev = warm[-1][0]
    host, t_host = timed(lambda: F.evaluate(dets, gt, sizes=sizes))
    for k in ("inter", "ann_area", "det_area", "m", "disc", "cont"):
        assert np.array_equal(dev[k], host[k]) and np.array_equal(dev_cold[k], host[k]), "%s: device and host differ" % k

    # the parts of one warm device run, and of the host run
    geom, t_geom = timed(lambda: F.geometry(F.align(dets, gt), gt, sizes))
    phase_ms = np.zeros(3)
    _, t_call = timed(lambda: F.pair_counts_device(geom, phase_ms))
    _, t_host_counts = timed(lambda: F.pair_counts_host(geom))
    t_dev = sorted(t_warm)[len(t_warm) // 2]
    box = geom["ell_box"]
    res = {
        "what": "FDDB evaluation (pixel counts of every annotation x detection pair, assignment, both ROC curves) of a seeded "
                "synthetic set: host numpy against the device path on the same structures, one process",
        "synthetic": True,
        "kernel_source_hash": kernel_source_hash(),
        "eval_source_hash": kernel_source_hash(["eval.hip", "eval.h"]),          # (the evaluation kernels alone)
        "generator": {"images": a.images, "faces": int(geom["ann_off"][-1]), "detections": int(geom["det_off"][-1]),
                      "pairs": int(F.pair_offsets(geom)[-1]), "seed": a.seed,
                      "scan_box_pixels_mean": float(np.mean((box[:, 2] - box[:, 0] + 1) * (box[:, 3] - box[:, 1] + 1)))},
        "host_s": round(t_host, 3),
        "device_s": round(t_dev, 3),
        "device_warm_runs_s": [round(t, 4) for t in t_warm],
        "device_first_call_s": round(t_cold, 3),
        "device_parts_s": {"geometry": round(t_geom, 4), "shf_fddb_pair_counts": round(t_call, 4),
                           "upload": round(phase_ms[0] / 1e3, 5), "kernels": round(phase_ms[1] / 1e3, 5),
                           "read_back": round(phase_ms[2] / 1e3, 5),
                           "host_remainder": round(t_dev - t_geom - t_call, 4)},
        "host_parts_s": {"geometry": round(t_geom, 4), "pair_counts_host": round(t_host_counts, 4),
                         "host_remainder": round(t_host - t_geom - t_host_counts, 4)},
        "results_identical": True,
        "disc_at_1000": host["disc_at_1000"], "cont_at_1000": host["cont_at_1000"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
