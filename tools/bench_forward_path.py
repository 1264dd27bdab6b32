"""The literal drop-in path with host levels, with device-resident levels, and with the units of an image as one grouped
forward, side by side.

    python tools/bench_forward_path.py                       # -> profiles/forward_grouped.json
    python tools/bench_forward_path.py --parent-json P.json  # ... with the parent commit's figures merged in

Runs ``test.detect(net, im=...)`` -- lib/test.py:109-178: five pyramid levels, ten ``forward_net`` / ``Net.forward()`` calls,
the > 0.05 cut and bbox_vote -- on bench.py's C5 image (1024 x 1024 uint8, seed 1000, the ``configs/smallhardface.toml``
pyramid with flip, synthetic weights seed 1234, conv mode f16x3) with ``SHF_DEVICE_LEVELS`` unset ("switch_off": the levels
come back to the host, are padded / flipped into the blob's pinned mirror and uploaded) and set to 1 ("switch_on": the levels
stay in HBM as caffe.DeviceArray and Blob.load_device pads / flips them on the device), and with ``SHF_GROUPED_FORWARD=1`` on top
of that ("grouped": one grouped load and ONE ``Net.forward_group`` over the ten units instead of ten loads and ten forwards).
After a warm-up each leg is timed
``--repeats`` times over ``--images`` images, the legs alternating inside one process; a repeat is a host clock around
whole detect() calls, each of which ends in synchronous read-backs.  Per leg: milliseconds per image of every repeat, their
median and spread (max - min), the ``Net.timing`` breakdown per image, and -- from one more, untimed image per leg with every
launch bracketed -- the profiler's kernel / h2d / d2h milliseconds per image.

With the switch off only interfaces older than the switch are used, so the same file runs on a tree without the feature
(it then measures the legs that tree has): run it there once and hand the result in with ``--parent-json``; its legs are
recorded under "parent_commit" next to this tree's.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10, help="images per repeat (at least 10)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed images per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_grouped.json"))
    ap.add_argument("--parent-json", default=None, help="this tool's output on the parent commit: merged in as parent_commit")
    args = ap.parse_args()
    n_img, n_rep = max(10, args.images), max(3, args.repeats)

    from smallhardface_amd import caffe, prototxt as P, weights
    from smallhardface_amd import test as T
    from smallhardface_amd.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(ROOT, "configs", "smallhardface.toml"))
    caffe.set_mode_gpu()
    caffe.set_device(0)
    msg = P._add_dimension_reduction(P.build_test_template(True))
    net = caffe.Net(None, prototxt_text=P.dumps(msg))
    for name, blobs in weights.synth_params(msg, seed=1234).items():
        for i, arr in enumerate(blobs):
            net.params[name][i].data[...] = arr
    net.commit_params()
    net.set_conv_mode("f16x3")
    im = np.random.default_rng(1000).integers(0, 256, (1024, 1024, 3)).astype(np.uint8)

    legs = ["switch_off"] + (["switch_on"] if hasattr(caffe, "DeviceArray") else []) + \
           (["grouped"] if hasattr(caffe.Net, "forward_group") else [])
    os.environ.pop("SHF_HOST_PREPROCESS", None)
    n_units = len(cfg.TEST.SCALES) * (2 if cfg.TEST.FLIP else 1)

    def select(leg):
        for k, on in (("SHF_DEVICE_LEVELS", leg in ("switch_on", "grouped")), ("SHF_GROUPED_FORWARD", leg == "grouped")):
            if on:
                os.environ[k] = "1"
            else:
                os.environ.pop(k, None)

    dets = {}
    for leg in legs:
        select(leg)
        for _ in range(max(1, args.warmup)):
            dets[leg] = np.asarray(T.detect(net, None, 0.05, pyramid=True, im=im)[0][0], dtype=np.float64)
    res = {leg: {"repeats_ms_per_image": [], "timing_ms_per_image": []} for leg in legs}
    for _ in range(n_rep):
        for leg in legs:                       # alternating: both legs see the same neighbours on a shared host
            select(leg)
            net.sync()
            net.timing = {}
            t0 = time.perf_counter()
            for _i in range(n_img):
                T.detect(net, None, 0.05, pyramid=True, im=im)
            dt = time.perf_counter() - t0
            tm, net.timing = net.timing, None
            res[leg]["repeats_ms_per_image"].append(1000.0 * dt / n_img)
            res[leg]["timing_ms_per_image"].append({k[:-2] + "_ms": 1000.0 * v / n_img for k, v in tm.items() if k.endswith("_s")})
            assert tm.get("units" if leg == "grouped" else "calls", 0) == n_img * n_units
            res[leg]["forward_calls_per_image"] = tm.get("calls", 0) / float(n_img)
    # the profiler's view of one more image per leg, outside the timed repeats (an event pair around every launch costs the
    # stream a few microseconds each): what the GPU spends in kernels and in copies
    for leg in legs:
        select(leg)
        net.prof_enable(True)
        net.prof_reset()
        T.detect(net, None, 0.05, pyramid=True, im=im)
        pr = net.prof_read()
        net.prof_enable(False)
        net.prof_reset()
        copies = {"h2d_copy": "h2d_ms", "d2h_copy": "d2h_ms"}
        prof = {"kernel_ms": float(sum(v["ms"] for k, v in pr.items() if k not in copies)),
                "kernel_launches": int(sum(v["launches"] for k, v in pr.items() if k not in copies))}
        for k, name in copies.items():
            prof[name] = float(pr[k]["ms"])
        res[leg]["profiler_per_image"] = prof
    select("switch_off")
    # forming the levels alone, outside the timed repeats (the call synchronises): switch off with their copy to the host
    from smallhardface_amd.test_utils import pyramid_scales
    level_blobs = T._get_image_blob_device    # (before the switch existed: test_utils' own, imported into test)
    for leg in legs:
        kw = {"on_device": True} if leg == "switch_on" else {}
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            level_blobs(im, pyramid_scales(im.shape), **kw)
            ts.append(1000.0 * (time.perf_counter() - t0))
        res[leg]["levels_ms"] = float(np.median(ts[2:]))
    for leg in legs:
        r = res[leg]
        v = r["repeats_ms_per_image"]
        r["ms_per_image"] = float(np.median(v))
        r["spread_ms"] = float(max(v) - min(v))
        keys = sorted(r["timing_ms_per_image"][0])
        r["timing_ms_per_image"] = {k: float(np.median([t[k] for t in r["timing_ms_per_image"]])) for k in keys}
        # what detect() spends outside Net.forward(): forming the levels (and, switch off, their D2H), the pad / flip on the host
        # or Blob.load_device, the box merge
        r["outside_forward_ms"] = r["ms_per_image"] - sum(v for k, v in r["timing_ms_per_image"].items() if k.endswith("_ms"))
        r["boxes"] = int(len(dets[leg]))
    out = {
        "workload": "test.detect(pyramid=True) on a 1024 x 1024 uint8 image (seed 1000), configs/smallhardface.toml pyramid "
                    "(scales %s, flip %s): %d Net.forward() per image, conv mode f16x3, synthetic weights seed 1234"
                    % (list(cfg.TEST.SCALES), bool(cfg.TEST.FLIP), len(cfg.TEST.SCALES) * (2 if cfg.TEST.FLIP else 1)),
        "images_per_repeat": n_img, "repeats": n_rep, "warmup_images_per_leg": max(1, args.warmup),
        "unit": "host milliseconds per image; spread = max - min over the repeats; timing = Net.timing per image",
    }
    out.update(res)
    if "switch_on" in res:
        off, on = res["switch_off"], res["switch_on"]
        out["identical_detections"] = bool(dets["switch_on"].shape == dets["switch_off"].shape and
                                           np.array_equal(dets["switch_on"], dets["switch_off"]))
        out["saving_ms"] = off["ms_per_image"] - on["ms_per_image"]
        out["saving_exceeds_spread"] = bool(out["saving_ms"] > max(off["spread_ms"], on["spread_ms"]))
    if "grouped" in res:
        on, gr = res["switch_on"], res["grouped"]
        out["identical_detections"] = bool(out["identical_detections"] and dets["grouped"].shape == dets["switch_off"].shape and
                                           np.array_equal(dets["grouped"], dets["switch_off"]))
        out["grouped_saving_ms"] = on["ms_per_image"] - gr["ms_per_image"]       # against the ungrouped device-levels leg
        out["grouped_saving_exceeds_spread"] = bool(out["grouped_saving_ms"] > max(on["spread_ms"], gr["spread_ms"]))
    if args.parent_json:
        pj = json.load(open(args.parent_json))
        out["parent_commit"] = {leg: pj[leg] for leg in ("switch_off", "switch_on", "grouped") if leg in pj}
        for leg, p in out["parent_commit"].items():
            d = abs(res[leg]["ms_per_image"] - p["ms_per_image"])
            out[leg + "_vs_parent_ms"] = res[leg]["ms_per_image"] - p["ms_per_image"]
            out[leg + "_within_spread_of_parent"] = bool(d <= max(res[leg]["spread_ms"], p["spread_ms"]))
            out[leg + "_launches_equal_parent"] = bool(res[leg]["profiler_per_image"]["kernel_launches"] ==
                                                       p.get("profiler_per_image", {}).get("kernel_launches"))
        if "grouped" in res and "switch_on" in out["parent_commit"]:
            out["grouped_vs_parent_switch_on_ms"] = res["grouped"]["ms_per_image"] - out["parent_commit"]["switch_on"]["ms_per_image"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}, sort_keys=True))
    for leg in legs:
        print(leg, json.dumps(res[leg], sort_keys=True))


if __name__ == "__main__":
    main()
