"""A multi-class image's cut and merge on the host against the per-class device lists, side by side.

    python tools/bench_class_merge.py                       # -> profiles/class_merge.json

Runs ``test.detect(net, im=...)`` -- lib/test.py:109-178 -- on a THREE-class graph of the shipped template's size (the
dilated template with every ``cls_score_*`` widened to three outputs and the final Reshape to nine channels; synthetic
weights seed 1234, whose class biases put the background at +4 and both foreground classes at -4; conv mode f16x3) and
bench.py's C5 image (1024 x 1024 uint8, seed 1000, the ``configs/smallhardface.toml`` pyramid with flip: ten units).  Both
legs keep the levels in HBM (``SHF_DEVICE_LEVELS=1``) and run the ten units as one ``Net.forward_group``:

  host_merge    ``SHF_GROUPED_FORWARD=1``: every unit's boxes / cls_prob read back, flip fix, unscale, tiling and
                concatenation in numpy, then per class np.where, one upload, one merge, one read-back (``_merge_class_dets``)
  device_merge  ``SHF_DEVICE_MERGE=1``: ``Net.class_lists_add`` after the grouped forward, ``Net.class_lists_finish`` per class

After a warm-up each leg is timed ``--repeats`` times over ``--images`` images, the legs alternating inside one process; a
repeat is a host clock around whole detect() calls, each of which ends in synchronous read-backs.  Per leg: milliseconds
per image of every repeat, their median and spread (max - min), detect()'s own two timers per image (``detect``: levels
and forwards -- on the device leg the list appends too --, ``misc``: the cut and the merges), and from one more, untimed
image with every launch bracketed the profiler's kernel / h2d / d2h milliseconds and launch counts.
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

CLASSES = 3
LEGS = {"host_merge": {"SHF_GROUPED_FORWARD": "1"}, "device_merge": {"SHF_DEVICE_MERGE": "1"}}


def three_class_template(P):
    """The dilated test template with C = 3: per-head class predictors of three outputs, nine softmax channels."""
    msg = P._add_dimension_reduction(P.build_test_template(True))
    heads = 0
    for L in msg.getall("layer"):
        name = str(L.get("name"))
        if name.startswith("cls_score_") and str(L.get("type")) == "Convolution":
            L.get("convolution_param").set("num_output", CLASSES)
            heads += 1
        if name == "cls_prob_reshape":
            shp = L.get("reshape_param").get("shape")
            shp.set_nth("dim", 1, CLASSES * 3)
    assert heads == 3
    return msg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10, help="images per repeat (at least 10)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed images per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_merge.json"))
    args = ap.parse_args()
    n_img, n_rep = max(10, args.images), max(3, args.repeats)

    from smallhardface_amd import caffe, prototxt as P, weights
    from smallhardface_amd import test as T
    from smallhardface_amd.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(ROOT, "configs", "smallhardface.toml"))
    caffe.set_mode_gpu()
    caffe.set_device(0)
    msg = three_class_template(P)
    net = caffe.Net(None, prototxt_text=P.dumps(msg))
    assert net.num_classes == CLASSES
    for name, blobs in weights.synth_params(msg, seed=1234).items():
        for i, arr in enumerate(blobs):
            net.params[name][i].data[...] = arr
    net.commit_params()
    net.set_conv_mode("f16x3")
    im = np.random.default_rng(1000).integers(0, 256, (1024, 1024, 3)).astype(np.uint8)
    os.environ.pop("SHF_HOST_PREPROCESS", None)
    os.environ["SHF_DEVICE_LEVELS"] = "1"

    def select(leg):
        for k in ("SHF_GROUPED_FORWARD", "SHF_DEVICE_MERGE"):
            os.environ.pop(k, None)
        os.environ.update(LEGS[leg])

    def one_image(timers=None):
        return T.detect(net, None, 0.05, timers=timers, pyramid=True, im=im)

    dets = {}
    for leg in LEGS:
        select(leg)
        for _ in range(max(1, args.warmup)):
            dets[leg] = [np.asarray(d, dtype=np.float64) for d in one_image()[0]]
    res = {leg: {"repeats_ms_per_image": [], "detect_timer_ms": [], "misc_timer_ms": []} for leg in LEGS}
    for _ in range(n_rep):
        for leg in LEGS:                       # alternating: both legs see the same neighbours on a shared host
            select(leg)
            net.sync()
            timers = {"detect": T.Timer(), "misc": T.Timer()}
            t0 = time.perf_counter()
            for _i in range(n_img):
                one_image(timers)
            dt = time.perf_counter() - t0
            res[leg]["repeats_ms_per_image"].append(1000.0 * dt / n_img)
            res[leg]["detect_timer_ms"].append(1000.0 * timers["detect"].total_time / n_img)
            res[leg]["misc_timer_ms"].append(1000.0 * timers["misc"].total_time / n_img)
    # the profiler's view of one more image per leg, outside the timed repeats (an event pair around every launch costs the
    # stream a few microseconds each).  The host leg's merges run in the stand-alone box context (shf_bbox_vote), which no
    # net's profiler sees: its merge kernels and copies are missing from these figures, the device leg's are in them.
    for leg in LEGS:
        select(leg)
        net.prof_enable(True)
        net.prof_reset()
        one_image()
        pr = net.prof_read()
        net.prof_enable(False)
        net.prof_reset()
        copies = {"h2d_copy": "h2d_ms", "d2h_copy": "d2h_ms"}
        prof = {"kernel_ms": float(sum(v["ms"] for k, v in pr.items() if k not in copies)),
                "kernel_launches": int(sum(v["launches"] for k, v in pr.items() if k not in copies)),
                "tail_ms": float(pr["detect_tail"]["ms"]), "tail_launches": int(pr["detect_tail"]["launches"]),
                "merge_ms": float(pr["box_merge"]["ms"]), "merge_launches": int(pr["box_merge"]["launches"])}
        for k, name in copies.items():
            prof[name] = float(pr[k]["ms"])
        res[leg]["profiler_per_image"] = prof
    for leg in LEGS:
        r = res[leg]
        v = r["repeats_ms_per_image"]
        r["ms_per_image"] = float(np.median(v))
        r["spread_ms"] = float(max(v) - min(v))
        r["detect_timer_ms"] = float(np.median(r["detect_timer_ms"]))
        r["misc_timer_ms"] = float(np.median(r["misc_timer_ms"]))
        r["boxes_per_class"] = [int(len(d)) for d in dets[leg]]
    select("host_merge")
    h, d = res["host_merge"], res["device_merge"]
    out = {
        "workload": "test.detect(pyramid=True) on a 1024 x 1024 uint8 image (seed 1000), configs/smallhardface.toml pyramid "
                    "(scales %s, flip %s): %d units per image as one Net.forward_group, device-resident levels, a %d-class "
                    "graph of the dilated template's size, conv mode f16x3, synthetic weights seed 1234, thresh 0.05, %s"
                    % (list(cfg.TEST.SCALES), bool(cfg.TEST.FLIP), len(cfg.TEST.SCALES) * (2 if cfg.TEST.FLIP else 1), CLASSES,
                       cfg.TEST.NMS_METHOD),
        "images_per_repeat": n_img, "repeats": n_rep, "warmup_images_per_leg": max(1, args.warmup),
        "unit": "host milliseconds per image; spread = max - min over the repeats; *_timer_ms = detect()'s own timers",
        "rows_per_class_before_merge": net.class_lists_count(),
        "identical_detections": bool(len(dets["host_merge"]) == len(dets["device_merge"]) and all(
            a.shape == b.shape and np.array_equal(a, b) for a, b in zip(dets["host_merge"], dets["device_merge"]))),
        "saving_ms": h["ms_per_image"] - d["ms_per_image"],
        "host_merge_share_of_image": h["misc_timer_ms"] / h["ms_per_image"],
    }
    out["saving_exceeds_spread"] = bool(out["saving_ms"] > max(h["spread_ms"], d["spread_ms"]))
    out.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, dict)}, sort_keys=True))
    for leg in LEGS:
        print(leg, json.dumps(res[leg], sort_keys=True))


if __name__ == "__main__":
    main()
