#!/usr/bin/env python3
"""Generate tests/golden/face_eval.npz (+ face_eval_names.json) from the REFERENCE's own AFW / Pascal Faces evaluator.

Run in the authoring container only (needs the reference tree, make_golden.REF):

    python tests/golden/make_face_eval_golden.py

What it does (nothing from the reference is copied into this repo):
  * converts external/marcopede-face-eval-f2870fd85d48/{VOCpr,loadData,database,util}.py to py3 in a scratch TEMP dir
    with lib2to3 (all fixers except fix_import) and applies the two Python 3 patches the evaluator needs, both to its
    ``cmp``-style sort:
      1. VOCpr.py:12-13   ``cmpscore`` returns ``-cmp(a[1], b[1])``; Python 3 has no ``cmp`` -> the same three-way value
                          spelled ``-((a[1] > b[1]) - (a[1] < b[1]))``;
      2. VOCpr.py:36,117  ``detlist.sort(cmpscore)``; Python 3's sort takes no comparison function ->
                          ``detlist.sort(key=functools.cmp_to_key(cmpscore))`` (a stable sort by the same order).
    Nothing is stubbed away: pylab is matplotlib's own on the Agg backend, the .mat files go through scipy;
  * reads the rows of the reference's detections/AFW/Ours.txt and detections/PASCAL/Ours.txt (data its programs read)
    with its loadDetections, and filters them with its filterdet;
  * builds a seeded synthetic ground truth from them (jittered, commonly shifted and stretched copies of the high-score
    detections, about 15 % flagged difficult, some under 30 px, duplicated boxes, the top-scored detection of all on a
    difficult box, images with an empty box list, images left out, one four-column Pascal matrix), writes it as
    annotations/*.mat in the layout database.py indexes and loads it back through the reference's AFW / PASCALfaces
    classes and getRecord;
  * runs the reference's evaluate_optim (iter = 5 and 1, ovr = 0.5 and 0.3) and records, per round, the tp / fp arrays
    and the four numpy.mean values of VOCprRecordOptim's lists, and the final rec / prec / VOCap / VOColdap.
The fixture is DATA only.  The archive is written with fixed member timestamps, so a rerun reproduces it bit for bit.

Reference entry points exercised (relative to external/marcopede-face-eval-f2870fd85d48):
  loadData.py:13,82     loadDetections / loadDetectionsPascalFormat
  VOCpr.py:234          filterdet
  database.py:437,526   AFW / PASCALfaces (getImageName, getBBox), :121 getRecord
  VOCpr.py:264          evaluate_optim -> :93 VOCprRecordOptim, :250 transf_dets, :214 drawPrfast, :191 VOCap,
                        :201 VOColdap; util.py:176 overlap
"""
import io
import json
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import REF  # noqa: E402

EVAL = os.path.join(REF, "external", "marcopede-face-eval-f2870fd85d48")
MODULES = ("VOCpr.py", "loadData.py", "database.py", "util.py")
ROUNDS = (5, 1)
OVRS = (0.5, 0.3)
MINW = MINH = 30


def convert_evaluator(tmp):
    from lib2to3 import refactor
    fixers = [f for f in refactor.get_fixers_from_package("lib2to3.fixes") if not f.endswith("fix_import")]
    rt = refactor.RefactoringTool(fixers)
    for fn in MODULES:
        src = open(os.path.join(EVAL, fn)).read()
        if not src.endswith("\n"):
            src += "\n"
        out = str(rt.refactor_string(src, fn))
        if fn == "VOCpr.py":
            a = "return -cmp(a[1], b[1])"
            b = "detlist.sort(cmpscore)"
            assert out.count(a) == 1 and out.count(b) == 2
            out = out.replace(a, "return -((a[1] > b[1]) - (a[1] < b[1]))")
            out = out.replace(b, "detlist.sort(key=__import__('functools').cmp_to_key(cmpscore))")
        open(os.path.join(tmp, fn), "w").write(out)


def synthetic_gt(dets, rng, pascal):
    """``dets``: the reference's [key, score, x1, y1, x2, y2] rows, score-descending.  Returns (names, objects): per image
    of the annotation its file name and its ``x1 y1 x2 y2 0 difficult`` matrix (k x 6; 0 x 0 for an empty image; one
    k x 4 matrix for Pascal)."""
    by_img, order = {}, []
    for d in dets:
        if d[0] not in by_img:
            by_img[d[0]] = []
            order.append(d[0])
        by_img[d[0]].append(d)
    top_key = dets[0][0]
    names, objects = [], []
    n_small = 0
    for k, key in enumerate(sorted(order)):
        if key != top_key and k % 17 == 3:
            continue                                   # detections without any ground truth
        names.append(key + ".jpg")
        if key != top_key and k % 13 == 5:
            objects.append(np.zeros((0, 0)))           # an image with an empty box list
            continue
        rows = []
        for d in by_img[key]:
            if d[1] < 0.6 and not (d is by_img[key][0]):
                continue
            box = np.array(d[2:6], dtype=np.float64)
            w, h = box[2] - box[0], box[3] - box[1]
            # jitter around a common shift and stretch, so that the refinement rounds have something to find
            box = np.round(box + (np.array([0.12, -0.10, 0.24, 0.06]) + rng.normal(0, 0.10, 4)) * np.array([w, h, w, h]))
            diff = float(rng.uniform() < 0.15)
            if rng.uniform() < 0.06:                    # a face under 30 px: difficult by the size rule
                box[2] = box[0] + float(rng.integers(8, 30))
                n_small += 1
            rows.append([box[0], box[1], box[2], box[3], 0.0, diff])
        if key == top_key:
            t = dets[0]
            rows[0] = [t[2], t[3], t[4], t[5], 0.0, 1.0]    # the top-scored detection of all sits on a difficult box
        if k % 11 == 2:
            rows.append(list(rows[-1]))                # a duplicated box: two equal IoUs
        if k % 7 == 1:                                 # a face nobody found
            rows.append([5.0, 5.0, 5.0 + float(rng.integers(35, 90)), 5.0 + float(rng.integers(35, 90)), 0.0, 0.0])
        objects.append(np.array(rows, dtype=np.float64).reshape(-1, 6))
    assert n_small > 0
    if pascal:                                         # one four-column row (database.py:586-588)
        j = next(i for i, o in enumerate(objects) if o.shape[0] == 1 and names[i] != top_key + ".jpg")
        objects[j] = objects[j][:, :4].copy()
    return names, objects


def save_annotations(path, names, objects):
    from scipy import io as sio
    ann = np.zeros((len(names), 1), dtype=[("imgname", object), ("objects", object)])
    for i, (n, o) in enumerate(zip(names, objects)):
        ann[i, 0]["imgname"] = n
        ann[i, 0]["objects"] = o
    sio.savemat(path, {"Annotations": ann})


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and a fixed order: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    os.environ["MPLBACKEND"] = "Agg"
    tmp = tempfile.mkdtemp(prefix="shf_face_eval_py3_")
    convert_evaluator(tmp)
    os.makedirs(os.path.join(tmp, "annotations"))
    os.chdir(tmp)
    sys.path.insert(0, tmp)
    old = sys.stdout
    sys.stdout = io.StringIO()                 # the evaluator prints its progress
    try:
        import VOCpr
        import database
        from loadData import loadDetections

        # recorders around the reference's own functions (they are looked up as module globals when evaluate_optim runs)
        rounds, curve = [], {}
        record_optim, draw_fast = VOCpr.VOCprRecordOptim, VOCpr.drawPrfast

        def recording_optim(*a, **kw):
            r = record_optim(*a, **kw)
            tp, fp, _, tot, tx, ty, sx, sy = r
            with np.errstate(all="ignore"):
                rounds.append((tp.copy(), fp.copy(), tot, [VOCpr.numpy.mean(v) for v in (tx, ty, sx, sy)]))
            return r

        def recording_draw(tp, fp, tot, show=True, col="g"):
            r = draw_fast(tp, fp, tot, show=show, col=col)
            curve["rec"], curve["prec"], curve["ap"] = r
            return r

        VOCpr.VOCprRecordOptim, VOCpr.drawPrfast = recording_optim, recording_draw

        out, names_out = {}, {}
        for ds, sub, ann_file, klass, seed in (
                ("afw", "AFW", "new_annotations_AFW.mat", database.AFW, 4101),
                ("pascal", "PASCAL", "Annotations_Face_PASCALLayout_large_fixed.mat", database.PASCALfaces, 4102)):
            det_file = os.path.join(EVAL, "detections", sub, "Ours.txt")
            raw = loadDetections(det_file)
            gt_names, objects = synthetic_gt(raw, np.random.default_rng(seed), ds == "pascal")
            save_annotations(os.path.join("annotations", ann_file), gt_names, objects)
            ts_images = database.getRecord(klass(minw=MINW, minh=MINH), 10000)
            minpix = int(np.sqrt(0.5 * MINW * MINH))
            # detections as read, in file order (the test reads them from text written with these values)
            lines = [l.strip().split(" ") for l in open(det_file).readlines()]
            keys = sorted(set(l[0] for l in lines))
            names_out[ds] = {"det_names": keys, "gt_names": gt_names}
            out[ds + "_det_name"] = np.array([keys.index(l[0]) for l in lines], dtype=np.int32)
            out[ds + "_det_rows"] = np.array([[float(v) for v in l[1:6]] for l in lines], dtype=np.float64)
            out[ds + "_n_filtered"] = np.array([len(VOCpr.filterdet(list(raw), minpix))])
            out[ds + "_gt_count"] = np.array([o.shape[0] for o in objects], dtype=np.int32)
            out[ds + "_gt_ncol"] = np.array([o.shape[1] for o in objects], dtype=np.int32)
            out[ds + "_gt_rows"] = np.concatenate([np.hstack([o, np.zeros((o.shape[0], 6 - o.shape[1]))]).reshape(-1, 6)
                                                   for o in objects if o.shape[0]])
            # what getBBox made of them: [y1, x1, y2, x2, 0, difficult] per image
            out[ds + "_gt_difficult"] = np.array([b[5] for im in ts_images for b in im["bbox"]], dtype=np.uint8)
            for nit in ROUNDS:
                for ovr in OVRS:
                    del rounds[:]
                    curve.clear()
                    dets = VOCpr.filterdet(loadDetections(det_file), minpix)
                    with np.errstate(all="ignore"):
                        r = VOCpr.evaluate_optim(ts_images, dets, "Ours", "green", iter=nit, ovr=ovr)
                        ap11 = VOCpr.VOColdap(curve["rec"], curve["prec"])
                    assert len(rounds) == nit and r[0] == curve["ap"]
                    tag = "%s_it%d_ovr%02d_" % (ds, nit, int(round(ovr * 100)))
                    out[tag + "tp"] = np.stack([t[0] for t in rounds]).astype(np.uint8)
                    out[tag + "fp"] = np.stack([t[1] for t in rounds]).astype(np.uint8)
                    out[tag + "means"] = np.array([t[3] for t in rounds], dtype=np.float64)
                    out[tag + "tot"] = np.array([rounds[-1][2]])
                    out[tag + "rec"] = np.asarray(curve["rec"], dtype=np.float64)
                    out[tag + "prec"] = np.asarray(curve["prec"], dtype=np.float64)
                    out[tag + "ap"] = np.array([curve["ap"], ap11], dtype=np.float64)
    finally:
        sys.stdout = old
    write_npz(os.path.join(OUT, "face_eval.npz"), out)
    json.dump(names_out, open(os.path.join(OUT, "face_eval_names.json"), "w"), sort_keys=True)
    os.chdir(OUT)
    shutil.rmtree(tmp, ignore_errors=True)
    for ds in ("afw", "pascal"):
        print(ds, "AP it5 ovr0.5 =", out[ds + "_it5_ovr50_ap"], " NaN precisions:", int(np.isnan(out[ds + "_it5_ovr50_prec"]).sum()),
              " filtered rows:", int(out[ds + "_n_filtered"][0]), "of", len(out[ds + "_det_rows"]))
    print("face_eval fixture written to", OUT)


if __name__ == "__main__":
    main()
