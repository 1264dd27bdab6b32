"""The in-repo AFW / Pascal Faces evaluator (smallhardface_amd/face_eval.py, host path) against what the REFERENCE's own
evaluator produced (tests/golden/make_face_eval_golden.py: external/marcopede-face-eval-f2870fd85d48 evaluate_optim on its
own detections/{AFW,PASCAL}/Ours.txt and a synthetic ground truth), and one hand case per rule."""
import os
import subprocess
import sys

import numpy as np
import pytest

from smallhardface_amd import datasets as D
from smallhardface_amd import face_eval as F
from tests import face_eval_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference's own output -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nit,ovr", K.COMBOS)
@pytest.mark.parametrize("ds", K.DATASETS)
def test_rounds_curve_and_ap_equal_the_reference(ds, nit, ovr):
    g, dets, gt, _ = K.golden_case(ds)
    kept = F.filter_detections(dets, F.min_pixels(30, 30))
    assert len(kept) == int(g[ds + "_n_filtered"][0]) < len(dets)
    ap, rec, prec, info = F.evaluate(kept, gt, ovr=ovr, iters=nit)
    K.assert_equals_fixture(g, K.tag(ds, nit, ovr), ap, rec, prec, info)


@pytest.mark.parametrize("ds", K.DATASETS)
def test_the_fixture_holds_the_cases_it_was_built_for(ds):
    g, dets, gt, objects = K.golden_case(ds)
    t = K.tag(ds, 5, 0.5)
    assert np.isnan(g[t + "prec"][0]) and not np.isnan(g[t + "prec"][-1])      # the top detection sits on a difficult box
    assert 0.0 < g[t + "ap"][0] < 1.0
    assert not np.array_equal(g[t + "tp"][0], g[t + "tp"][-1])                    # the refinement rounds change the matching
    assert g[t + "ap"][0] != g[K.tag(ds, 1, 0.5) + "ap"][0]
    assert any(o.shape[0] == 0 for o in objects)                                  # images with an empty box list
    keys = set(F.image_key(n) for n in gt.names)
    assert any(n not in keys for n in dets.names)                                 # detections without ground truth
    flags = np.concatenate(gt.difficult)
    np.testing.assert_array_equal(flags, g[ds + "_gt_difficult"] != 0)            # database.py's difficult rule
    said = np.concatenate([o[:, 5] != 0 if o.shape[1] >= 6 else np.zeros(len(o), bool) for o in objects if len(o)])
    assert 0.05 < said.mean() < 0.3 and (flags & ~said).any()                     # ~15 % flagged, some by size alone
    assert any(len(b) and len(np.unique(b, axis=0)) < len(b) for b in gt.boxes)   # a duplicated box
    assert (ds == "pascal") == any(o.shape[1] == 4 for o in objects if len(o))    # the four-column Pascal row


# ---- the vectorised host round against a scalar walk ---------------------------------------------------------------------
@pytest.mark.parametrize("ovr", [0.5, 0.3])
@pytest.mark.parametrize("kw", [{}, {"equal_scores": True}, {"equal_ious": True}, {"all_difficult": True}],
                         ids=["plain", "equal_scores", "equal_ious", "all_difficult"])
def test_host_round_equals_the_scalar_walk(kw, ovr):
    dets, gt = K.batch(31, K.boundary_shapes(), **kw)
    dets, code, index = K.one_round(dets, gt, ovr, F.match_host)
    want_code, want_index = K.scalar_round(dets, gt, ovr)
    np.testing.assert_array_equal(code, want_code)
    np.testing.assert_array_equal(index, want_index)
    assert (code == F.TRUE_POSITIVE).any() != bool(kw.get("all_difficult"))
    if kw.get("all_difficult"):
        assert (code == F.NEITHER).any() and (code == F.FALSE_POSITIVE).any()


@pytest.mark.parametrize("ds", K.DATASETS)
def test_host_round_equals_the_scalar_walk_on_the_fixture(ds):
    _, dets, gt, _ = K.golden_case(ds)
    dets, code, index = K.one_round(dets, gt, 0.5, F.match_host)
    want_code, want_index = K.scalar_round(dets, gt, 0.5)
    np.testing.assert_array_equal(code, want_code)
    np.testing.assert_array_equal(index, want_index)


# ---- hand cases, one per rule -----------------------------------------------------------------------------------------------
def run(det_rows, boxes, difficult=None, names=None, ovr=0.5, iters=1, gt_names=("a.jpg",)):
    """detections (score, x1, y1, x2, y2) of image 'a' unless ``names`` says otherwise, one ground-truth image"""
    det_rows = np.array(det_rows, dtype=np.float64).reshape(-1, 5)
    dets = F.Detections(names or ["a"] * len(det_rows), det_rows)
    boxes = [np.array(b, dtype=np.float64).reshape(-1, 4) for b in ([boxes] if len(gt_names) == 1 else boxes)]
    difficult = [np.zeros(len(b), bool) for b in boxes] if difficult is None else \
        ([difficult] if len(gt_names) == 1 else difficult)
    ap, rec, prec, info = F.evaluate(dets, F.FaceGT(list(gt_names), boxes, difficult), ovr=ovr, iters=iters)
    r = info["rounds"][-1]
    return ap, rec, prec, r["tp"], r["fp"], r["index"]


def test_iou_exactly_equal_to_ovr_is_a_false_positive():
    # (0,0,9,9) has 100 pixels, (0,0,9,4) 50 of them: IoU = 50 / 100 exactly
    ap, _, _, tp, fp, _ = run([[0.9, 0, 0, 9, 4]], [[0, 0, 9, 9]])
    assert tp.tolist() == [0] and fp.tolist() == [1] and ap == 0.0
    ap, _, _, tp, fp, _ = run([[0.9, 0, 0, 9, 4]], [[0, 0, 9, 9]], ovr=0.4999)
    assert tp.tolist() == [1] and fp.tolist() == [0] and ap == 1.0


def test_two_boxes_with_equal_iou_take_the_later_one():
    _, _, _, tp, fp, index = run([[0.9, 10, 10, 50, 50]], [[10, 10, 50, 50], [200, 200, 240, 240], [10, 10, 50, 50]])
    assert index.tolist() == [2] and tp.tolist() == [1]
    # ... so a difficult twin behind the plain box turns the detection into "neither", the other way round it counts
    _, _, _, tp, fp, _ = run([[0.9, 10, 10, 50, 50]], [[10, 10, 50, 50], [10, 10, 50, 50]], difficult=[False, True])
    assert tp.tolist() == [0] and fp.tolist() == [0]
    _, _, _, tp, fp, _ = run([[0.9, 10, 10, 50, 50]], [[10, 10, 50, 50], [10, 10, 50, 50]], difficult=[True, False])
    assert tp.tolist() == [1] and fp.tolist() == [0]


def test_no_overlap_at_all_ends_on_the_last_box():
    """covr = 0 >= maxovr = 0 on every box: the walk ends on the last index, and the detection is a false positive"""
    _, _, _, tp, fp, index = run([[0.9, 500, 500, 540, 540]], [[10, 10, 50, 50], [100, 100, 140, 140]])
    assert index.tolist() == [1] and fp.tolist() == [1]


def test_a_taken_box_gives_a_false_positive():
    ap, rec, prec, tp, fp, _ = run([[0.9, 10, 10, 50, 50], [0.8, 11, 10, 50, 50], [0.7, 100, 100, 140, 140]],
                                   [[10, 10, 50, 50], [100, 100, 140, 140]])
    assert tp.tolist() == [1, 0, 1] and fp.tolist() == [0, 1, 0]
    np.testing.assert_array_equal(rec, [0.5, 0.5, 1.0])
    np.testing.assert_array_equal(prec, [1.0, 0.5, 2.0 / 3.0])
    assert ap == 0.5 * 1.0 + 0.5 * (2.0 / 3.0)


def test_a_difficult_box_gives_neither_and_a_nan_precision_that_stays():
    ap, rec, prec, tp, fp, _ = run([[0.9, 10, 10, 50, 50], [0.8, 100, 100, 140, 140]],
                                   [[10, 10, 50, 50], [100, 100, 140, 140]], difficult=[True, False])
    assert tp.tolist() == [0, 1] and fp.tolist() == [0, 0]
    assert np.isnan(prec[0]) and prec[1] == 1.0 and rec.tolist() == [0.0, 1.0]
    assert ap == 1.0        # tot counts the plain box only; the NaN sits on a recall step of width 0


def test_an_unknown_image_gives_a_false_positive():
    _, rec, prec, tp, fp, index = run([[0.9, 10, 10, 50, 50], [0.8, 10, 10, 50, 50], [0.7, 10, 10, 50, 50]],
                                      [[[10, 10, 50, 50]], np.zeros((0, 4))], names=["nobody", "a", "empty"],
                                      gt_names=("dir/a.png", "empty.jpg"))
    assert fp.tolist() == [1, 0, 1] and tp.tolist() == [0, 1, 0] and index.tolist() == [-1, 0, -1]
    np.testing.assert_array_equal(prec, [0.0, 0.5, 1.0 / 3.0])


def test_filterdet_at_width_21_versus_22():
    assert F.min_pixels(30, 30) == 21
    dets = F.Detections(["a", "b", "c", "d"], [[0.9, 0, 0, 21, 21], [0.8, 0, 0, 22, 5], [0.7, 0, 0, 5, 21.5], [0.6, 0, 0, 21, 3]])
    assert F.filter_detections(dets, 21).names == ["b", "c"]           # width OR height strictly above minpix
    assert F.min_pixels(40, 20) == 20 and F.min_pixels(50, 50) == 35


def test_the_minw_flag_makes_small_boxes_difficult():
    objects = [[[0, 0, 29, 40, 0, 0], [0, 0, 30, 30, 0, 0], [0, 0, 40, 29.5, 0, 0], [0, 0, 90, 90, 0, 1]]]
    assert F.make_gt(["a.jpg"], objects, 30, 30).difficult[0].tolist() == [True, False, True, True]
    assert F.make_gt(["a.jpg"], objects, 20, 20).difficult[0].tolist() == [False, False, False, True]
    assert F.make_gt(["a.jpg"], objects, 31, 10).difficult[0].tolist() == [True, True, False, True]
    four = F.make_gt(["a.jpg"], [[[0, 0, 50, 50], [0, 0, 10, 50]]], 30, 30)    # Pascal rows without the flag columns
    assert four.difficult[0].tolist() == [False, True]
    with pytest.raises(ValueError):
        F.make_gt(["a.jpg"], [[[0, 0, 50, 50]]], 30, 30, four_columns_ok=False)


def test_a_round_without_true_positives_gives_ap_zero():
    """the means of empty lists are NaN, the boxes NaN from the second round on, every detection a false positive"""
    dets = F.Detections(["a", "a"], [[0.9, 300, 300, 340, 340], [0.8, 400, 300, 440, 340]])
    gt = F.FaceGT(["a.jpg"], [[[10, 10, 50, 50]]], [[False]])
    ap, rec, prec, info = F.evaluate(dets, gt, iters=3)
    assert ap == 0.0 and rec.tolist() == [0.0, 0.0] and prec.tolist() == [0.0, 0.0]
    assert all(np.isnan(r["means"]).all() for r in info["rounds"]) and np.isnan(info["boxes"]).all()
    assert all(r["fp"].tolist() == [1, 1] for r in info["rounds"])


def test_refinement_moves_the_boxes_by_the_mean_of_the_true_positives():
    """one true positive, shifted by (+4, -2) and half the size: the means are its own terms and the transform puts every
    detection through them (transf_dets)"""
    ap, rec, prec, info = F.evaluate(F.Detections(["a", "a"], [[0.9, 0, 0, 40, 20], [0.5, 100, 100, 120, 140]]),
                                     F.FaceGT(["a.jpg"], [[[14, 3, 34, 13]]], [[False]]), ovr=0.2, iters=1)
    tx, ty, sx, sy = info["rounds"][0]["means"]
    assert (tx, ty, sx, sy) == ((24. - 20.) / 40., (8. - 10.) / 20., 0.5, 0.5)
    np.testing.assert_array_equal(info["boxes"], [[14, 3, 34, 13], [100 + 10 + 2 - 5, 100 + 20 - 4 - 10, 117, 126]])


# ---- readers, wiring, command line ------------------------------------------------------------------------------------------
def test_load_annotations_mat_reads_the_shape_database_py_indexes(tmp_path):
    _, _, gt, objects = K.golden_case("pascal")
    path = str(tmp_path / "Annotations_Face_PASCALLayout_large_fixed.mat")
    K.save_annotations(path, gt.names, objects)
    back = F.load_annotations_mat(path, 30, 30)
    assert back.names == gt.names
    for a, b, c, d in zip(back.boxes, gt.boxes, back.difficult, gt.difficult):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(c, d)
    wide = F.load_annotations_mat(path, 10, 10)
    assert np.concatenate(wide.difficult).sum() < np.concatenate(gt.difficult).sum()
    with pytest.raises(ValueError):
        F.load_annotations_mat(path, 30, 30, dataset="AFW")            # the AFW class has no four-column rule


def fixture_as_written(ds, out_dir):
    """the fixture's detections put through the product's writer: (image paths, all_boxes, the rows as the writer prints
    them).  The writer lowers ymin by 20 % of the height; the boxes handed in are chosen so that it prints the fixture's."""
    _, dets, _, _ = K.golden_case(ds)
    paths, per = [], {}
    for n, r in zip(dets.names, dets.rows):
        if n not in per:
            per[n] = []
            paths.append("images/%s.jpg" % n)
        per[n].append([r[1], (r[2] - 0.2 * (r[4] + 1)) / 0.8, r[3], r[4], r[0]])
    boxes = [np.array(per[os.path.basename(p)[:-4]], dtype=np.float64) for p in paths]
    return paths, [[[] for _ in paths], boxes], dets


@pytest.mark.parametrize("ds", K.DATASETS)
def test_load_detections_reads_what_the_writer_wrote(ds, tmp_path):
    paths, all_boxes, dets = fixture_as_written(ds, tmp_path)
    writer = D.write_detections_afw if ds == "afw" else D.write_detections_pascal
    writer(paths, all_boxes, str(tmp_path))
    path = str(tmp_path / ("afw_res.txt" if ds == "afw" else "pascal_res.txt"))
    assert open(path).read() == K.detection_lines(dets)               # (the fixture's rows, in the fixture's order)
    back = F.load_detections(path)
    want = dets.sorted_by_score()
    assert back.names == want.names
    np.testing.assert_array_equal(back.rows, want.rows)
    assert (np.diff(back.rows[:, 0]) <= 0).all()


@pytest.mark.parametrize("ds", K.DATASETS)
def test_imagelist_evaluates_when_the_annotation_file_is_there(ds, tmp_path):
    g, _, gt, objects = K.golden_case(ds)
    paths, all_boxes, _ = fixture_as_written(ds, tmp_path)
    db = "afw_val" if ds == "afw" else "pascalface_val"
    out = str(tmp_path / "out")
    today = "detections written to {}".format(os.path.join(out, "detections"))
    assert D.ImageList(db, paths).evaluate_detections(all_boxes, output_dir=out) == today
    gt_dir = tmp_path / "ground_truth"
    gt_dir.mkdir()
    assert D.ImageList(db, paths, ground_truth=str(gt_dir)).evaluate_detections(all_boxes, output_dir=out) == today
    # the OTHER dataset's annotation file does not count
    K.save_annotations(str(gt_dir / F.ANNOTATION_FILES["PASCAL" if ds == "afw" else "AFW"]), gt.names, objects)
    assert D.ImageList(db, paths, ground_truth=str(gt_dir)).evaluate_detections(all_boxes, output_dir=out) == today
    K.save_annotations(str(gt_dir / F.ANNOTATION_FILES["AFW" if ds == "afw" else "PASCAL"]), gt.names, objects)
    msg = D.ImageList(db, paths, ground_truth=str(gt_dir)).evaluate_detections(all_boxes, output_dir=out)
    assert msg == "AP: {:.4f}".format(g[K.tag(ds, 5, 0.5) + "ap"][0])
    # a WIDER list is not touched by these files
    assert D.ImageList("wider_val", ["0--Parade/x.jpg"], ground_truth=str(gt_dir)).evaluate_detections(
        [[[]], [np.zeros((0, 5))]], output_dir=out) == today


def test_the_module_cli_prints_the_same_ap(tmp_path):
    g, dets, gt, objects = K.golden_case("pascal")
    det_file, ann = str(tmp_path / "pascal_res.txt"), str(tmp_path / "ann.mat")
    open(det_file, "w").write(K.detection_lines(dets))
    K.save_annotations(ann, gt.names, objects)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("SHF_DEVICE_EVAL", None)

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "smallhardface_amd.face_eval"] + list(args), cwd=str(tmp_path),
                              env=env, capture_output=True, text=True, check=True).stdout
    assert cli("--dataset", "PASCAL", "--ann", ann, det_file).startswith(
        "AP: {:.4f}".format(g[K.tag("pascal", 5, 0.5) + "ap"][0]))
    assert cli("--dataset", "PASCAL", "--ann", ann, "--nit", "1", det_file).startswith(
        "AP: {:.4f}".format(g[K.tag("pascal", 1, 0.5) + "ap"][0]))
    ap_wide = F.face_eval(det_file, ann, "PASCAL", minw=10, minh=12)[0]
    assert cli("--dataset", "PASCAL", "--ann", ann, "--minw", "10", "--minh", "12", det_file).startswith(
        "AP: {:.4f}".format(ap_wide))
    assert "{:.4f}".format(ap_wide) != "{:.4f}".format(g[K.tag("pascal", 5, 0.5) + "ap"][0])
