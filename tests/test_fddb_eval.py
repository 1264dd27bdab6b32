"""The in-repo FDDB evaluator (smallhardface_amd/fddb_eval.py, host path) against counts derived by hand.

FDDB's published ``evaluate`` binary is not available, so nothing here is held to it: the mask rules are the ones the module
states, the pixel counts below were worked out from those rules (integer radii at angle 0 only, half-integer radii where
the shape is rotated, so that no lattice point sits on a boundary), and the ROC of the three-image file is written out in
full."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from smallhardface_amd import datasets as D
from smallhardface_amd import fddb_eval as F
from tests import fddb_eval_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = K.PI


# ---- masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,pixels", [(1, 5), (2, 13), (3, 29), (4, 49), (5, 81), (10, 317)])
def test_a_circle_on_a_pixel_centre_has_the_lattice_count(r, pixels):
    assert K.single([r, r, 0.0, 50, 50])[1] == pixels
    assert K.single([r, r, 0.0, 50, 50], size=(200, 200))[1] == pixels


@pytest.mark.parametrize("angle", [0.0, PI / 4, PI / 2, 1.0])
def test_a_half_integer_circle_has_97_pixels_at_any_angle(angle):
    assert K.single([5.5, 5.5, angle, 50, 50])[1] == 97


def test_an_integer_circle_at_a_quarter_turn_loses_its_four_boundary_pixels():
    """cos(pi/2) is 6e-17, not 0: the four lattice points ON the circle fall outside.  Documented, not corrected."""
    assert K.single([5, 5, 0.0, 50, 50])[1] == 81
    assert K.single([5, 5, PI / 2, 50, 50])[1] == 77


def test_a_rectangle_over_the_circle():
    inter, area, det_area = K.single([5.5, 5.5, 0.0, 20, 20], rows=[[14, 14, 12, 12, 0.9]])
    assert (inter.tolist(), area, det_area.tolist()) == ([97], 97, [169])
    S = F.scores(inter.reshape(1, 1), [area], det_area)
    assert S[0, 0] == 97 / 169 and S[0, 0] > 0.5


@pytest.mark.parametrize("angle,inside,cut", [(0.0, 183, 130), (PI / 2, 183, 159)])
def test_an_ellipse_and_its_clipping_on_the_left(angle, inside, cut):
    assert K.single([10.5, 5.5, angle, 30, 30], size=(100, 100))[1] == inside
    assert K.single([10.5, 5.5, angle, 3, 30], size=(100, 100))[1] == cut
    assert K.single([10.5, 5.5, angle, 3, 30])[1] == inside               # without a size nothing is clipped


def test_the_corner_rule_rounds_halves_to_even():
    geom, _ = K.geom_of([[]], [[[14.5, 14, 3, 3, 0.9], [15.5, 14, 3, 3, 0.9], [14, 14, 0, 3, 0.5]]], [(100, 100)])
    assert geom["rect"].tolist() == [[14, 14, 18, 17], [16, 14, 18, 17], [14, 14, 14, 17]]
    assert geom["det_area"].tolist() == [5 * 4, 3 * 4, 1 * 4]            # (w = 0 is one column)


def test_a_rectangle_outside_the_canvas_has_no_area_and_no_score():
    inter, area, det_area = K.single([5.5, 5.5, 0.0, 20, 20], rows=[[200, 200, 5, 5, 0.9], [-30, 10, 5, 5, 0.9]],
                                     size=(100, 100))
    assert det_area.tolist() == [0, 0] and inter.tolist() == [0, 0]
    assert F.scores(inter.reshape(1, 2), [area], det_area).tolist() == [[0.0, 0.0]]


def test_a_zero_union_scores_zero():
    assert F.scores(np.zeros((1, 1), dtype=np.int64), [0], [0]).tolist() == [[0.0]]
    # an ellipse smaller than a pixel, between pixel centres, against a rectangle outside the canvas
    inter, area, det_area = K.single([0.3, 0.3, 0.0, 10.5, 10.5], rows=[[200, 200, 5, 5, 0.9]], size=(100, 100))
    assert (area, det_area.tolist(), inter.tolist()) == (0, [0], [0])
    assert F.scores(inter.reshape(1, 1), [area], det_area)[0, 0] == 0.0


def test_scan_boxes_hold_every_pixel_of_the_ellipse():
    """a box one pixel wider on every side counts the same: the scan box changes no count"""
    rng = np.random.default_rng(5)
    for _ in range(40):
        e = [rng.uniform(0.3, 30), rng.uniform(0.3, 30), rng.uniform(-PI, PI), rng.uniform(20, 80), rng.uniform(20, 80)]
        geom, _ = K.geom_of([[e]], [[]])
        wide = geom["ell_box"][0] + np.array([-1, -1, 1, 1])
        assert F.ellipse_mask(geom["ell"][0], wide).sum() == F.ellipse_mask(geom["ell"][0], geom["ell_box"][0]).sum()


# ---- matching -----------------------------------------------------------------------------------------------------------------
def test_the_assignment_maximises_the_sum_not_each_row():
    assert F.match_pairs([[0.6, 0.55], [0.58, 0.0]]) == [(0, 1), (1, 0)]


def test_an_all_zero_matrix_has_no_pairs():
    assert F.match_pairs(np.zeros((2, 3))) == []
    assert F.match_pairs(np.zeros((0, 3))) == [] and F.match_pairs(np.zeros((2, 0))) == []


def test_extra_detections_and_extra_annotations_stay_unmatched():
    assert F.match_pairs([[0.2, 0.7, 0.6]]) == [(0, 1)]                   # detections 0 and 2 keep m = 0
    assert F.match_pairs([[0.2], [0.7], [0.6]]) == [(1, 0)]
    assert F.match_pairs([[0.9, 0.0], [0.8, 0.0]]) == [(0, 0)]           # (the zero pair is dropped)
    dets = F.Detections(["a"], [[[14, 14, 12, 12, 0.9], [14, 14, 12, 13, 0.8], [60, 60, 5, 5, 0.7]]])
    res = F.evaluate(dets, F.Annotations(["a"], [[[5.5, 5.5, 0.0, 20, 20]]]))
    assert res["m"].tolist() == [97 / 169, 0.0, 0.0] and res["pairs"] == [[(0, 0, 97 / 169)]]


# ---- curves -----------------------------------------------------------------------------------------------------------------
def test_the_three_image_file_has_the_roc_written_out_here():
    dets, gt = K.three_images()
    res = F.evaluate(dets, gt, sizes=K.THREE_SIZES)
    assert res["N"] == 4
    assert res["ann_area"].tolist() == [97, 183, 13, 29]
    assert res["det_area"].tolist() == [169, 121, 299, 713, 25]
    assert res["inter"].tolist() == [97, 0, 183, 183, 13, 0]
    a, b, c = 97 / 169, 183 / 299, 13 / 25
    assert res["m"].tolist() == [a, 0.0, b, 0.0, c]
    assert res["pairs"] == [[(0, 0, a)], [(0, 0, b)], [(0, 0, c)]]
    # thresholds 0.7, 0.8 (two detections share it: one row), 0.9, 0.95; TPC adds in falling score, then file order
    all_five = (((c + a) + 0.0) + b) + 0.0
    four = ((c + a) + 0.0) + b
    np.testing.assert_array_equal(res["disc"], [[3 / 4, 2], [3 / 4, 1], [2 / 4, 0], [1 / 4, 0]])
    np.testing.assert_array_equal(res["cont"], [[all_five / 4, 2], [four / 4, 1], [(c + a) / 4, 0], [c / 4, 0]])
    assert res["disc_at_1000"] == 3 / 4 and res["cont_at_1000"] == all_five / 4
    assert F.result_string(res) == "rect_disc_at_1000: 0.7500, rect_cont_at_1000: {:.4f}".format(all_five / 4)
    # an image of the annotation file without a detection block has no detections; an unknown block is dropped
    fewer = F.Detections(K.THREE_NAMES[:2] + ["elsewhere"], K.THREE_ROWS[:2] + [[[1, 1, 5, 5, 0.99]]])
    res2 = F.evaluate(fewer, gt, sizes=K.THREE_SIZES)
    assert res2["N"] == 4 and res2["m"].tolist() == [a, 0.0, b, 0.0]
    np.testing.assert_array_equal(res2["disc"], [[2 / 4, 2], [2 / 4, 1], [1 / 4, 0]])


def test_a_score_of_exactly_one_half_is_not_a_discrete_hit():
    """a rectangle over half of another rectangle's pixels: 50 / (100 + 50 - 50)"""
    S = F.scores(np.array([[50]]), [100], [50])
    assert S[0, 0] == 0.5
    disc, cont = F.roc([0.9, 0.8], [S[0, 0], np.nextafter(0.5, 1.0)], 2)
    np.testing.assert_array_equal(disc, [[1 / 2, 1], [0 / 2, 1]])
    np.testing.assert_array_equal(cont, [[(0.5 + np.nextafter(0.5, 1.0)) / 2, 1], [0.5 / 2, 1]])


def test_equal_scores_collapse_to_one_row():
    disc, cont = F.roc([0.5, 0.5, 0.5, 0.25], [0.9, 0.0, 0.6, 0.7], 3)
    np.testing.assert_array_equal(disc, [[3 / 3, 1], [2 / 3, 1]])
    np.testing.assert_array_equal(cont, [[(((0.9 + 0.0) + 0.6) + 0.7) / 3, 1], [((0.9 + 0.0) + 0.6) / 3, 1]])


def thousand_file(tmp_path, equal_scores):
    """one face; detection 0 sits on it, 1000 more lie away from it"""
    rows = [[14, 14, 12, 12, 0.9]] + [[60, 60, 10, 10, 0.9 if equal_scores else 0.8 - k * 1e-4] for k in range(1000)]
    ann, det = str(tmp_path / "val_gt.txt"), str(tmp_path / "detection_rect.txt")
    open(ann, "w").write(K.annotation_text(["a/img_1"], [[[5.5, 5.5, 0.0, 20, 20]]]))
    open(det, "w").write(K.detection_text(["a/img_1"], [rows]))
    return det, ann


def test_the_readout_is_the_first_row_under_1000_false_positives(tmp_path):
    res = F.fddb_eval(*thousand_file(tmp_path, equal_scores=False))
    assert res["disc"].shape == (1001, 2)
    assert res["disc"][:2, 1].tolist() == [1000, 999]                     # the lowest threshold still has 1000
    assert res["disc_at_1000"] == 1.0 and res["cont_at_1000"] == (97 / 169 + 0.0 * 999) / 1
    assert F.rate_at(res["disc"], 1000) == res["disc"][1, 0]
    assert F.rate_at(res["disc"], 1) == 1.0 and res["disc"][-1].tolist() == [1.0, 0]


def test_no_row_under_1000_gives_nan_and_a_warning(tmp_path, caplog):
    with caplog.at_level(logging.WARNING):
        res = F.fddb_eval(*thousand_file(tmp_path, equal_scores=True))
    assert res["disc"].tolist() == [[1.0, 1000.0]]
    assert np.isnan(res["disc_at_1000"]) and np.isnan(res["cont_at_1000"])
    assert sum("fewer than 1000" in r.getMessage() for r in caplog.records) == 2
    assert F.result_string(res) == "rect_disc_at_1000: nan, rect_cont_at_1000: nan"
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        empty = F.evaluate(F.Detections([], []), F.Annotations(["a"], [[[5.5, 5.5, 0.0, 20, 20]]]))
    assert empty["disc"].shape == (0, 2) and np.isnan(empty["disc_at_1000"]) and len(caplog.records) == 2


def test_the_roc_files_read_back_with_the_reference_s_expression(tmp_path):
    dets, gt = K.three_images()
    res = F.evaluate(dets, gt, sizes=K.THREE_SIZES)
    paths = F.write_roc(res, str(tmp_path / "out"), prefix="rect_")
    assert [os.path.basename(p) for p in paths] == ["rect_DiscROC.txt", "rect_ContROC.txt"]
    for path, key in zip(paths, ("disc", "cont")):
        with open(path, "r") as f:
            lines = f.readlines()
        back = np.array(list(map(lambda x: x.strip().split(), lines))).astype(float)     # lib/datasets/fddb.py:90-99
        np.testing.assert_array_equal(back, res[key])
        assert back[np.where(back[:, 1] < 1000)[0][0], 0] == res[key + "_at_1000"]


# ---- what neither path takes ---------------------------------------------------------------------------------------------------
def test_an_unbounded_ellipse_without_a_canvas_is_refused_by_name_not_by_memory():
    dets = F.Detections(["a"], [[[14, 14, 12, 12, 0.9]]])
    for ell in ([float("inf"), 5.5, 0.0, 20, 20], [1e7, 1e7, 0.0, 20, 20]):
        gt = F.Annotations(["a"], [[ell]])
        with pytest.raises(ValueError, match="annotation 0 of image 0 has a scan box"):
            F.evaluate(dets, gt)
        with pytest.raises(ValueError, match="for the device"):            # (before any library is loaded)
            F.pair_counts_device(F.geometry(F.align(dets, gt), gt))
    # a canvas cuts the second one to 100 x 100 pixels, all inside the ellipse
    res = F.evaluate(dets, F.Annotations(["a"], [[[1e7, 1e7, 0.0, 20, 20]]]), sizes=[(100, 100)])
    assert res["ann_area"].tolist() == [10000] and res["inter"].tolist() == [169]


def test_the_device_is_not_offered_more_pairs_than_one_launch_holds():
    many = np.tile([[1.0, 1.0, 2.0, 2.0, 0.5]], (8192, 1))
    for n_ann, safe in ((8191, True), (8192, False)):                      # 8192 x 8192 = 2^26 pairs
        gt = F.Annotations(["a"], [np.tile([[2.0, 2.0, 0.0, 5.0, 5.0]], (n_ann, 1))])
        assert F._device_safe(F.geometry([many], gt, [(20, 20)])) is safe


# ---- readers ------------------------------------------------------------------------------------------------------------------
def test_the_readers_read_what_the_writers_wrote(tmp_path):
    dets, gt = K.three_images()
    ann, det = str(tmp_path / "val_gt.txt"), str(tmp_path / "detection_rect.txt")
    open(ann, "w").write(K.annotation_text(gt.names, gt.ellipses))
    boxes = [np.array([[x, y, x + w - 1, y + h - 1, s] for x, y, w, h, s in rr], dtype=np.float64) for rr in K.THREE_ROWS]
    D.write_detections_fddb([n + ".jpg" for n in K.THREE_NAMES], [[[]] * 3, boxes], str(tmp_path))
    assert open(det).read() == K.detection_text(K.THREE_NAMES, K.THREE_ROWS)
    back_gt, back = F.load_annotations(ann), F.load_detections(det)
    assert back_gt.names == gt.names and back.names == dets.names
    for a, b in zip(back_gt.ellipses + back.rows, gt.ellipses + dets.rows):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("text,line", [("a/img_1\n3\n1 2 3 4 0.5\n1 2 3 4 0.5\n", 2),              # a count larger than the rows left
                                       ("a/img_1\n1\n1 2 3 4 0.5\nb/img_2\n1\n1 2 3 4\n", 6),      # a row with four numbers
                                       ("a/img_1\n1\n1 2 3 x 0.5\n", 3), ("a/img_1\nmany\n", 2), ("a/img_1\n", 1)])
def test_malformed_files_raise_naming_the_line(text, line, tmp_path):
    path = str(tmp_path / "bad.txt")
    open(path, "w").write(text)
    with pytest.raises(ValueError, match="line %d:" % line):
        F.load_detections(path)
    with pytest.raises(ValueError, match="line \\d+:"):
        F.load_annotations(path)                                          # (six numbers per row there)


# ---- ImageList and the command line ---------------------------------------------------------------------------------------------
def test_imagelist_evaluates_when_the_annotation_file_is_there(tmp_path, monkeypatch):
    monkeypatch.delenv("SHF_DEVICE_EVAL", raising=False)
    root, paths, all_boxes, dets, gt = K.written_case(tmp_path)
    out = str(tmp_path / "out")
    today = "detections written to {}".format(os.path.join(out, "detections"))
    assert D.ImageList("fddb_val", paths, root=str(root)).evaluate_detections(all_boxes, output_dir=out) == today
    gt_dir = tmp_path / "ground_truth"
    (gt_dir / "FDDB-folds").mkdir(parents=True)
    assert D.ImageList("fddb_val", paths, root=str(root), ground_truth=str(gt_dir)).evaluate_detections(
        all_boxes, output_dir=out) == today
    assert not os.path.exists(os.path.join(out, "detections", "rect_DiscROC.txt"))
    clipped = F.evaluate(dets, gt, sizes=K.THREE_SIZES)
    unclipped = F.evaluate(dets, gt)
    assert clipped["ann_area"][0] == 130 and unclipped["ann_area"][0] == 183
    assert F.result_string(clipped) != F.result_string(unclipped)
    for sub in ("FDDB-folds", ""):
        ann = gt_dir / sub / "val_gt.txt"
        ann.write_text(K.annotation_text(gt.names, gt.ellipses))
        msg = D.ImageList("fddb_val", paths, root=str(root), ground_truth=str(gt_dir)).evaluate_detections(
            all_boxes, output_dir=out)
        assert msg == F.result_string(clipped)
        for fname, key in (("rect_DiscROC.txt", "disc"), ("rect_ContROC.txt", "cont")):
            path = os.path.join(out, "detections", fname)                 # next to detection_rect.txt
            np.testing.assert_array_equal(np.loadtxt(path).reshape(-1, 2), clipped[key])
            os.remove(path)
    # without the image files the masks are not clipped
    msg = D.ImageList("fddb_val", paths, root=str(tmp_path / "nowhere"), ground_truth=str(gt_dir)).evaluate_detections(
        all_boxes, output_dir=out)
    assert msg == F.result_string(unclipped)
    # another dataset's list is not touched by the file
    assert D.ImageList("wider_val", ["0--Parade/x.jpg"], ground_truth=str(gt_dir)).evaluate_detections(
        [[[]], [np.zeros((0, 5))]], output_dir=out) == today


def test_the_module_cli_prints_the_reference_s_string_and_writes_both_files(tmp_path):
    root, paths, all_boxes, dets, gt = K.written_case(tmp_path)
    D.write_detections_fddb(paths, all_boxes, str(tmp_path))
    det_file, ann = str(tmp_path / "detection_rect.txt"), str(tmp_path / "val_gt.txt")
    open(ann, "w").write(K.annotation_text(gt.names, gt.ellipses))
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("SHF_DEVICE_EVAL", None)

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "smallhardface_amd.fddb_eval"] + list(args), cwd=str(tmp_path),
                              env=env, capture_output=True, text=True, check=True).stdout
    clipped = F.evaluate(dets, gt, sizes=K.THREE_SIZES)
    assert cli("--ann", ann, det_file) == F.result_string(F.evaluate(dets, gt)) + "\n"
    assert cli("--ann", ann, "--images", str(root), "--out", str(tmp_path / "roc"), det_file) == \
        F.result_string(clipped) + "\n"
    np.testing.assert_array_equal(np.loadtxt(str(tmp_path / "roc" / "rect_DiscROC.txt")).reshape(-1, 2), clipped["disc"])
    np.testing.assert_array_equal(np.loadtxt(str(tmp_path / "roc" / "rect_ContROC.txt")).reshape(-1, 2), clipped["cont"])
