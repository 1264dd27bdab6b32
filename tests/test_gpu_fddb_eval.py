"""The device path of the FDDB evaluator (shf_fddb_pair_counts, csrc/eval.hip) against the unchanged host functions.

The device returns integers (per pair the intersection count, per annotation its area), so every comparison is
``assert_array_equal`` against ``pair_counts_host``, and ``evaluate(device=True)`` is held to ``evaluate()`` on every curve
value.  Sweep widths cross the 64 lanes of the wave that owns a pair (1, 63, 64, 65, 130; heights 1 and 70), detections per
image run 0, 1, 64, 65, annotations 0, 1, 3, and one call holds 1 image or 70."""
import ctypes as C
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from smallhardface_amd import _lib
from smallhardface_amd import fddb_eval as F
from tests import fddb_eval_cases as K

pytestmark = pytest.mark.gpu
PI = K.PI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_counts(geom):
    """device == host on every integer array"""
    want = F.pair_counts_host(geom)
    got = F.pair_counts_device(geom)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    return want


def check_evaluate(dets, gt, sizes):
    want = F.evaluate(dets, gt, sizes=sizes)
    got = F.evaluate(dets, gt, sizes=sizes, device=True)
    for k in ("inter", "ann_area", "det_area", "m", "disc", "cont"):
        np.testing.assert_array_equal(got[k], want[k])
    assert got["pairs"] == want["pairs"] and got["N"] == want["N"]
    assert np.array_equal([got["disc_at_1000"], got["cont_at_1000"]], [want["disc_at_1000"], want["cont_at_1000"]],
                          equal_nan=True)
    return want


# ---- the hand-derived counts, through the device ------------------------------------------------------------------------------
def test_the_hand_derived_counts():
    dev = F.pair_counts_device
    for r, pixels in [(1, 5), (2, 13), (3, 29), (4, 49), (5, 81), (10, 317)]:
        assert K.single([r, r, 0.0, 50, 50], counts=dev)[1] == pixels
    for angle in (0.0, PI / 4, PI / 2, 1.0):
        assert K.single([5.5, 5.5, angle, 50, 50], counts=dev)[1] == 97
    assert K.single([5, 5, PI / 2, 50, 50], counts=dev)[1] == 77
    inter, area, det_area = K.single([5.5, 5.5, 0.0, 20, 20], rows=[[14, 14, 12, 12, 0.9]], counts=dev)
    assert (inter.tolist(), area, det_area.tolist()) == ([97], 97, [169])
    for angle, inside, cut in [(0.0, 183, 130), (PI / 2, 183, 159)]:
        assert K.single([10.5, 5.5, angle, 30, 30], size=(100, 100), counts=dev)[1] == inside
        assert K.single([10.5, 5.5, angle, 3, 30], size=(100, 100), counts=dev)[1] == cut
    inter, area, _ = K.single([0.3, 0.3, 0.0, 10.5, 10.5], rows=[[9, 9, 3, 3, 0.9]], counts=dev)
    assert inter.tolist() == [0] and area == 0                            # smaller than a pixel, between pixel centres


def test_the_three_image_file():
    dets, gt = K.three_images()
    res = check_evaluate(dets, gt, K.THREE_SIZES)
    assert res["inter"].tolist() == [97, 0, 183, 183, 13, 0] and res["ann_area"].tolist() == [97, 183, 13, 29]


# ---- sweep widths and heights across the 64 lanes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("height", [1, 70])
@pytest.mark.parametrize("width", [1, 63, 64, 65, 130])
def test_scan_box_widths_and_heights(width, height):
    """an ellipse larger than the canvas: its scan box IS the width x height canvas; the rectangles cut the sweep to
    every narrower width of the list as well"""
    ells = [[[150.0, 120.0, 0.3, width / 2.0, height / 2.0], [width / 2.0 + 0.25, height / 3.0 + 0.5, -1.2, width / 2.0, height / 2.0]]]
    rows = [[[-5, -5, 300, 300, 0.9]] + [[3, 0, w - 1, height, 0.8] for w in (1, 63, 64, 65, 130)] +
            [[0.5, height / 2.0, width, 0, 0.7]]]
    geom, _ = K.geom_of(ells, rows, [(width, height)])
    box = geom["ell_box"][0]
    assert (box[2] - box[0] + 1, box[3] - box[1] + 1) == (width, height)
    inter, ann_area, det_area = check_counts(geom)
    assert det_area[0] == width * height and inter[0] == ann_area[0] > 0


def test_unclipped_scan_boxes_of_every_width():
    """without a canvas: circles whose own scan boxes are 63, 64, 65 and 130 pixels wide"""
    ells = [[29.5, 29.5, 0.0, 40.0, 50.0], [30.25, 30.25, 0.0, 40.5, 50.0], [30.5, 30.5, 0.0, 40.0, 50.0],
            [63.25, 63.25, 0.0, 70.5, 50.0]]
    geom, _ = K.geom_of([ells], [[[0, 0, 200, 200, 0.9], [30, 40, 20, 3, 0.5]]])
    widths = (geom["ell_box"][:, 2] - geom["ell_box"][:, 0] + 1).tolist()
    assert widths == [63, 64, 65, 130], widths
    check_counts(geom)


# ---- clipping, angles, degenerate shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cx,cy", [(3, 30), (97, 30), (50, 2), (50, 58), (2, 3), (98, 57)],
                         ids=["left", "right", "top", "bottom", "top-left", "bottom-right"])
@pytest.mark.parametrize("angle", [0.0, PI / 2, -PI / 2, PI / 4, -1.2])
def test_clipping_on_every_side_at_every_angle(cx, cy, angle):
    ell = [10.5, 5.5, angle, cx, cy]
    rows = [[cx - 12, cy - 12, 24, 24, 0.9], [cx - 3, cy - 20, 40, 25, 0.8], [cx - 30, cy + 2, 28, 3, 0.7]]
    geom, _ = K.geom_of([[ell, [7.5, 7.5, angle, cx, cy]]], [rows], [(100, 60)])
    inter, ann_area, _ = check_counts(geom)
    free = K.single(ell)[1]
    assert 0 < ann_area[0] < free                                         # the canvas cuts pixels off


def test_the_unclipped_mode_with_negative_coordinates():
    ells = [[[10.5, 5.5, 0.4, -30.0, -12.0], [5.5, 5.5, 0.0, 2.0, -3.0]]]
    rows = [[[-45, -20, 30, 16, 0.9], [-4, -9, 12, 12, 0.8], [-100, -100, 5, 5, 0.7], [5, 5, 10, 10, 0.6]]]
    geom, _ = K.geom_of(ells, rows)
    inter, ann_area, _ = check_counts(geom)
    assert ann_area[1] == 97 and inter.reshape(2, 4)[1, 1] == 97 and inter.reshape(2, 4)[0, 0] == ann_area[0] > 100


# ---- counts per image, images per call ------------------------------------------------------------------------------------------
def test_detection_and_annotation_counts_per_image():
    """annotations {0, 1, 3} x detections {0, 1, 64, 65}: 12 images in one call"""
    shapes = [(a, d) for a in (0, 1, 3) for d in (0, 1, 64, 65)]
    dets, gt, sizes = K.batch(11, shapes, angles=[0.0, PI / 2, -PI / 2, PI / 4, -1.2])
    res = check_evaluate(dets, gt, sizes)
    assert res["N"] == 16 and (res["m"] > 0.5).any() and (res["inter"] == 0).any()
    check_evaluate(dets, gt, None)                                        # the same shapes without a canvas


@pytest.mark.parametrize("shape", [(0, 1), (1, 0), (1, 1), (3, 65)], ids=str)
def test_one_image_in_one_call(shape):
    dets, gt, sizes = K.batch(13, [shape])
    check_evaluate(dets, gt, sizes)


def test_seventy_images_in_one_call():
    rng = np.random.default_rng(17)
    shapes = [(int(rng.integers(0, 4)), int(rng.integers(0, 12))) for _ in range(70)]
    dets, gt, sizes = K.batch(19, shapes)
    res = check_evaluate(dets, gt, sizes)
    assert res["disc"].shape[0] > 10


# ---- refusals: argument checks only -----------------------------------------------------------------------------------------
def raw_call(ann_off, det_off, box=(10, 10, 30, 30), rect=(12, 12, 28, 28), null=()):
    """the C entry point on dummy one-row arrays: a refused call reads no further than what it checks"""
    lib = _lib.load()
    ell = np.array([[5.5, 5.5, 1.0, 0.0, 20.0, 20.0]])
    ell_box, rect4 = np.array([box], dtype=np.int32), np.array([rect], dtype=np.int32)
    ao, do = np.array(ann_off, dtype=np.int64), np.array(det_off, dtype=np.int64)
    inter, area = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int)
    args = dict(ell=ell.ctypes.data_as(dp), ell_box=ell_box.ctypes.data_as(ip), ann_off=ao.ctypes.data_as(lp),
                rect=rect4.ctypes.data_as(ip), det_off=do.ctypes.data_as(lp), inter=inter.ctypes.data_as(ip),
                area=area.ctypes.data_as(ip))
    for k in null:
        args[k] = None
    rc = lib.shf_fddb_pair_counts(args["ell"], args["ell_box"], args["ann_off"], args["rect"], args["det_off"],
                                  len(ao) - 1, args["inter"], args["area"], None)
    return rc, _lib.last_error(), inter, area


REFUSED = [
    ("negative offset", dict(ann_off=[0, -1], det_off=[0, 1]), "negative offset in ann_off"),
    ("negative det offset", dict(ann_off=[0, 1], det_off=[-2, 1]), "negative offset in det_off"),
    ("non-monotone", dict(ann_off=[0, 1, 0], det_off=[0, 1, 1]), "non-monotone offsets in ann_off"),
    ("non-monotone det", dict(ann_off=[0, 1, 1], det_off=[0, 1, 0]), "non-monotone offsets in det_off"),
    ("offsets from 1", dict(ann_off=[1, 2], det_off=[0, 1]), "offsets must start at 0"),
    ("2^31 rows", dict(ann_off=[0, 2 ** 31], det_off=[0, 1]), "2^31 rows or more"),
    ("2^31 det rows", dict(ann_off=[0, 1, 1], det_off=[0, 4096, 2 ** 31]), "2^31 rows or more"),
    ("2^31 pairs", dict(ann_off=[0, 2 ** 16], det_off=[0, 2 ** 15]), "2^26 (annotation, detection) pairs or more"),
    ("2^26 pairs", dict(ann_off=[0, 2 ** 13], det_off=[0, 2 ** 13]), "2^26 (annotation, detection) pairs or more"),
    ("2^26 pairs over two images", dict(ann_off=[0, 2 ** 12, 2 ** 13], det_off=[0, 2 ** 13, 2 ** 14]),
     "2^26 (annotation, detection) pairs or more"),
    ("null offsets", dict(ann_off=[0, 1], det_off=[0, 1], null=("ann_off",)), "null offsets"),
    ("null ellipses", dict(ann_off=[0, 1], det_off=[0, 1], null=("ell",)), "null shape or output array"),
    ("null boxes", dict(ann_off=[0, 1], det_off=[0, 1], null=("ell_box",)), "null shape or output array"),
    ("null rectangles", dict(ann_off=[0, 1], det_off=[0, 1], null=("rect",)), "null shape or output array"),
    ("null counts", dict(ann_off=[0, 1], det_off=[0, 1], null=("inter",)), "null shape or output array"),
    ("null areas", dict(ann_off=[0, 1], det_off=[0, 1], null=("area",)), "null shape or output array"),
    ("box over the cap", dict(ann_off=[0, 1], det_off=[0, 1], box=(0, 0, 1024, 1023)), "the cap is 1048576"),
    ("huge corner", dict(ann_off=[0, 1], det_off=[0, 1], box=(0, 0, 2 ** 30, 0)), "2^30 or more in magnitude"),
    ("huge rectangle corner", dict(ann_off=[0, 1], det_off=[0, 1], rect=(-2 ** 30, 0, 5, 5)), "2^30 or more in magnitude"),
]


@pytest.mark.parametrize("name,args,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_bad_arguments_are_refused_and_the_next_call_is_right(name, args, msg):
    rc, err, inter, area = raw_call(**args)
    assert rc != 0 and msg in err, (rc, err)
    assert inter.tolist() == [-7] and area.tolist() == [-7]              # nothing ran: the outputs are untouched
    rc, _, inter, area = raw_call([0, 1], [0, 1])
    assert rc == 0 and inter.tolist() == [97] and area.tolist() == [97]


def test_a_box_at_the_cap_passes_and_calls_without_work_return_at_once():
    rc, err, inter, area = raw_call([0, 1], [0, 1], box=(0, 0, 1023, 1023), rect=(0, 0, 1023, 1023))
    assert rc == 0 and inter.tolist() == [97] and area.tolist() == [97], err     # 2^20 pixels, 97 of them inside
    rc, _, inter, area = raw_call([0, 1], [0, 0])                        # no detections: the area alone
    assert rc == 0 and inter.tolist() == [-7] and area.tolist() == [97]
    rc, _, inter, area = raw_call([0, 0], [0, 1])                        # no annotations: nothing to count
    assert rc == 0 and inter.tolist() == [-7] and area.tolist() == [-7]
    rc, _, inter, area = raw_call([0], [0])                              # no images
    assert rc == 0 and inter.tolist() == [-7]


# ---- fallback -------------------------------------------------------------------------------------------------------------
def test_huge_or_non_finite_shapes_take_the_host_path_with_a_warning(caplog):
    dets = F.Detections(["a"], [[[14, 14, 12, 12, 0.9]]])
    for ell in ([600.0, 600.0, 0.0, 20, 20], [5.5, float("nan"), 0.0, 20, 20]):          # over the cap unclipped; NaN
        gt = F.Annotations(["a"], [[ell]])
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            got = F.evaluate(dets, gt, device=True)
        assert any("host" in r.getMessage() for r in caplog.records)
        want = F.evaluate(dets, gt)
        np.testing.assert_array_equal(got["inter"], want["inter"])
        np.testing.assert_array_equal(got["disc"], want["disc"])
    # clipped to a canvas the large ellipse fits the cap again and runs on the device
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        check_evaluate(dets, F.Annotations(["a"], [[[600.0, 600.0, 0.0, 20, 20]]]), [(100, 100)])
    assert not any("host" in r.getMessage() for r in caplog.records)


# ---- the command line under SHF_DEVICE_EVAL=1 ---------------------------------------------------------------------------------
def test_the_module_cli_prints_and_writes_the_same_bytes_on_the_device(tmp_path):
    """two fresh child processes on the same files, one with the switch set: the same stdout, the same two ROC files"""
    from smallhardface_amd import datasets as D
    root, paths, all_boxes, dets, gt = K.written_case(tmp_path)
    D.write_detections_fddb(paths, all_boxes, str(tmp_path))
    ann = str(tmp_path / "val_gt.txt")
    open(ann, "w").write(K.annotation_text(gt.names, gt.ellipses))
    out = {}
    for leg, switch in (("host", None), ("device", "1")):
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("SHF_DEVICE_EVAL", None)
        if switch:
            env["SHF_DEVICE_EVAL"] = switch
        run = subprocess.run([sys.executable, "-m", "smallhardface_amd.fddb_eval", "--ann", ann, "--images", str(root),
                              "--out", str(tmp_path / leg), str(tmp_path / "detection_rect.txt")], cwd=str(tmp_path),
                             env=env, capture_output=True, check=True, timeout=120)
        out[leg] = (run.stdout, open(str(tmp_path / leg / "rect_DiscROC.txt"), "rb").read(),
                    open(str(tmp_path / leg / "rect_ContROC.txt"), "rb").read())
    assert out["device"] == out["host"]
    assert out["host"][0].decode() == F.result_string(F.evaluate(dets, gt, sizes=K.THREE_SIZES)) + "\n"
    assert len(out["host"][1]) > 0 and len(out["host"][2]) > 0
