"""Builders for the FDDB evaluator's tests (tests/test_fddb_eval.py on the host, tests/test_gpu_fddb_eval.py on the device)
and for tools/bench_fddb_eval.py: single shapes, the hand-derived three-image file, file texts, and seeded random sets."""
import numpy as np

from smallhardface_amd import fddb_eval as F

PI = float(np.pi)


def geom_of(ellipses, rows, sizes=None):
    """per image a list of ``ra rb angle cx cy`` rows and a list of ``x y w h score`` rows -> (geometry, Annotations)"""
    names = ["img_%d" % i for i in range(len(ellipses))]
    gt = F.Annotations(names, ellipses)
    rows = [np.array(r, dtype=np.float64).reshape(-1, 5) for r in rows]
    return F.geometry(rows, gt, sizes), gt


def single(ellipse, rows=(), size=None, counts=F.pair_counts_host):
    """one ellipse against some rectangles: (inter (D,), area of the ellipse, areas of the rectangles (D,))"""
    geom, _ = geom_of([[ellipse]], [list(rows)], None if size is None else [size])
    inter, ann_area, det_area = counts(geom)
    return inter, int(ann_area[0]), det_area


def annotation_text(names, ellipses):
    out = []
    for n, ell in zip(names, ellipses):
        out.append("%s\n%d\n" % (n, len(ell)))
        for e in ell:
            out.append("%r %r %r %r %r  1\n" % tuple(float(v) for v in e))        # (FDDB writes two spaces there)
    return "".join(out)


def detection_text(names, rows):
    out = []
    for n, rr in zip(names, rows):
        out.append("%s\n%d\n" % (n, len(rr)))
        for r in rr:
            out.append("{:.3f} {:.3f} {:.3f} {:.3f} {:.10f}\n".format(*r))
    return "".join(out)


# ---- the three-image file whose ROC is written out by hand in tests/test_fddb_eval.py ------------------------------------
THREE_NAMES = ["2002/07/19/big/img_1", "2002/07/19/big/img_2", "2002/07/20/big/img_3"]
THREE_SIZES = [(100, 100)] * 3
THREE_ELLIPSES = [
    [[5.5, 5.5, 0.0, 20.0, 20.0]],                                    # 97 pixels
    [[10.5, 5.5, 0.0, 30.0, 30.0]],                                   # 183 pixels
    [[2.0, 2.0, 0.0, 10.0, 10.0], [3.0, 3.0, 0.0, 30.0, 30.0]],       # 13 and 29 pixels
]
THREE_ROWS = [
    [[14, 14, 12, 12, 0.9],          # 13 x 13 = 169 pixels over the whole circle: S = 97/169, a discrete hit
     [60, 60, 10, 10, 0.8]],         # away from it: S = 0
    [[19, 24, 22, 12, 0.8],          # 23 x 13 = 299 pixels over the whole ellipse: S = 183/299, the assignment's choice
     [19, 24, 22, 30, 0.7]],         # 23 x 31 = 713 pixels over it as well: S = 183/713, left without a face
    [[8, 8, 4, 4, 0.95]],            # 5 x 5 = 25 pixels over the radius-2 circle: S = 13/25; the other face is missed
]


def three_images():
    return F.Detections(THREE_NAMES, THREE_ROWS), F.Annotations(THREE_NAMES, THREE_ELLIPSES)


def written_case(tmp_path):
    """the three-image case with its first face moved to the left edge, as image files + an annotation file"""
    from PIL import Image
    ells = [[[10.5, 5.5, 0.0, 3.0, 30.0]]] + THREE_ELLIPSES[1:]
    rows = [[[-8, 24, 22, 12, 0.9], [60, 60, 10, 10, 0.8]]] + THREE_ROWS[1:]
    root = tmp_path / "data"
    for n, (w, h) in zip(THREE_NAMES, THREE_SIZES):
        (root / n).parent.mkdir(parents=True, exist_ok=True)
        Image.new("RGB", (w, h)).save(str(root / (n + ".jpg")))
    paths = [n + ".jpg" for n in THREE_NAMES]
    boxes = [np.array([[x, y, x + w - 1, y + h - 1, s] for x, y, w, h, s in rr], dtype=np.float64) for rr in rows]
    return root, paths, [[[]] * 3, boxes], F.Detections(THREE_NAMES, rows), F.Annotations(THREE_NAMES, ells)


# ---- seeded random sets ---------------------------------------------------------------------------------------------------
def random_image(rng, n_ann, n_det, size=(120, 90), angles=None):
    """``n_ann`` ellipses in and around the canvas and ``n_det`` rectangles, about half of them drawn around an ellipse"""
    W, H = size
    ell = []
    for k in range(n_ann):
        ra = rng.uniform(4, 40)
        ang = angles[k % len(angles)] if angles else rng.uniform(-PI / 2, PI / 2)
        ell.append([ra, ra * rng.uniform(0.4, 1.0), ang, rng.uniform(-10, W + 10), rng.uniform(-10, H + 10)])
    rows = []
    for k in range(n_det):
        if n_ann and k % 2 == 0:
            e = ell[rng.integers(n_ann)]
            w, h = 2 * e[1] * rng.uniform(0.7, 1.4), 2 * e[0] * rng.uniform(0.7, 1.4)
            x, y = e[3] - w / 2 + rng.uniform(-6, 6), e[4] - h / 2 + rng.uniform(-6, 6)
        else:
            w, h = rng.uniform(3, 60), rng.uniform(3, 60)
            x, y = rng.uniform(-20, W), rng.uniform(-20, H)
        rows.append([round(x, 3), round(y, 3), round(w, 3), round(h, 3), round(float(rng.uniform(0.05, 1.0)), 2)])
    return ell, rows


def batch(seed, shapes, size=(120, 90), angles=None):
    """``shapes``: per image (annotations, detections) -> (Detections, Annotations, sizes)"""
    rng = np.random.default_rng(seed)
    names = ["img_%d" % i for i in range(len(shapes))]
    ells, rows = [], []
    for n_ann, n_det in shapes:
        e, r = random_image(rng, n_ann, n_det, size, angles)
        ells.append(e)
        rows.append(r)
    return F.Detections(names, rows), F.Annotations(names, ells), [size] * len(shapes)


def fddb_sized_set(seed=2845, n_images=2845, n_faces=5171, dets_per_image=(20, 90)):
    """A SYNTHETIC set of FDDB's size: ``n_images`` images of 300..450 pixels a side, ``n_faces`` upright-ish ellipses
    spread over them (every image at least one), and per image detections drawn around and away from them."""
    rng = np.random.default_rng(seed)
    per = np.ones(n_images, dtype=np.int64)
    np.add.at(per, rng.integers(0, n_images, n_faces - n_images), 1)
    names, ells, rows, sizes = [], [], [], []
    for i in range(n_images):
        W, H = int(rng.integers(300, 451)), int(rng.integers(300, 451))
        ell = []
        for _ in range(per[i]):
            ra = rng.uniform(15, 90)
            ell.append([ra, ra * rng.uniform(0.55, 0.8), PI / 2 + rng.uniform(-0.4, 0.4), rng.uniform(0, W), rng.uniform(0, H)])
        rr = []
        for k in range(int(rng.integers(*dets_per_image))):
            if k % 3 != 2:
                e = ell[rng.integers(len(ell))]
                w, h = 2 * e[1] * rng.uniform(0.6, 1.5), 2 * e[0] * rng.uniform(0.6, 1.5)
                x, y = e[3] - w / 2 + rng.uniform(-15, 15), e[4] - h / 2 + rng.uniform(-15, 15)
            else:
                w, h = rng.uniform(8, 150), rng.uniform(8, 150)
                x, y = rng.uniform(-10, W - 10), rng.uniform(-10, H - 10)
            rr.append([round(x, 3), round(y, 3), round(w, 3), round(h, 3), round(float(rng.uniform(0.05, 1.0)), 4)])
        names.append("img_%d" % i)
        ells.append(ell)
        rows.append(rr)
        sizes.append((W, H))
    return F.Detections(names, rows), F.Annotations(names, ells), sizes
