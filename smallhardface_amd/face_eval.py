"""AFW / Pascal Faces evaluation (AP) of a written ``afw_res.txt`` / ``pascal_res.txt``.

What the reference's README sends the user to after ``test_net`` for these two imdbs:
external/marcopede-face-eval-f2870fd85d48/plot_AP.py (citations below are relative to that directory).  Semantics kept
exactly, because they decide the published AP numbers:

  * detections are ``name score x1 y1 x2 y2`` lines, keyed by ``name.split('.')[0]`` and ordered stably by falling score
    (loadData.py:82-97); ``filterdet`` keeps a row whose width OR height exceeds ``minpix = int(sqrt(0.5 * minw * minh))``
    (VOCpr.py:234-247, plot_AP.py:25-35);
  * a ground-truth box is "difficult" when its annotation says so or when ``|x1 - x2| < minw`` or ``|y1 - y2| < minh``
    (database.py:510-516, 590-596); images without boxes do not take part, ``tot`` counts the non-difficult boxes
    (VOCpr.py:103-110);
  * matching in global score order (VOCprRecordOptim, VOCpr.py:118-162): IoU is util.overlap (util.py:176-193: +1 on
    abs() extents, a strict ``>`` intersection test, ``ia / float(a1 + a2 - ia)``), the best box is chosen with
    ``covr >= maxovr`` (the LAST of equal maxima), a detection is a true positive when ``maxovr > ovr`` (strict) on a
    box that is neither difficult nor taken, a false positive when the box is taken or ``maxovr <= ovr``, and neither on a
    difficult box;
  * ``iters`` rounds of box refinement (evaluate_optim, VOCpr.py:264-289): the numpy.mean of the true positives'
    translations and scales moves every detection (transf_dets, :250-259); the curve is the last round's.  A round
    without a true positive leaves NaN means and NaN boxes, as there;
  * cumulative precision / recall with their 0 / 0 = NaN, ``VOCap`` with Python's ``max`` (NaN on the left stays) and the
    11-point ``VOColdap`` (drawPrfast, VOCap, VOColdap, :191-231).

No plotting and no "point" methods.  The structures are in memory (``Detections``, ``FaceGT``) with separate readers.

The default path is host numpy.  ``evaluate(..., device=True)`` runs the matching -- every round x every detection x its
image's boxes -- on the GPU (``shf_face_eval_match``, csrc/eval.hip).  The device returns integers only (per detection a
code and the chosen box); translations, means, the transform, the cumulative sums and the AP are formed on the host from
them, so the result is the host path's bit for bit.
"""
import ctypes as C
import logging
import os
import warnings

import numpy as np

NEITHER, TRUE_POSITIVE, FALSE_POSITIVE = 0, 1, 2      # the per-detection codes of a matching round
ANNOTATION_FILES = {'AFW': 'new_annotations_AFW.mat', 'PASCAL': 'Annotations_Face_PASCALLayout_large_fixed.mat'}
_FINITE_BOUND = 1e150        # below it no product or sum of the IoU can overflow to inf (and inf / inf to NaN)


class Detections(object):
    """``names[i]`` the image key, ``rows[i]`` = (score, x1, y1, x2, y2) of detection i, float64."""

    def __init__(self, names, rows):
        self.names = list(names)
        self.rows = np.array(rows, dtype=np.float64).reshape(-1, 5)
        if len(self.names) != self.rows.shape[0]:
            raise ValueError('Detections: %d names for %d rows' % (len(self.names), self.rows.shape[0]))

    def __len__(self):
        return len(self.names)

    def take(self, idx):
        return Detections([self.names[i] for i in idx], self.rows[idx])

    def sorted_by_score(self):
        """Falling score, equal scores in their given order (``sorted(..., reverse=True)`` and ``list.sort`` are stable)."""
        return self.take(np.argsort(-self.rows[:, 0], kind='stable'))


class FaceGT(object):
    """Per image its key, (k, 4) x1-y1-x2-y2 boxes and the (k,) difficult flags (after the minw / minh rule)."""

    def __init__(self, names, boxes, difficult):
        self.names = list(names)
        self.boxes = [np.array(b, dtype=np.float64).reshape(-1, 4) for b in boxes]
        self.difficult = [np.array(d).reshape(-1) != 0 for d in difficult]

    def __len__(self):
        return len(self.names)


def image_key(name):
    return str(name).split('/')[-1].split('.')[0]


def min_pixels(minw=30, minh=30):
    return int(np.sqrt(0.5 * minw * minh))


# ---- readers ----------------------------------------------------------------------------------------------------------
def load_detections(path):
    """``name score x1 y1 x2 y2`` per line (loadData.py:82-97; what datasets.write_detections_afw / _pascal write) ->
    Detections ordered by falling score."""
    names, rows = [], []
    with open(path) as f:
        for line in f.readlines():
            dd = line.strip().split(' ')
            names.append(dd[0].split('.')[0])
            rows.append([float(dd[1]), float(dd[2]), float(dd[3]), float(dd[4]), float(dd[5])])
    return Detections(names, rows).sorted_by_score()


def filter_detections(dets, minpix):
    """filterdet (VOCpr.py:234-247): rows with width > minpix or height > minpix."""
    r = dets.rows
    with np.errstate(invalid='ignore'):
        keep = ((r[:, 3] - r[:, 1]) > minpix) | ((r[:, 4] - r[:, 2]) > minpix)
    return dets.take(np.nonzero(keep)[0])


def make_gt(names, objects, minw=30, minh=30, four_columns_ok=True):
    """Per image a (k, 6) ``x1 y1 x2 y2 _ difficult`` or (k, 4) matrix -> FaceGT with the size rule applied
    (database.py:505-517, 582-597).  A four-column matrix has no difficult boxes (the Pascal class accepts it, :586-588;
    the AFW class does not)."""
    boxes, diff = [], []
    for obj in objects:
        o = np.asarray(obj, dtype=np.float64)
        o = o.reshape(0, 6) if o.size == 0 else o.reshape(o.shape[0], -1)
        if o.shape[1] < 6:
            if not four_columns_ok:
                raise ValueError('annotation rows with fewer than six columns')
            o = np.hstack([o[:, :4], np.zeros((o.shape[0], 2))])
        b = o[:, :4]
        d = (o[:, 5] != 0) | (np.abs(b[:, 0] - b[:, 2]) < minw) | (np.abs(b[:, 1] - b[:, 3]) < minh)
        boxes.append(b)
        diff.append(d)
    return FaceGT([str(n) for n in names], boxes, diff)


def load_annotations_mat(path, minw=30, minh=30, dataset='PASCAL'):
    """``new_annotations_AFW.mat`` / ``Annotations_Face_PASCALLayout_large_fixed.mat`` -> FaceGT.

    The annotation files are not distributed with the reference; this reader is pinned to the index chain of
    database.py:455-517 and :534-597 only: ``loadmat(path)['Annotations']`` is a struct array, image i's name is
    ``ann[i]['imgname'][0][0]`` and its boxes ``ann[i]['objects'][0]``, a k x 6 (``x1 y1 x2 y2 _ difficult``) or, for
    Pascal, k x 4 matrix."""
    from scipy.io import loadmat
    ann = loadmat(path)['Annotations']
    names, objects = [], []
    for i in range(len(ann)):
        names.append(str(ann[i]['imgname'][0][0]))
        objects.append(ann[i]['objects'][0])
    return make_gt(names, objects, minw, minh, four_columns_ok=(dataset != 'AFW'))


# ---- one matching round -------------------------------------------------------------------------------------------------
def group_by_image(dets, gt):
    """The flat arrays of a matching round.  Images in play: the ground-truth images with a non-empty box list, the last
    of equal keys (the reference fills a dict, VOCpr.py:103-107), plus one box-less image for all the detections whose
    key is not among them.  Returns a dict: ``perm`` (detections grouped by image, the global order kept within an
    image), ``det_off`` / ``gt_off`` (I + 1) int64, ``gt4`` (G, 4) x1-y1-x2-y2, ``difficult`` (G,) uint8, ``tot``."""
    slot, tot = {}, 0
    for j in range(len(gt)):
        if gt.boxes[j].shape[0]:
            slot[image_key(gt.names[j])] = j
            tot += int((~gt.difficult[j]).sum())
    order = sorted(slot.values())
    image_of = {j: i for i, j in enumerate(order)}
    n_img = len(order) + 1                         # the last image collects the detections without ground truth
    img = np.array([image_of[slot[n]] if n in slot else n_img - 1 for n in dets.names], dtype=np.int64).reshape(-1)
    perm = np.argsort(img, kind='stable')
    det_off = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum(np.bincount(img, minlength=n_img), out=det_off[1:])
    gt_off = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([gt.boxes[j].shape[0] for j in order] + [0], out=gt_off[1:])
    gt4 = np.concatenate([gt.boxes[j] for j in order] + [np.zeros((0, 4))], axis=0)
    difficult = np.concatenate([gt.difficult[j] for j in order] + [np.zeros(0, dtype=bool)]).astype(np.uint8)
    return dict(perm=perm, det_off=det_off, gt_off=gt_off, gt4=np.ascontiguousarray(gt4), difficult=difficult, tot=tot)


def overlaps(det4, gt4):
    """util.overlap (util.py:176-193) of every detection with every box: (n, 4) x (k, 4) x1-y1-x2-y2 -> (n, k) float64,
    each element in the operation order of the scalar function."""
    dx1, dy1, dx2, dy2 = (det4[:, c][:, None] for c in range(4))
    gx1, gy1, gx2, gy2 = (gt4[:, c][None, :] for c in range(4))
    a1 = (np.abs(dx1 - dx2) + 1) * (np.abs(dy1 - dy2) + 1)
    a2 = (np.abs(gx1 - gx2) + 1) * (np.abs(gy1 - gy2) + 1)
    meet = (dy2 > gy1) & (gy2 > dy1) & (dx2 > gx1) & (gx2 > dx1)
    ia = (np.minimum(dx2, gx2) - np.maximum(dx1, gx1) + 1) * (np.minimum(dy2, gy2) - np.maximum(dy1, gy1) + 1)
    ia = np.where(meet, ia, 0.0)
    return ia / (a1 + a2 - ia)


def best_boxes(covr):
    """The ``covr >= maxovr`` walk of VOCpr.py:125-134 over each row at once: (maxovr, index).  The running maximum
    starts at 0 and a NaN never passes ``>=``, so the walk ends on the LAST index holding max(0, the row's largest
    non-NaN value), and on index 0 with maxovr 0 when no element reaches that."""
    c = np.where(np.isnan(covr), -np.inf, covr)
    top = np.maximum(c.max(axis=1), 0.0)
    eq = c == top[:, None]
    last = covr.shape[1] - 1 - np.argmax(eq[:, ::-1], axis=1)
    found = eq.any(axis=1)
    return np.where(found, top, 0.0), np.where(found, last, 0)


def match_host(det4, flat, ovr):
    """One round on the host.  ``det4`` (N, 4) x1-y1-x2-y2 grouped as ``flat`` says.  Returns (code, index) int32: per
    detection NEITHER / TRUE_POSITIVE / FALSE_POSITIVE and the chosen box's index within its image, -1 for an image
    without boxes."""
    n = det4.shape[0]
    code = np.full(n, FALSE_POSITIVE, dtype=np.int32)
    index = np.full(n, -1, dtype=np.int32)
    det_off, gt_off = flat['det_off'], flat['gt_off']
    with np.errstate(all='ignore'):
        for i in range(len(det_off) - 1):
            h0, h1, g0, g1 = det_off[i], det_off[i + 1], gt_off[i], gt_off[i + 1]
            if h0 == h1 or g0 == g1:
                continue
            maxovr, gi = best_boxes(overlaps(det4[h0:h1], flat['gt4'][g0:g1]))
            index[h0:h1] = gi
            hard = flat['difficult'][g0:g1] != 0
            taken = np.zeros(g1 - g0, dtype=bool)
            for h in np.nonzero(maxovr > ovr)[0]:
                g = gi[h]
                if hard[g]:
                    code[h0 + h] = NEITHER
                elif not taken[g]:
                    taken[g] = True
                    code[h0 + h] = TRUE_POSITIVE
    return code, index


def match_device(det4, flat, ovr):
    """The same round through ``shf_face_eval_match`` (ShfError without the library or a GPU)."""
    from . import _lib
    lib = _lib.load()
    det4 = np.ascontiguousarray(det4, dtype=np.float64)
    gt4 = np.ascontiguousarray(flat['gt4'], dtype=np.float64)
    det_off = np.ascontiguousarray(flat['det_off'], dtype=np.int64)
    gt_off = np.ascontiguousarray(flat['gt_off'], dtype=np.int64)
    difficult = np.ascontiguousarray(flat['difficult'], dtype=np.uint8)
    code = np.zeros(det4.shape[0], dtype=np.int32)
    index = np.zeros(det4.shape[0], dtype=np.int32)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int)
    _lib.check(lib.shf_face_eval_match(
        det4.ctypes.data_as(dp), det_off.ctypes.data_as(lp), gt4.ctypes.data_as(dp), gt_off.ctypes.data_as(lp),
        difficult.ctypes.data_as(C.POINTER(C.c_uint8)), len(det_off) - 1, float(ovr), code.ctypes.data_as(ip),
        index.ctypes.data_as(ip)), "face_eval_match")
    return code, index


def _device_safe(*arrays):
    """Everything finite and far from overflow: only then is the device's walk the host's bit for bit."""
    with np.errstate(invalid='ignore'):
        return all(bool(np.all(np.abs(a) < _FINITE_BOUND)) for a in arrays)


# ---- refinement, curve, AP ----------------------------------------------------------------------------------------------
def refinement_terms(det4, gt4):
    """tx, ty, sx, sy of matched (detection, box) pairs as VOCpr.py:141-156 writes them; rows are x1-y1-x2-y2."""
    gtx, dtx = gt4[:, 2] - gt4[:, 0], det4[:, 2] - det4[:, 0]
    gty, dty = gt4[:, 3] - gt4[:, 1], det4[:, 3] - det4[:, 1]
    gtcx, dtcx = (gt4[:, 2] + gt4[:, 0]) / 2., (det4[:, 2] + det4[:, 0]) / 2.
    gtcy, dtcy = (gt4[:, 3] + gt4[:, 1]) / 2., (det4[:, 3] + det4[:, 1]) / 2.
    return (gtcx - dtcx) / dtx, (gtcy - dtcy) / dty, gtx / dtx, gty / dty


def transform_boxes(det4, tx, ty, sx, sy):
    """transf_dets (VOCpr.py:250-259) on (n, 4) x1-y1-x2-y2 rows."""
    w = (det4[:, 2] - det4[:, 0]) / 2.0
    h = (det4[:, 3] - det4[:, 1]) / 2.0
    cx = (det4[:, 2] + det4[:, 0]) / 2. + tx * w * 2
    cy = (det4[:, 3] + det4[:, 1]) / 2. + ty * h * 2
    return np.stack([cx - w * sx, cy - h * sy, cx + w * sx, cy + h * sy], axis=1)


def voc_ap(rec, prec):
    """VOCap (VOCpr.py:191-198): the envelope is built with Python's ``max(a, b)``, which keeps ``a`` unless ``b > a``
    -- a NaN precision stays where it is and does not spread."""
    mrec = np.concatenate(([0], rec, [1]))
    mpre = np.concatenate(([0], prec, [0])).tolist()
    for i in range(len(mpre) - 2, 0, -1):
        if mpre[i + 1] > mpre[i]:
            mpre[i] = mpre[i + 1]
    mpre = np.array(mpre, dtype=np.float64)
    i = np.where(mrec[1:] != mrec[0:-1])[0] + 1
    return np.sum((mrec[i] - mrec[i - 1]) * mpre[i])


def voc_old_ap(rec, prec):
    """VOColdap (VOCpr.py:201-211), the 11-point average."""
    rec, prec = np.array(rec), np.array(prec)
    ap = 0.0
    for t in np.linspace(0, 1, 11):
        pr = prec[rec >= t]
        if pr.size == 0:
            pr = 0
        ap = ap + np.max(pr) / 11.0
    return ap


def pr_curve(tp, fp, tot):
    """drawPrfast (VOCpr.py:214-231) without the plot: (rec, prec)."""
    tp, fp = np.cumsum(tp), np.cumsum(fp)
    with np.errstate(divide='ignore', invalid='ignore'):
        return tp / tot, tp / (fp + tp)


def evaluate(dets, gt, ovr=0.5, iters=5, device=False):
    """``dets``: Detections (already filtered; any order), ``gt``: FaceGT.  Returns (ap, rec, prec, info) as
    evaluate_optim + drawPrfast compute them; ``info`` holds ``tot``, ``ap11`` (VOColdap), the score-ordered ``names``,
    the final ``boxes`` and, per round, ``tp`` / ``fp`` (float 0/1 arrays in score order), ``index`` (the chosen box
    within the image, -1 without ground truth) and ``means`` (tx, ty, sx, sy).
    ``device=True``: the matching of every round on the GPU (same result, bit for bit; ShfError without a GPU)."""
    if iters < 1:
        raise ValueError('face_eval.evaluate: iters must be at least 1')
    dets = dets.sorted_by_score()
    flat = group_by_image(dets, gt)
    perm = flat['perm']
    boxes = dets.rows[:, 1:5].copy()
    log = logging.getLogger(__name__)
    rounds = []
    for _ in range(iters):
        grouped = np.ascontiguousarray(boxes[perm])
        on_device = device
        if on_device and not _device_safe(dets.rows[:, 0], grouped, flat['gt4']):
            log.warning('face_eval: non-finite boxes or scores, matching on the host')
            on_device = False
        code_g, index_g = (match_device if on_device else match_host)(grouped, flat, ovr)
        code = np.empty_like(code_g)
        index = np.empty_like(index_g)
        code[perm], index[perm] = code_g, index_g
        # the true positives in global score order, with the box each sits on
        hit = np.nonzero(code_g == TRUE_POSITIVE)[0]
        img_of = np.searchsorted(flat['det_off'], hit, side='right') - 1
        gbox = flat['gt4'][flat['gt_off'][img_of] + index_g[hit]]
        back = np.argsort(perm[hit], kind='stable')
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)        # (the mean of an empty list: NaN, as there)
            terms = refinement_terms(grouped[hit][back], gbox[back])
            means = tuple(np.mean(np.ascontiguousarray(t)) for t in terms)
            boxes = transform_boxes(boxes, *means)
        rounds.append(dict(tp=(code == TRUE_POSITIVE).astype(np.float64), fp=(code == FALSE_POSITIVE).astype(np.float64),
                           index=index, means=means))
    rec, prec = pr_curve(rounds[-1]['tp'], rounds[-1]['fp'], flat['tot'])
    with np.errstate(invalid='ignore'):
        ap, ap11 = voc_ap(rec, prec), voc_old_ap(rec, prec)
    info = dict(tot=flat['tot'], ap11=ap11, rounds=rounds, names=dets.names, scores=dets.rows[:, 0].copy(), boxes=boxes)
    return ap, rec, prec, info


def face_eval(det_file, ann_file, dataset='PASCAL', minw=30, minh=30, iters=5, ovr=0.5, device=False):
    """plot_AP.py for one detection file: ``afw_res.txt`` / ``pascal_res.txt`` + the dataset's annotation .mat ->
    (ap, rec, prec, info)."""
    dataset = dataset.upper()
    if dataset not in ANNOTATION_FILES:
        raise ValueError('Unknown Dataset')
    gt = load_annotations_mat(ann_file, minw, minh, dataset)
    dets = filter_detections(load_detections(det_file), min_pixels(minw, minh))
    return evaluate(dets, gt, ovr=ovr, iters=iters, device=device)


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog='python -m smallhardface_amd.face_eval', description='AP on AFW / PASCAL faces')
    p.add_argument('detfile', help='detection file (name score x1 y1 x2 y2 per line)')
    p.add_argument('--dataset', default='PASCAL', choices=sorted(ANNOTATION_FILES))
    p.add_argument('--ann', required=True, help="the dataset's annotation .mat")
    p.add_argument('--minw', type=int, default=30, help='minimum width of a face that counts')
    p.add_argument('--minh', type=int, default=30, help='minimum height of a face that counts')
    p.add_argument('--nit', type=int, default=5, help='rounds of bounding-box refinement')
    a = p.parse_args(argv)
    ap, _, _, info = face_eval(a.detfile, a.ann, a.dataset, a.minw, a.minh, a.nit,
                               device=os.environ.get('SHF_DEVICE_EVAL') == '1')
    print('AP: {:.4f} (11-point {:.4f})'.format(ap, info['ap11']))


if __name__ == '__main__':
    main()
