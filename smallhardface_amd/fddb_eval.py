"""FDDB evaluation (discrete and continuous ROC) of a written ``detection_rect.txt``.

The reference hands that file to FDDB's published ``evaluate`` binary (lib/datasets/fddb.py:22-24, 75-105:
``/{root}/evaluation/evaluate -a .../FDDB-folds/val_gt.txt ... -f 0 -r .../rect_``) and reads ``rect_DiscROC.txt`` /
``rect_ContROC.txt`` for the rate of the first row with fewer than 1000 false positives.  Neither the binary nor OpenCV
is available to this package, so this module follows the FDDB technical report, the two file formats and the
reference's readout, and fixes the protocol below.  It does NOT claim pixel equality with the published binary; two
points are unpinned against it:

  * the rasterisation of the two shapes (the binary draws them with OpenCV; here a pixel belongs to a shape by the rules
    below);
  * tie-breaking among assignments of equal total score (here: whatever ``scipy.optimize.linear_sum_assignment`` returns).

Protocol:

  * annotations are FDDB's ellipse list: per image a name line, a count line and ``major_radius minor_radius angle
    center_x center_y 1`` per face, the angle in radians, that of the major axis against the x axis.  Detections are what
    ``datasets.write_detections_fddb`` writes: a name line, a count line and ``x y w h score`` per detection;
  * masks live on integer pixel coordinates (ix, iy).  RECTANGLE: ``rint(x) <= ix <= rint(x + w)`` and ``rint(y) <= iy <=
    rint(y + h)``, both corners inclusive, ``rint`` rounding halves to even.  ELLIPSE: with ``c = cos(angle)``,
    ``s = sin(angle)`` computed once on the host, ``dx = ix - cx``, ``dy = iy - cy``, ``u = dx*c + dy*s``,
    ``v = dy*c - dx*s`` the pixel is inside when ``(u*u)*(rb*rb) + (v*v)*(ra*ra) <= (ra*ra)*(rb*rb)`` -- float64 in exactly
    that operation order: adds, multiplies and one compare, nothing that rounds differently on host and device;
  * with an image size (W, H) both masks are clipped to ``0 <= ix < W``, ``0 <= iy < H``.  WITHOUT sizes nothing is
    clipped (shapes may reach negative coordinates);
  * ``S = inter / (area(a) + area(d) - inter)`` in float64 per (annotation, detection) pair of an image, 0 where the
    union is 0;
  * matching once per image over all its detections: the one-to-one assignment maximising the sum of S, pairs with
    ``S == 0`` dropped; a matched detection gets ``m = S``, every other one ``m = 0``;
  * N = the annotations of all listed images; thresholds = the distinct detection scores, ascending; at t over the
    detections with ``score >= t``: TPD = how many have ``m > 0.5`` (strict), TPC = the sum of m (accumulated in falling
    score, then file order), FP = their number - TPD for BOTH curves; rows ``TPD / N  FP`` and ``TPC / N  FP``;
  * readout: the rate of the first row with ``FP < 1000``; NaN with a logged warning when there is none.

The images evaluated are those of the annotation file, in its order; a detection block is looked up by its name line
(the last of equal names), an image without one has no detections, and blocks of unknown names are dropped with a warning.

The default path is host numpy.  ``device=True`` counts the mask pixels -- every (annotation, detection) pair of every
image, and every annotation's area -- on the GPU (``shf_fddb_pair_counts``, csrc/eval.hip).  The device returns integers
only; S, the assignment, the curves and the readout are formed on the host from them, so the result is the host path's bit
for bit.  Shapes the device does not take -- non-finite parameters, a scan box of more than 2^20 pixels, corners of 2^30 or
more, 2^26 pairs or more -- are counted on the host with a logged warning.  The host path in turn raises ``ValueError`` for
an ellipse whose scan box exceeds 2^24 pixels (an infinite or absurd radius without an image size to clip it), naming it.
"""
import ctypes as C
import logging
import os

import numpy as np

ANNOTATION_FILE = 'val_gt.txt'
MAX_SCAN_BOX = 1 << 20       # pixels of one ellipse scan box the device accepts (kFddbMaxScanBox, csrc/eval.h)
MAX_PAIRS = 1 << 26          # (annotation, detection) pairs of one device call (kFddbMaxPairs: one wave per pair, one launch)
MAX_HOST_SCAN_BOX = 1 << 24  # pixels of one scan box the host path rasterises (a handful of float64 planes of that size)
_COORD_BOUND = 1 << 30       # every integer corner handed to the device stays below it in magnitude
_FINITE_BOUND = 1e9          # parameters below it round to corners inside _COORD_BOUND


class Annotations(object):
    """``names[i]`` the image, ``ellipses[i]`` its (k, 5) ``ra rb angle cx cy`` rows, float64."""

    def __init__(self, names, ellipses):
        self.names = [str(n) for n in names]
        self.ellipses = [np.array(e, dtype=np.float64).reshape(-1, 5) for e in ellipses]
        if len(self.names) != len(self.ellipses):
            raise ValueError('Annotations: %d names for %d ellipse lists' % (len(self.names), len(self.ellipses)))

    def __len__(self):
        return len(self.names)


class Detections(object):
    """``names[i]`` the image, ``rows[i]`` its (n, 5) ``x y w h score`` rows in file order, float64."""

    def __init__(self, names, rows):
        self.names = [str(n) for n in names]
        self.rows = [np.array(r, dtype=np.float64).reshape(-1, 5) for r in rows]
        if len(self.names) != len(self.rows):
            raise ValueError('Detections: %d names for %d row lists' % (len(self.names), len(self.rows)))

    def __len__(self):
        return len(self.names)


# ---- readers ----------------------------------------------------------------------------------------------------------
def _read_blocks(path, n_numbers, what):
    """name line, count line, count rows of ``n_numbers`` numbers each -> (names, [(count, n_numbers) arrays])."""
    with open(path) as f:
        lines = f.read().splitlines()
    while lines and not lines[-1].strip():
        lines.pop()
    names, blocks, i = [], [], 0
    while i < len(lines):
        name = lines[i].strip()
        if i + 1 >= len(lines):
            raise ValueError('%s: line %d: name %r without a count line' % (path, i + 1, name))
        try:
            count = int(lines[i + 1].strip())
        except ValueError:
            raise ValueError('%s: line %d: expected the number of %s of %r, got %r'
                             % (path, i + 2, what, name, lines[i + 1]))
        if count < 0 or i + 2 + count > len(lines):
            raise ValueError('%s: line %d: %r announces %d %s, %d lines are left'
                             % (path, i + 2, name, count, what, len(lines) - i - 2))
        rows = np.zeros((count, n_numbers), dtype=np.float64)
        for k in range(count):
            parts = lines[i + 2 + k].split()
            try:
                if len(parts) != n_numbers:
                    raise ValueError
                rows[k] = [float(p) for p in parts]
            except ValueError:
                raise ValueError('%s: line %d: expected %d numbers, got %r' % (path, i + 3 + k, n_numbers, lines[i + 2 + k]))
        names.append(name)
        blocks.append(rows)
        i += 2 + count
    return names, blocks


def load_annotations(path):
    """FDDB's ellipse list (``FDDB-folds/val_gt.txt``) -> Annotations."""
    names, blocks = _read_blocks(path, 6, 'faces')
    return Annotations(names, [b[:, :5] for b in blocks])


def load_detections(path):
    """``detection_rect.txt`` as ``datasets.write_detections_fddb`` writes it -> Detections."""
    names, blocks = _read_blocks(path, 5, 'detections')
    return Detections(names, blocks)


# ---- the shared geometry step ---------------------------------------------------------------------------------------------
def align(dets, gt):
    """The detections of every annotated image, in the annotation file's order: a list of (n, 5) arrays."""
    slot = {n: i for i, n in enumerate(dets.names)}            # (the last of equal names)
    unknown = sorted(set(dets.names) - set(gt.names))
    if unknown:
        logging.getLogger(__name__).warning('fddb_eval: %d detection blocks of images without annotations are dropped '
                                            '(first: %s)', len(unknown), unknown[0])
    return [dets.rows[slot[n]] if n in slot else np.zeros((0, 5)) for n in gt.names]


def geometry(rows, gt, sizes=None):
    """Everything both paths count from, computed once.  ``rows``: per image of ``gt`` its (n, 5) detections (``align``);
    ``sizes``: None (nothing is clipped) or per image ``(W, H)`` / None.  Returns a dict of flat arrays:
    ``ann_off`` / ``det_off`` (I + 1) int64, ``ell`` (A, 6) float64 ``ra rb c s cx cy``, ``ell_box`` (A, 4) int64 the
    inclusive scan box ``x0 y0 x1 y1`` of each ellipse (its bounding box with a pixel to spare, cut to the canvas; empty
    when x1 < x0 or y1 < y0), ``rect`` (D, 4) int64 the inclusive rounded corners ``x0 y0 x1 y1`` cut to the canvas,
    ``det_area`` (D,) int64 and ``score`` (D,)."""
    n_img = len(gt)
    ann_off = np.zeros(n_img + 1, dtype=np.int64)
    det_off = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([e.shape[0] for e in gt.ellipses], out=ann_off[1:])
    np.cumsum([r.shape[0] for r in rows], out=det_off[1:])
    e = np.concatenate(list(gt.ellipses) + [np.zeros((0, 5))], axis=0)
    r = np.concatenate(list(rows) + [np.zeros((0, 5))], axis=0)
    # the canvas of every row: [0, W - 1] x [0, H - 1], or everything
    lo, hi = -(2 ** 62), 2 ** 62
    canvas = np.empty((n_img, 2), dtype=np.int64)
    canvas[:] = hi
    clipped = np.zeros(n_img, dtype=bool)
    if sizes is not None:
        for i, wh in enumerate(sizes):
            if wh is not None:
                canvas[i] = (int(wh[0]) - 1, int(wh[1]) - 1)
                clipped[i] = True
    a_img = np.repeat(np.arange(n_img), np.diff(ann_off))
    d_img = np.repeat(np.arange(n_img), np.diff(det_off))

    def cut(x0, y0, x1, y1, img):
        c = clipped[img]
        x0, y0 = np.where(c, np.maximum(x0, 0), x0), np.where(c, np.maximum(y0, 0), y0)
        x1, y1 = np.where(c, np.minimum(x1, canvas[img, 0]), x1), np.where(c, np.minimum(y1, canvas[img, 1]), y1)
        return np.stack([x0, y0, x1, y1], axis=1).astype(np.int64).reshape(-1, 4)

    with np.errstate(invalid='ignore', over='ignore'):
        ra, rb, ang, cx, cy = (e[:, k] for k in range(5))
        c, s = np.cos(ang), np.sin(ang)
        hx = np.sqrt((ra * c) ** 2 + (rb * s) ** 2)
        hy = np.sqrt((ra * s) ** 2 + (rb * c) ** 2)
        box = [np.floor(cx - hx) - 1, np.floor(cy - hy) - 1, np.ceil(cx + hx) + 1, np.ceil(cy + hy) + 1]
        box = [np.clip(np.nan_to_num(b, nan=0.0), lo, hi).astype(np.int64) for b in box]
        rect = [np.rint(r[:, 0]), np.rint(r[:, 1]), np.rint(r[:, 0] + r[:, 2]), np.rint(r[:, 1] + r[:, 3])]
        rect = [np.clip(np.nan_to_num(b, nan=0.0), lo, hi).astype(np.int64) for b in rect]
    ell_box = cut(*box, img=a_img)
    rect = cut(*rect, img=d_img)
    det_area = np.maximum(rect[:, 2] - rect[:, 0] + 1, 0) * np.maximum(rect[:, 3] - rect[:, 1] + 1, 0)
    return dict(ann_off=ann_off, det_off=det_off, ell=np.ascontiguousarray(np.stack([ra, rb, c, s, cx, cy], axis=1)),
                ell_box=ell_box, rect=rect, det_area=det_area, score=r[:, 4].copy())


def pair_offsets(geom):
    """Where image i's (A_i, D_i) intersection counts start in the flat ``inter`` array: (I + 1) int64."""
    off = np.zeros(len(geom['ann_off']), dtype=np.int64)
    np.cumsum(np.diff(geom['ann_off']) * np.diff(geom['det_off']), out=off[1:])
    return off


# ---- pixel counts ---------------------------------------------------------------------------------------------------------
def ellipse_mask(ell, box):
    """The (h, w) boolean mask of one ellipse row ``ra rb c s cx cy`` over its inclusive scan box."""
    x0, y0, x1, y1 = (int(v) for v in box)
    if x1 < x0 or y1 < y0:
        return np.zeros((max(y1 - y0 + 1, 0), max(x1 - x0 + 1, 0)), dtype=bool)
    ra, rb, c, s, cx, cy = ell
    dx = (np.arange(x0, x1 + 1, dtype=np.int64) - cx)[None, :]
    dy = (np.arange(y0, y1 + 1, dtype=np.int64) - cy)[:, None]
    u = dx * c + dy * s
    v = dy * c - dx * s
    return (u * u) * (rb * rb) + (v * v) * (ra * ra) <= (ra * ra) * (rb * rb)


def pair_counts_host(geom):
    """numpy.  Returns integers only: ``inter`` (flat int64; image i's (A_i, D_i) block row-major at ``pair_offsets``),
    ``ann_area`` (A,) int64, ``det_area`` (D,) int64."""
    ann_off, det_off, poff = geom['ann_off'], geom['det_off'], pair_offsets(geom)
    inter = np.zeros(poff[-1], dtype=np.int64)
    ann_area = np.zeros(ann_off[-1], dtype=np.int64)
    rect = geom['rect']
    for i in range(len(ann_off) - 1):
        d0, d1 = det_off[i], det_off[i + 1]
        for k, a in enumerate(range(ann_off[i], ann_off[i + 1])):
            bx0, by0, bx1, by1 = (int(v) for v in geom['ell_box'][a])
            if bx1 >= bx0 and by1 >= by0 and (bx1 - bx0 + 1) * (by1 - by0 + 1) > MAX_HOST_SCAN_BOX:
                raise ValueError('fddb_eval: annotation %d of image %d has a scan box of %d x %d pixels (ra rb c s cx cy = %s); '
                                 'the host path rasterises at most %d'
                                 % (k, i, bx1 - bx0 + 1, by1 - by0 + 1, geom['ell'][a].tolist(), MAX_HOST_SCAN_BOX))
            mask = ellipse_mask(geom['ell'][a], geom['ell_box'][a])
            ann_area[a] = int(mask.sum())
            if d1 == d0 or mask.size == 0:
                continue
            # summed-area table of the mask: the pixels of rect n box in four look-ups per detection
            table = np.zeros((mask.shape[0] + 1, mask.shape[1] + 1), dtype=np.int64)
            np.cumsum(np.cumsum(mask, axis=0, dtype=np.int64), axis=1, out=table[1:, 1:])
            x0 = np.maximum(rect[d0:d1, 0], bx0) - bx0
            y0 = np.maximum(rect[d0:d1, 1], by0) - by0
            x1 = np.minimum(rect[d0:d1, 2], bx1) - bx0 + 1
            y1 = np.minimum(rect[d0:d1, 3], by1) - by0 + 1
            ok = (x1 > x0) & (y1 > y0)
            x0, y0, x1, y1 = (np.where(ok, t, 0) for t in (x0, y0, x1, y1))
            row = table[y1, x1] - table[y0, x1] - table[y1, x0] + table[y0, x0]
            inter[poff[i] + k * (d1 - d0): poff[i] + (k + 1) * (d1 - d0)] = np.where(ok, row, 0)
    return inter, ann_area, geom['det_area'].copy()


def pair_counts_device(geom, phase_ms=None):
    """The same integers through ``shf_fddb_pair_counts`` (ShfError without the library or a GPU).  ``phase_ms``: None, or
    a float64 array of 3 that receives the milliseconds of the uploads, the kernels and the read-back."""
    if not _device_safe(geom):             # (before the corners are narrowed to 32 bits)
        raise ValueError('fddb_eval.pair_counts_device: non-finite or huge shapes, or too many pairs, for the device')
    from . import _lib
    lib = _lib.load()
    ell = np.ascontiguousarray(geom['ell'], dtype=np.float64)
    ell_box = np.ascontiguousarray(geom['ell_box'], dtype=np.int32)
    rect = np.ascontiguousarray(geom['rect'], dtype=np.int32)
    ann_off = np.ascontiguousarray(geom['ann_off'], dtype=np.int64)
    det_off = np.ascontiguousarray(geom['det_off'], dtype=np.int64)
    inter = np.zeros(pair_offsets(geom)[-1], dtype=np.int32)
    ann_area = np.zeros(ann_off[-1], dtype=np.int32)
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int)
    _lib.check(lib.shf_fddb_pair_counts(
        ell.ctypes.data_as(dp), ell_box.ctypes.data_as(ip), ann_off.ctypes.data_as(lp), rect.ctypes.data_as(ip),
        det_off.ctypes.data_as(lp), len(ann_off) - 1, inter.ctypes.data_as(ip), ann_area.ctypes.data_as(ip),
        None if phase_ms is None else phase_ms.ctypes.data_as(dp)),
        "fddb_pair_counts")
    return inter.astype(np.int64), ann_area.astype(np.int64), geom['det_area'].copy()


def _device_safe(geom):
    """Finite parameters, corners that fit 31 bits, scan boxes and a pair count under the device's caps: only then does
    the device count what the host counts."""
    if int(pair_offsets(geom)[-1]) >= MAX_PAIRS:
        return False
    with np.errstate(invalid='ignore'):
        if not bool(np.all(np.abs(geom['ell']) < _FINITE_BOUND)):
            return False
    for k in ('ell_box', 'rect'):
        if geom[k].size and int(np.abs(geom[k]).max()) >= _COORD_BOUND:
            return False
    b = geom['ell_box']
    pixels = np.maximum(b[:, 2] - b[:, 0] + 1, 0) * np.maximum(b[:, 3] - b[:, 1] + 1, 0)
    return not (pixels.size and int(pixels.max()) > MAX_SCAN_BOX)


# ---- scores, matching, curves ---------------------------------------------------------------------------------------------
def scores(inter, ann_area, det_area):
    """(A, D) intersections, (A,) and (D,) areas -> S (A, D) float64: inter / union, 0 where the union is 0."""
    inter = np.asarray(inter, dtype=np.int64)
    union = np.asarray(ann_area, dtype=np.int64)[:, None] + np.asarray(det_area, dtype=np.int64)[None, :] - inter
    out = np.zeros(inter.shape, dtype=np.float64)
    np.divide(inter.astype(np.float64), union.astype(np.float64), out=out, where=union != 0)
    return out


def match_pairs(S):
    """The one-to-one assignment that maximises the sum of S, without its pairs of S == 0: a list of (annotation,
    detection) index pairs in rising annotation order."""
    S = np.asarray(S, dtype=np.float64)
    if S.ndim != 2 or S.size == 0 or not (S > 0).any():
        return []
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(S, maximize=True)
    return [(int(a), int(d)) for a, d in zip(rows, cols) if S[a, d] > 0]


def roc(score, m, n_faces):
    """``score`` and ``m`` per detection in file order -> (disc, cont), each (T, 2) float64 ``rate FP``, one row per
    distinct score in ascending order.  TPC is accumulated in falling score, then file order."""
    score, m = np.asarray(score, dtype=np.float64).reshape(-1), np.asarray(m, dtype=np.float64).reshape(-1)
    order = np.argsort(-score, kind='stable')
    s, ms = score[order], m[order]
    tpd = np.cumsum(ms > 0.5, dtype=np.int64)
    tpc = np.cumsum(ms)                                   # (sequential: one fixed order of additions)
    thresh = np.unique(score)                              # ascending
    count = np.searchsorted(-s, -thresh, side='right')    # detections with score >= t; at least one each
    fp = (count - tpd[count - 1]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        disc = np.stack([tpd[count - 1] / np.float64(n_faces), fp], axis=1)
        cont = np.stack([tpc[count - 1] / np.float64(n_faces), fp], axis=1)
    return disc.reshape(-1, 2), cont.reshape(-1, 2)


def rate_at(curve, fp_below=1000):
    """The reference's readout (fddb.py:94, 99): the rate of the first row with FP < ``fp_below``; NaN and a warning when
    there is none."""
    curve = np.asarray(curve, dtype=np.float64).reshape(-1, 2)
    hit = np.nonzero(curve[:, 1] < fp_below)[0]
    if hit.size == 0:
        logging.getLogger(__name__).warning('fddb_eval: no ROC row with fewer than %d false positives', fp_below)
        return float('nan')
    return float(curve[hit[0], 0])


def write_roc(result, directory, prefix='rect_'):
    """``<prefix>DiscROC.txt`` and ``<prefix>ContROC.txt`` in ``directory``: ``rate FP`` per row, the rate with all its
    digits.  Returns the two paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for key, fname in (('disc', 'DiscROC.txt'), ('cont', 'ContROC.txt')):
        path = os.path.join(directory, prefix + fname)
        with open(path, 'w') as f:
            for rate, fp in result[key]:
                f.write('%r %d\n' % (float(rate), int(fp)))
        paths.append(path)
    return tuple(paths)


def result_string(result):
    return 'rect_disc_at_1000: {:.4f}, rect_cont_at_1000: {:.4f}'.format(result['disc_at_1000'], result['cont_at_1000'])


def evaluate(dets, gt, sizes=None, device=False):
    """``dets``: Detections, ``gt``: Annotations, ``sizes``: None (unclipped) or per image of ``gt`` ``(W, H)`` / None.
    Returns a dict: ``disc`` / ``cont`` (T, 2) curves, ``disc_at_1000`` / ``cont_at_1000``, ``N``, ``pairs`` (per image
    the matched (annotation, detection, S) triples), ``m`` and ``score`` per detection (annotation-file image order,
    then file order) and the integer arrays ``inter`` / ``ann_area`` / ``det_area``.
    ``device=True``: the pixel counts on the GPU (same result, bit for bit; ShfError without a GPU)."""
    geom = geometry(align(dets, gt), gt, sizes)
    if device and not _device_safe(geom):
        logging.getLogger(__name__).warning('fddb_eval: non-finite or huge shapes, or too many pairs, for the device: counting on the host')
        device = False
    inter, ann_area, det_area = (pair_counts_device if device else pair_counts_host)(geom)
    ann_off, det_off, poff = geom['ann_off'], geom['det_off'], pair_offsets(geom)
    m = np.zeros(det_off[-1], dtype=np.float64)
    pairs = []
    for i in range(len(gt)):
        a0, a1, d0, d1 = ann_off[i], ann_off[i + 1], det_off[i], det_off[i + 1]
        S = scores(inter[poff[i]:poff[i + 1]].reshape(a1 - a0, d1 - d0), ann_area[a0:a1], det_area[d0:d1])
        found = [(a, d, float(S[a, d])) for a, d in match_pairs(S)]
        for a, d, v in found:
            m[d0 + d] = v
        pairs.append(found)
    n_faces = int(ann_off[-1])
    disc, cont = roc(geom['score'], m, n_faces)
    return dict(disc=disc, cont=cont, disc_at_1000=rate_at(disc, 1000), cont_at_1000=rate_at(cont, 1000), N=n_faces,
                pairs=pairs, m=m, score=geom['score'], inter=inter, ann_area=ann_area, det_area=det_area)


def sizes_of(paths):
    """``PIL.Image.open(path).size`` (the header only) per path; None for a path that is None or not a file.  One log line
    when some are missing: the masks of those images are not clipped."""
    from PIL import Image
    out = []
    for path in paths:
        if path is not None and os.path.isfile(path):
            with Image.open(path) as im:
                out.append(im.size)
        else:
            out.append(None)
    missing = sum(s is None for s in out)
    if missing:
        logging.getLogger(__name__).warning('fddb_eval: %d of %d image files not found: their masks are not clipped to the '
                                            'image size', missing, len(out))
    return out


def image_sizes(names, image_root, exts=('.jpg', '.png', '.jpeg', '')):
    """The sizes of the images ``names`` under ``image_root``, whichever of ``exts`` the file carries."""
    def find(n):
        hits = [os.path.join(image_root, n + e) for e in exts if os.path.isfile(os.path.join(image_root, n + e))]
        return hits[0] if hits else None
    return sizes_of([find(n) for n in names])


def fddb_eval(det_file, ann_file, image_root=None, device=False):
    """``detection_rect.txt`` + FDDB's ellipse list (+ the directory its image names are relative to) -> the dict of
    ``evaluate``.  Without ``image_root``, or for an image that is not found under it, nothing is clipped."""
    gt = load_annotations(ann_file)
    dets = load_detections(det_file)
    sizes = image_sizes(gt.names, image_root) if image_root else None
    return evaluate(dets, gt, sizes=sizes, device=device)


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog='python -m smallhardface_amd.fddb_eval', description='FDDB discrete / continuous ROC')
    p.add_argument('detfile', help='detection file (detection_rect.txt: name, count, then x y w h score per line)')
    p.add_argument('--ann', required=True, help="FDDB's ellipse annotation list (FDDB-folds/val_gt.txt)")
    p.add_argument('--images', default=None, help='directory the image names are relative to (masks are clipped to the '
                                                  'image sizes; without it nothing is clipped)')
    p.add_argument('--out', default=None, help='directory for rect_DiscROC.txt and rect_ContROC.txt')
    a = p.parse_args(argv)
    res = fddb_eval(a.detfile, a.ann, a.images, device=os.environ.get('SHF_DEVICE_EVAL') == '1')
    if a.out:
        write_roc(res, a.out)
    print(result_string(res))


if __name__ == '__main__':
    main()
