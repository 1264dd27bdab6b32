"""The per-class detection lists of a multi-class image on the device (C ABI shf_class_lists_*, csrc/class_lists.hip; run
on an MI355X: ``pytest -m gpu``): the reference's own three-class vectors, the boundaries of the compaction against its
numpy restatement, forwarded members, the two-class list against the fused path's, detect() under SHF_DEVICE_MERGE=1
against plain detect(), and the refusals.

Everything here is compared bit for bit: the compaction copies scores, its box arithmetic is one fp32 subtraction and one
fp32 division per coordinate (IEEE, the same two operations numpy performs), and the merges run the same kernels on the
same rows whichever way the rows reached the device.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import helpers as H
from tests import multiclass_cases as M

pytestmark = pytest.mark.gpu

METHODS = ["BBOX_VOTE", "NMS"]
_nets = {}


def _one_hot_net(C):
    """A net with a C-class proposal tail (one-hot 1x1 convolution in front); cached per class count."""
    from smallhardface_amd import caffe
    if C not in _nets:
        net = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, C, 3, False))
        wt = np.zeros((128, 128, 1, 1), np.float32)
        wt[np.arange(128), np.arange(128), 0, 0] = 1.0
        net.params["c0"][0].data[...] = wt
        net.params["c0"][1].data[...] = 0
        _nets[C] = net
    return _nets[C]


def _np_rows(units, C):
    """Per unit the flip fix and the unscale in float32 (lib/test.py:52-66), the units concatenated: (boxes (N, 4),
    probs (N, C)).  units: (boxes5 (max(R, 1), 5), probs (R, C), im_w, im_scale, flip)."""
    boxes, probs = [], []
    for b, p, w, s, f in units:
        bx = np.array(b[:len(p), 1:5], dtype=np.float32)
        if f:
            bx[:, [0, 2]] = np.float32(w) - bx[:, [2, 0]]
        boxes.append(bx / np.float32(s))
        probs.append(np.asarray(p, np.float32).reshape(-1, C))
    boxes, probs = np.concatenate(boxes), np.concatenate(probs)
    assert boxes.dtype == np.float32 and probs.dtype == np.float32
    return boxes, probs


def _np_lists(units, C, thresh):
    """The numpy restatement of the lists: np.where per class over the concatenated units (lib/test.py:161-167)."""
    boxes, probs = _np_rows(units, C)
    out = []
    for c in range(1, C):
        inds = np.where(probs[:, c] > thresh)[0]
        out.append(np.hstack((boxes[inds], probs[inds, c:c + 1])).astype(np.float32))
    return out


def _inject(net, units, thresh):
    net.debug_class_lists_add([u[0] for u in units], [u[1] for u in units], [u[2] for u in units], [u[3] for u in units],
                              [u[4] for u in units], thresh)


def _lists(net):
    return [net.class_lists_export(c) for c in range(1, net.num_classes)]


def _assert_lists(net, want):
    assert net.class_lists_count() == [len(w) for w in want]
    for got, w in zip(_lists(net), want):
        assert got.dtype == np.float32 and got.shape == w.shape
        np.testing.assert_array_equal(got.view(np.uint32), w.view(np.uint32))     # bit for bit (NaN-safe, -0.0-safe)


def _host_merge(dets, method, nms_thresh):
    from smallhardface_amd.nms import bbox_vote, nms
    if method == "BBOX_VOTE":
        return bbox_vote(dets, nms_thresh)
    return dets[nms(dets, nms_thresh), :]


def _assert_merged(net, want_lists, method, nms_thresh):
    for c, dets in enumerate(want_lists):
        got = net.class_lists_finish(c + 1, method, nms_thresh)
        want = _host_merge(dets, method, nms_thresh)
        assert got.dtype == (np.float64 if method == "BBOX_VOTE" else np.float32)
        assert got.shape == want.shape, (method, c)
        np.testing.assert_array_equal(got, want)


# ---- 1. the reference's own vectors ---------------------------------------------------------------------------------------------
class _Canned(object):
    def __init__(self, boxes, probs):
        self.blobs = {"boxes": O.OBlob(boxes.shape), "cls_prob": O.OBlob(probs.shape)}
        self.blobs["boxes"].data[...] = boxes
        self.blobs["cls_prob"].data[...] = probs


def test_lists_and_merges_on_the_reference_three_class_vectors(golden):
    from smallhardface_amd import test as T
    g = golden("proposal_multiclass.npz")
    thresh, nms_thresh = float(g["detect_thresh"][0]), float(g["detect_nms_thresh"][0])
    units, all_probs, all_boxes = [], [], []
    for u in (0, 1):
        boxes, probs, info = g["detect_u%d_boxes" % u], g["detect_u%d_probs" % u], g["detect_u%d_im_info" % u]
        w, flip = int(g["detect_u%d_width" % u][0]), bool(g["detect_u%d_flip" % u][0])
        units.append((boxes, probs, w, float(info[0, 2]), flip))
        net = _Canned(boxes, probs)           # (_unit_results flips its argument in place: the canned net's own copy)
        out = {"boxes": net.blobs["boxes"].data, "cls_prob": net.blobs["cls_prob"].data}
        pr, bx = T._unit_results(net, out, w, float(info[0, 2]), flip)
        all_probs.append(pr[0].copy())
        all_boxes.append(bx[0][:, 0:4])
    assert [len(u[1]) for u in units] == [26, 28] and units[1][4] and not units[0][4]
    probs, boxes = np.concatenate(all_probs), np.concatenate(all_boxes)
    want = []
    for c in (1, 2):
        inds = np.where(probs[:, c] > thresh)[0]
        want.append(np.hstack((boxes[inds, :], probs[inds, c][:, np.newaxis])).astype(np.float32, copy=False))
    assert all(len(w) > 0 for w in want)
    net = _one_hot_net(3)
    net.class_lists_begin()
    _inject(net, units, thresh)
    _assert_lists(net, want)
    for method in METHODS:
        for c in (0, 1):
            got = net.class_lists_finish(c + 1, method, nms_thresh)
            ref = g["detect_%s_dets%d" % (method, c)]
            assert got.shape == ref.shape, (method, c)
            np.testing.assert_array_equal(np.asarray(got, np.float64), ref)
    _assert_lists(net, want)                  # a merge leaves its list as it was


# ---- 2. boundaries of the compaction -----------------------------------------------------------------------------------------------
ROWS16 = [0, 1, 63, 64, 65, 255, 256, 257, 700, 1, 0, 64, 300, 256, 5, 129]     # R = 0 first and between two others
THRESH = 0.5


def _random_units(rows, C, fill, seed):
    """Random probabilities; class 1 per `fill`: "random", "all" (every row survives), "none" (no survivor; for C > 2 the
    LAST class then has every row surviving, so lists of both kinds sit side by side).  A "random" fill carries NaNs.
    Boxes as the layer emits them (column 0 zero), every other unit flipped, non-integer scales."""
    rng = np.random.default_rng(seed)
    units = []
    for i, R in enumerate(rows):
        p = rng.random((R, C), dtype=np.float32)
        if fill == "all":
            p[:, 1] = THRESH + np.float32(0.25) * (1 + p[:, 1])
        elif fill == "none":
            p[:, 1] = THRESH * p[:, 1]                      # <= thresh, some of them exactly thresh-near
            if R:
                p[0, 1] = THRESH                            # equality is not a survivor
            if C > 2:
                p[:, C - 1] = 0.75
        elif R > 2:
            p[R // 2, 1] = np.nan
            p[R - 1, C - 1] = np.nan
        b = np.zeros((max(R, 1), 5), np.float32)
        b[:, 1:] = rng.uniform(0, 640, (max(R, 1), 4)).astype(np.float32)
        if R == 0:
            b[0] = [0, 0, 0, 16, 16]                        # the dummy roi (proposal_layer.py:207-208)
        units.append((b, p, 601 + 7 * i, [1.7, 0.37, 1.0, 2.5][i % 4], i % 2 == 1))
    return units


@pytest.mark.parametrize("fill", ["random", "all", "none"])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_a_group_of_sixteen_units_with_mixed_row_counts(C, fill):
    net = _one_hot_net(C)
    units = _random_units(ROWS16, C, fill, 100 + C)
    want = _np_lists(units, C, THRESH)
    if fill == "all":
        assert len(want[0]) == sum(ROWS16)
    if fill == "none":
        assert len(want[0]) == 0 and (C == 2 or len(want[-1]) == sum(ROWS16))
    if fill == "random":
        assert all(0 < len(w) < sum(ROWS16) for w in want)
    net.class_lists_begin()
    _inject(net, units, THRESH)
    _assert_lists(net, want)
    assert not any(np.isnan(l).any() for l in _lists(net))
    # the same units as two calls on one image: the second continues the lists
    net.class_lists_begin()
    _inject(net, units[:7], THRESH)
    _assert_lists(net, _np_lists(units[:7], C, THRESH))
    _inject(net, units[7:], THRESH)
    _assert_lists(net, want)
    # ... and begin empties them
    net.class_lists_begin()
    assert net.class_lists_count() == [0] * (C - 1)


@pytest.mark.parametrize("R", [0, 1, 64, 257, 700])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_a_group_of_one_unit(C, R):
    net = _one_hot_net(C)
    units = _random_units([R], C, "random", 7 * R + C)
    units = [units[0][:3] + (0.37, True)]                   # flipped, non-integer scale
    want = _np_lists(units, C, THRESH)
    net.class_lists_begin()
    _inject(net, units, THRESH)
    _assert_lists(net, want)
    for method in METHODS:
        _assert_merged(net, want, method, 0.4)              # an empty class: the dummy row (vote) / no row (NMS)
    if R == 0:
        assert [len(net.class_lists_finish(c, "BBOX_VOTE")) for c in range(1, C)] == [1] * (C - 1)
        np.testing.assert_array_equal(net.class_lists_finish(1, "BBOX_VOTE"), [[10, 10, 20, 20, 0.0001]])
        assert net.class_lists_finish(1, "NMS").shape == (0, 5)


def test_lists_clamp_at_their_capacity_and_keep_the_first_rows():
    """Capacity is units x rmax per class, at least 16 x rmax: with cfg.TEST.N_DETS_PER_MODULE = 4 a fresh net's lists hold
    64 rows.  A unit injected with more rows than that fills them with the first 64 survivors in order."""
    from smallhardface_amd import caffe
    cfg.TEST.N_DETS_PER_MODULE = 4
    net = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 3, 3, False))
    units = _random_units([100, 60], 3, "all", 11)
    rng = np.random.default_rng(12)
    for u in units:
        u[1][:, 2] = rng.random(len(u[1]), dtype=np.float32) * 0.9       # class 2: 4 of 9 rows survive
    want = _np_lists(units, 3, THRESH)
    cap = 64
    net.class_lists_begin()
    _inject(net, units[:1], THRESH)
    first = _np_lists(units[:1], 3, THRESH)
    assert len(first[0]) == 100 and len(want[0]) == 160 and len(first[1]) < cap < len(want[1])   # class 2 fills up in the second call
    _assert_lists(net, [first[0][:cap], first[1]])
    _inject(net, units[1:], THRESH)                                       # class 1 is full; class 2 fills up to the clamp
    _assert_lists(net, [want[0][:cap], want[1][:cap]])
    _assert_merged(net, [want[0][:cap], want[1][:cap]], "BBOX_VOTE", 0.4)


# ---- 3. forwarded members ---------------------------------------------------------------------------------------------------------
WHOLE_CFG = dict(pre_nms_topN=40, score_thresh=0.3)


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("per_head", [True, False], ids=["per_head", "single_blob"])
def test_forwarded_members_of_a_three_class_net(per_head, mode):
    from smallhardface_amd import caffe
    from smallhardface_amd import test as T
    msg = P.parse(M.whole_net_txt(3, per_head))
    root = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(root, M.whole_params(msg))
    cfg.TEST.N_DETS_PER_MODULE = WHOLE_CFG["pre_nms_topN"]
    cfg.TEST.SCORE_THRESH = WHOLE_CFG["score_thresh"]
    root.set_conv_mode(mode)
    sizes = [(9, 13), (7, 9), (12, 10)]
    inputs = [dict(zip(("data", "im_info"), M.whole_input(h, w))) for h, w in sizes]
    members = [root, root.clone(), root.clone()]
    for m, inp in zip(members, inputs):
        m.blobs["data"].reshape(*inp["data"].shape)
        m.blobs["im_info"].reshape(1, 3)
    root.forward_group(members, inputs)
    widths, scales, flips, thresh = [8 * w for _, w in sizes], [1.0, 1.3, 0.77], [False, True, False], 0.4
    units = [(np.array(m.blobs["boxes"].data), np.array(m.blobs["cls_prob"].data), w, s, f)
             for m, w, s, f in zip(members, widths, scales, flips)]
    assert all(u[1].shape[1] == 3 and len(u[1]) > 1 for u in units)
    want = _np_lists(units, 3, thresh)
    assert all(len(w) > 0 for w in want)
    root.class_lists_begin()
    root.class_lists_add(members, widths, scales, flips, thresh)
    _assert_lists(root, want)
    # the merged boxes against the driver's class loop on the same rows
    boxes, probs = _np_rows(units, 3)
    cfg.TEST.NMS_THRESH = 0.4
    for method in METHODS:
        cfg.TEST.NMS_METHOD = method
        ref = T._merge_class_dets(probs, boxes, thresh)
        for c in (1, 2):
            got = root.class_lists_finish(c, method, cfg.TEST.NMS_THRESH)
            assert got.dtype == ref[c - 1].dtype and got.shape == ref[c - 1].shape, (method, c)
            np.testing.assert_array_equal(got, ref[c - 1])
    # a single forward() completes a member just as well: the head alone, appended to the same image
    root.forward(**inputs[0])
    root.class_lists_add([root], widths[:1], scales[:1], flips[:1], thresh)
    _assert_lists(root, _np_lists(units + units[:1], 3, thresh))


# ---- 4. two classes: the single list against the fused path's -----------------------------------------------------------------------
def test_two_class_list_equals_the_fused_paths_list_and_merge():
    import torch
    from smallhardface_amd import caffe
    two = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 2, 3, False))
    rng = np.random.default_rng(5)
    wt = np.zeros((128, 128, 1, 1), np.float32)
    wt[np.arange(128), np.arange(128), 0, 0] = 1.0
    two.params["c0"][0].data[...] = wt
    two.params["c0"][1].data[...] = 0
    for name in [n for n in two.params if n.startswith(("cls_score", "bbox_pred"))]:
        wb, bb = two.params[name]
        wb.data[...] = rng.normal(0, 1.0 / np.sqrt(128), wb.shape).astype(np.float32)
        bb.data[...] = 0
    lanes = [two, two.clone()]
    xs = [rng.normal(0, 1, (1, 128, 7, 9)).astype(np.float32) for _ in lanes]
    units = [(xs[0], 7, 9, 53, 67, 1.0, False), (xs[1], 7, 9, 53, 67, 1.3, True)]
    thresh = 0.05
    buf = torch.zeros((1024, 5), dtype=torch.float32, device="cuda")
    fused = {}
    two.detect_begin()
    two.detect_add_levels(lanes, units, thresh)
    n = two.detect_export(buf.data_ptr(), buf.shape[0])
    rows = buf[:n].cpu().numpy()
    assert len(rows) > 6
    for method in METHODS:
        two.detect_begin()
        two.detect_add_levels(lanes, units, thresh)
        fused[method] = two.detect_finish(method, 0.4)
    for m, u in zip(lanes, units):
        m.blobs["data"].reshape(*u[0].shape)
        m.blobs["im_info"].reshape(1, 3)
    two.forward_group(lanes, [dict(data=u[0], im_info=np.array([[u[3], u[4], u[5]]], np.float32)) for u in units])
    two.class_lists_begin()
    two.class_lists_add(lanes, [u[4] for u in units], [u[5] for u in units], [u[6] for u in units], thresh)
    assert two.class_lists_count() == [n]
    np.testing.assert_array_equal(two.class_lists_export(1).view(np.uint32), rows.view(np.uint32))
    n2 = two.class_lists_export(1, buf.data_ptr(), 3)                     # the device-buffer form: count back, cap honoured
    assert n2 == n
    for method in METHODS:
        got = two.class_lists_finish(1, method, 0.4)
        np.testing.assert_array_equal(np.asarray(got, np.float64), fused[method])


# ---- 5. the driver ---------------------------------------------------------------------------------------------------------------
def _driver_net(C):
    from smallhardface_amd import caffe
    txt = H.single_layer_net(M.conv3("conv_a", "data", 128) + M.tail("conv_a", C, 3, M.PSTR_A3), 3, 16, 16)
    msg = P.parse(txt)
    net = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(net, M.whole_params(msg))
    return net


@pytest.mark.parametrize("C", [3, 2])
def test_detect_with_device_merge_equals_plain_detect(C, monkeypatch):
    from smallhardface_amd import test as T
    for k in ("SHF_DEVICE_MERGE", "SHF_GROUPED_FORWARD", "SHF_DEVICE_LEVELS", "SHF_HOST_PREPROCESS"):
        monkeypatch.delenv(k, raising=False)
    net = _driver_net(C)
    im = np.random.default_rng(8).integers(0, 255, (40, 56, 3), dtype=np.uint8)
    for method in METHODS:
        cfg.TEST.PYRAMID_BASE_SIZE = [40, 56]
        cfg.TEST.SCALES = [40, 60]
        cfg.TEST.FLIP = True
        cfg.TEST.N_DETS_PER_MODULE = 300
        cfg.TEST.ANCHOR_MIN_SIZE = 0
        cfg.TEST.NMS_METHOD = method
        monkeypatch.delenv("SHF_DEVICE_MERGE", raising=False)
        want, _ = T.detect(net, None, thresh=0.4, pyramid=True, im=im)
        monkeypatch.setenv("SHF_DEVICE_MERGE", "1")
        got, _ = T.detect(net, None, thresh=0.4, pyramid=True, im=im)
        assert len(got) == len(want) == C - 1
        assert net.class_lists_count() != [0] * (C - 1)
        for g_, w_ in zip(got, want):
            assert len(w_) > 1
            assert g_.dtype == w_.dtype and g_.shape == w_.shape, method
            np.testing.assert_array_equal(g_, w_)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_and_what_they_leave_alone():
    import torch
    from smallhardface_amd import _lib, caffe
    three = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 3, 3, False))
    two = caffe.Net(None, prototxt_text=M.one_hot_net_txt(128, 7, 9, 2, 3, False))
    rng = np.random.default_rng(5)
    for net in (two, three):
        for name in [n for n in net.params if n.startswith(("cls_score", "bbox_pred"))]:
            wb, bb = net.params[name]
            wb.data[...] = rng.normal(0, 1.0 / np.sqrt(128), wb.shape).astype(np.float32)
            bb.data[...] = 0
    x = rng.normal(0, 1, (1, 128, 7, 9)).astype(np.float32)
    info = np.array([[53, 67, 1.0]], np.float32)
    unit = (x, 7, 9, 53, 67, 1.0, False)
    buf = torch.zeros((1024, 5), dtype=torch.float32, device="cuda")

    def two_class_pass():
        two.detect_begin()
        two.detect_add_levels([two], [unit], 0.05)
        n = two.detect_export(buf.data_ptr(), buf.shape[0])
        return buf[:n].cpu().numpy()

    def forward(net):
        net.blobs["data"].reshape(*x.shape)
        net.blobs["im_info"].reshape(1, 3)
        return {k: np.array(v) for k, v in net.forward(data=x, im_info=info).items()}

    before = two_class_pass()
    assert len(before) > 3
    three.class_lists_begin()
    ok = lambda n: ([67] * n, [1.0] * n, [False] * n, 0.05)
    with pytest.raises(RuntimeError, match=r"class_lists_add: member 0 has not completed a forward"):
        three.class_lists_add([three], *ok(1))
    out3 = forward(three)
    forward(two)
    with pytest.raises(_lib.ShfError, match=r"class_lists_add: 0 units: a group holds 1\.\.16"):
        three.class_lists_add([], *ok(0))
    with pytest.raises(_lib.ShfError, match=r"class_lists_add: 17 units: a group holds 1\.\.16"):
        three.class_lists_add([three] * 17, *ok(17))
    with pytest.raises(_lib.ShfError, match=r"debug_class_lists_add: 17 units: a group holds 1\.\.16"):
        three.debug_class_lists_add([np.zeros((1, 5))] * 17, [np.zeros((1, 3))] * 17, *ok(17))
    with pytest.raises(_lib.ShfError, match=r"class_lists_add: member 1 has not completed a forward"):
        three.class_lists_add([three, three.clone()], *ok(2))
    with pytest.raises(_lib.ShfError, match=r"class_lists_add: member 1 has 2 classes, the head 3"):
        three.class_lists_add([three, two], *ok(2))
    with pytest.raises(_lib.ShfError, match=r"class_lists_add: member 0 is NULL"):
        three.class_lists_add([object()], *ok(1))
    plain = caffe.Net(None, prototxt_text=H.single_layer_net(M.conv1("c0", "data", 128), 128))
    for call in (plain.class_lists_begin, plain.class_lists_count, lambda: plain.class_lists_finish(1, count=1),
                 lambda: plain.class_lists_add([three], *ok(1)), lambda: plain.class_lists_export(1)):
        with pytest.raises(_lib.ShfError, match=r"class_lists_\w+: net has no proposal layer"):
            call()
    with pytest.raises(_lib.ShfError, match=r"class_lists_add: member 0 has no proposal layer"):
        three.class_lists_add([plain], *ok(1))
    head = three.clone()
    forward(head)
    head.set_pipeline(True)
    for call in (head.class_lists_begin, lambda: head.class_lists_add([head], *ok(1)), head.class_lists_count,
                 lambda: head.class_lists_export(1), lambda: head.class_lists_finish(1, count=1)):
        with pytest.raises(_lib.ShfError, match=r"class_lists_\w+: the head has shf_net_set_pipeline enabled"):
            call()
    assert forward(head)["cls_prob"].shape == out3["cls_prob"].shape       # the refused head still forwards
    for cls in (0, 3, -1):
        with pytest.raises(_lib.ShfError, match=r"class_lists_export: class %d is outside 1\.\.2" % cls):
            three.class_lists_export(cls)
        with pytest.raises(_lib.ShfError, match=r"class_lists_finish: class %d is outside 1\.\.2" % cls):
            three.class_lists_finish(cls, count=1)
    # null pointers, straight at the C ABI
    lib, h = three._lib, three._h
    one_i, one_f, n_out = (ctypes.c_int * 1)(67), (ctypes.c_float * 1)(1.0), ctypes.c_int(0)
    mem = (ctypes.c_void_p * 1)(h)
    nulls = [
        (lambda: lib.shf_class_lists_begin(None), "class_lists_begin: NULL net"),
        (lambda: lib.shf_class_lists_add(h, 1, None, one_i, one_f, one_i, 0.05), "class_lists_add: NULL argument"),
        (lambda: lib.shf_class_lists_add(h, 1, mem, None, one_f, one_i, 0.05), "class_lists_add: NULL argument"),
        (lambda: lib.shf_debug_class_lists_add(h, 1, None, None, one_i, one_i, one_f, one_i, 0.05),
         "debug_class_lists_add: NULL argument"),
        (lambda: lib.shf_debug_class_lists_add(h, 1, (ctypes.c_void_p * 1)(None), (ctypes.c_void_p * 1)(None), one_i, one_i,
                                               one_f, one_i, 0.05), "debug_class_lists_add: unit 0: NULL boxes5 / probs"),
        (lambda: lib.shf_class_lists_count(h, None), "class_lists_count: NULL argument"),
        (lambda: lib.shf_class_lists_export(h, 1, None, 4), "class_lists_export: NULL argument"),
        (lambda: lib.shf_class_lists_finish(h, 1, 0, 0.4, None, 4, ctypes.byref(n_out)), "class_lists_finish: NULL argument"),
        (lambda: lib.shf_class_lists_finish(h, 1, 0, 0.4, (ctypes.c_double * 20)(), 4, None), "class_lists_finish: NULL argument"),
    ]
    for call, message in nulls:
        assert call() == -1
        assert _lib.last_error() == message
    # nothing above reached the lists; the refused head still forwards and its outputs still go into them
    assert three.class_lists_count() == [0, 0]
    np.testing.assert_array_equal(forward(three)["cls_prob"], out3["cls_prob"])
    three.class_lists_add([three], *ok(1))
    want = _np_lists([(out3["boxes"], out3["cls_prob"], 67, 1.0, False)], 3, 0.05)
    _assert_lists(three, want)
    assert sum(len(w) for w in want) > 3
    # the two-class net's fused pass is what it was, before and after class-list use on the same net
    two.class_lists_begin()
    two.class_lists_add([two], *ok(1))
    assert two.class_lists_count() == [len(before)]
    two.class_lists_finish(1, "BBOX_VOTE")
    np.testing.assert_array_equal(two_class_pass(), before)
    np.testing.assert_array_equal(two.class_lists_export(1), before)       # ... and the fused pass left the class list alone
