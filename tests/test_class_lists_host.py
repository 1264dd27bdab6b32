"""The per-class device lists (C ABI shf_class_lists_*, SHF_DEVICE_MERGE=1) as far as a machine without a GPU can see
them: the entry points are declared and exported, and detect() drives them -- one ``class_lists_add`` per chunk of
``group_units``, in unit order -- only when the switch is set.  The net is a stand-in that records what detect() calls."""
import numpy as np
import pytest

from smallhardface_amd import _lib
from smallhardface_amd import test as T
from smallhardface_amd.config import cfg

SYMBOLS = ["shf_class_lists_begin", "shf_class_lists_add", "shf_debug_class_lists_add", "shf_class_lists_count",
           "shf_class_lists_export", "shf_class_lists_finish"]


def test_the_entry_points_are_declared_and_exported():
    names = _lib.declared_symbols()
    lib = _lib.load(require_gpu=False)
    for s in SYMBOLS:
        assert s in names, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s          # ... and bound with a signature


def test_the_net_surface_has_the_methods():
    from smallhardface_amd import caffe
    for m in ("class_lists_begin", "class_lists_add", "debug_class_lists_add", "class_lists_count", "class_lists_export",
              "class_lists_finish"):
        assert callable(getattr(caffe.Net, m))


def test_the_kernels_build_for_gfx950_without_scratch_or_spills(tmp_path):
    """class_lists.hip compiled for the device with the build recipe's own flags, and the compiler's resource-usage remarks
    read: seven class counts x (count, scatter) + the scan, none with a private segment, none with a spilled register."""
    import os
    import re
    import subprocess
    from smallhardface_amd import build as B
    extra = dict(B.SOURCES)["class_lists.hip"]
    assert "-ffp-contract=off" in extra                              # the box arithmetic rounds like numpy
    cmd = [B.HIPCC, "--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           os.path.join(B.CSRC, "class_lists.hip"), "-o", str(tmp_path / "class_lists.o"),
           "-Rpass-analysis=kernel-resource-usage"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    tile = [k for k in kernels if "class_lists_tile_kernel" in k]
    scan = [k for k in kernels if "class_lists_scan_kernel" in k]
    assert len(tile) == 14 and len(scan) == 1 and len(kernels) == 15, sorted(kernels)
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)
        assert 0 < k["VGPRs"] <= 32 and k["LDS Size"] <= 7 * 4 * 4, (name, k)


class _Blob(object):
    def __init__(self, shape):
        self.data = np.zeros(shape, np.float32)

    @property
    def shape(self):
        return self.data.shape

    def reshape(self, *shape):
        if tuple(shape) != self.data.shape:
            self.data = np.zeros(shape, np.float32)


class _StandIn(object):
    """What detect() touches of a net.  A forward leaves three score rows (C classes) that depend on the unit's width;
    every call lands in ``log``, shared by the net and its lanes."""
    C = 3

    def __init__(self, log=None, name="net"):
        self.log = [] if log is None else log
        self.name = name
        self.n_clones = 0
        self.blobs = {"data": _Blob((1, 3, 1, 1)), "im_info": _Blob((1, 3)), "boxes": _Blob((3, 5)),
                      "cls_prob": _Blob((3, self.C))}

    num_classes = C

    def clone(self):
        self.n_clones += 1
        return _StandIn(self.log, "%s.lane%d" % (self.name, self.n_clones))

    def _run(self):
        w = float(self.blobs["data"].shape[3])
        self.blobs["boxes"].data[...] = [[0, 1, 2, w / 2, 9], [0, 2, 3, w / 3, 8], [0, 3, 4, w / 4, 7]]
        self.blobs["cls_prob"].data[...] = [[0.1, 0.8, 0.1], [0.2, 0.1, 0.7], [0.9, 0.06, 0.04]]
        return {"boxes": self.blobs["boxes"].data, "cls_prob": self.blobs["cls_prob"].data}

    def forward(self, **kw):
        self.log.append(("forward", self.name))
        return self._run()

    def forward_group(self, members):
        self.log.append(("forward_group", self.name, [m.name for m in members],
                         [tuple(m.blobs["data"].shape) for m in members]))
        return [m._run() for m in members]

    def class_lists_begin(self):
        self.log.append(("begin", self.name))

    def class_lists_add(self, members, im_w, im_scale, flip, thresh):
        self.log.append(("add", self.name, [m.name for m in members], list(im_w), list(im_scale), list(flip), thresh))

    def class_lists_count(self):
        self.log.append(("count", self.name))
        return [4, 0]

    def class_lists_finish(self, cls, method, nms_thresh, count=None):
        self.log.append(("finish", self.name, cls, method, nms_thresh, count))
        return np.full((1, 5), cls, np.float64)


@pytest.fixture
def small_pyramid(monkeypatch):
    """Nine levels x flip = 18 units of a 20 x 28 image (two chunks: 16 + 2), levels formed on the host, and the host merge
    replaced by a marker (bbox_vote needs the GPU)."""
    monkeypatch.setenv("SHF_HOST_PREPROCESS", "1")
    monkeypatch.delenv("SHF_DEVICE_MERGE", raising=False)
    monkeypatch.delenv("SHF_GROUPED_FORWARD", raising=False)
    monkeypatch.delenv("SHF_DEVICE_LEVELS", raising=False)
    cfg.TEST.PYRAMID_BASE_SIZE = [20, 28]
    cfg.TEST.SCALES = [10, 12, 14, 16, 18, 20, 22, 24, 26]
    cfg.TEST.FLIP = True
    cfg.TEST.NMS_METHOD = "BBOX_VOTE"
    monkeypatch.setattr(T, "bbox_vote", lambda dets: np.asarray(dets, np.float64))
    return np.random.default_rng(0).integers(0, 255, (20, 28, 3), dtype=np.uint8)


CLASS_LIST_CALLS = ("begin", "add", "count", "finish")


@pytest.mark.parametrize("grouped", [False, True], ids=["loop", "grouped"])
def test_detect_without_the_switch_never_touches_the_class_lists(small_pyramid, monkeypatch, grouped):
    if grouped:
        monkeypatch.setenv("SHF_GROUPED_FORWARD", "1")
    net = _StandIn()
    cls_dets, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=small_pyramid)
    assert len(cls_dets) == 2 and all(d.shape[1] == 5 for d in cls_dets)
    assert len(cls_dets[0]) == 3 * 18 and len(cls_dets[1]) == 2 * 18  # 3 / 2 rows of a unit above 0.05: the host merge ran
    calls = [e[0] for e in net.log]
    assert not set(calls) & set(CLASS_LIST_CALLS)
    assert calls == (["forward_group"] * 2 if grouped else ["forward"] * 18)
    # ... and a value other than "1" is not the switch
    monkeypatch.setenv("SHF_DEVICE_MERGE", "0")
    del net.log[:]
    T.detect(net, None, thresh=0.05, pyramid=True, im=small_pyramid)
    assert not set(e[0] for e in net.log) & set(CLASS_LIST_CALLS)


def test_detect_with_the_switch_adds_each_chunk_once_in_unit_order(small_pyramid, monkeypatch):
    monkeypatch.setenv("SHF_DEVICE_MERGE", "1")
    cfg.TEST.NMS_THRESH = 0.3
    net = _StandIn()
    cls_dets, timers = T.detect(net, None, thresh=0.25, pyramid=True, im=small_pyramid)
    chunks = T.group_units(9, True, T.GROUP_UNITS)
    assert [len(c) for c in chunks] == [16, 2]
    scales = T.pyramid_scales(small_pyramid.shape)
    lane_names = ["net"] + ["net.lane%d" % i for i in range(1, 16)]
    want, widths_seen = [("begin", "net")], []
    for ch in chunks:
        members = lane_names[:len(ch)]
        widths = [T.caffe.pyramid_level_shape(20, 28, scales[i], 1)[1] for i, _ in ch]
        widths_seen += widths
        shapes = [(1, 3) + T.caffe.pyramid_level_shape(20, 28, scales[i], cfg.MAX_RESOLUTION)[2:] for i, _ in ch]
        want.append(("forward_group", "net", members, shapes))
        want.append(("add", "net", members, widths, [scales[i] for i, _ in ch], [f for _, f in ch], 0.25))
    want += [("count", "net"), ("finish", "net", 1, "BBOX_VOTE", 0.3, 4), ("finish", "net", 2, "BBOX_VOTE", 0.3, 0)]
    assert net.log == want
    assert len(set(widths_seen)) > 4                                   # the widths tell the units apart
    # the result is what the finishes returned, class 1 first; nothing went through the host merge
    assert [d.tolist() for d in cls_dets] == [[[1.0] * 5], [[2.0] * 5]]
    assert timers["detect"].calls == 1 and timers["misc"].calls == 1


def test_the_switch_leaves_level_subsets_and_single_scale_detection_on_the_host(small_pyramid, monkeypatch):
    monkeypatch.setenv("SHF_DEVICE_MERGE", "1")
    net = _StandIn()
    cfg.TEST.LEVEL = ["3"]
    T.detect(net, None, thresh=0.05, pyramid=True, im=small_pyramid)
    assert not set(e[0] for e in net.log) & set(CLASS_LIST_CALLS) and len(net.log) == 18
    cfg.TEST.LEVEL = []
    del net.log[:]
    with pytest.raises(NotImplementedError):                           # the reference's single-scale path
        T.detect(net, None, thresh=0.05, pyramid=False, im=small_pyramid)
    assert not set(e[0] for e in net.log) & set(CLASS_LIST_CALLS)
    # an unknown merge method is refused before anything is forwarded
    cfg.TEST.NMS_METHOD = "SOFT"
    del net.log[:]
    with pytest.raises(NotImplementedError, match="Unknown NMS method: SOFT"):
        T.detect(net, None, thresh=0.05, pyramid=True, im=small_pyramid)
    assert net.log == []
