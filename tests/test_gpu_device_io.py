"""Device-resident inputs and outputs on the Net / Blob surface (run on an MI355X: ``pytest -m gpu``):
Blob.load_device (C ABI shf_blob_load_device -> csrc/blob_io.hip pad_flip_nchw_kernel), Blob.device (shf_blob_device_data),
Net.forward with a device input, forward_net / detect() on device-resident levels (shf_image_blobs_device,
SHF_DEVICE_LEVELS=1).

Nothing here changes any arithmetic: a level takes another road into the same blob, an activation another road out of it.
Every comparison is therefore ``assert_array_equal`` -- no tolerance.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import _lib, caffe
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import helpers as H

pytestmark = pytest.mark.gpu

# tops of the layers folded into the detection tail (net_internal.h BK_FUSED): host-side read-back only
TAIL_FUSED = {"cls_score_1_output", "cls_score_2_output", "cls_score_4_output", "bbox_pred_1_output", "bbox_pred_2_output",
              "bbox_pred_4_output", "cls_score_reshape_output", "cls_prob_output"}


@pytest.fixture(scope="module")
def net():
    """The small detector graph of the GPU parity tests with seeded synthetic parameters."""
    msg = H.detector_msg(True)
    n = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(n, O.synth_params(msg, seed=1234, cls_bias=1.0))
    return n


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def _rand(shape, seed):
    # signed values, -0.0 and a denormal among them: the kernel moves bit patterns
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[0] = -0.0
    if flat.size > 1:
        flat[-1] = np.float32(1e-41)
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- kernel exactness ---------------------------------------------------------------------------------------------------
PAD_CASES = [(1, 1, 16, 16),
             (16, 16, 16, 16),     # no padding
             (5, 3, 16, 16),       # w below one vector
             (17, 31, 32, 32),
             (33, 16, 48, 16),     # rows only
             (16, 45, 16, 48),     # columns only, odd w
             (40, 129, 48, 144),
             (7, 9, 7, 9),         # scalar path: W % 4 != 0
             (6, 10, 9, 10)]


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("h,w,HH,WW", PAD_CASES, ids=["%dx%d-%dx%d" % c for c in PAD_CASES])
def test_load_device_equals_np_pad(net, h, w, HH, WW, flip):
    src = _rand((2, 3, h, w), seed=h * 1000 + w)       # six planes: the plane index takes part in every offset
    b = net.blobs["data"]
    b.reshape(2, 3, HH, WW)
    b.data[...] = np.float32(7.0)                      # what the grow-only buffer "held before" on the host side ...
    b.load_device(_dev(np.full((2, 3, HH, WW), 9.0, np.float32)))    # ... and on the device: every element must be rewritten
    b.load_device(_dev(src), flip=flip)
    want = np.pad(src[..., ::-1] if flip else src, ((0, 0), (0, 0), (0, HH - h), (0, WW - w)), "constant")
    got = np.array(b.data)
    np.testing.assert_array_equal(_bits(got), _bits(want))          # bit patterns: -0.0 stays -0.0, the padding is +0.0


def test_flipped_view_and_flip_argument_xor(net):
    src = _rand((1, 3, 17, 31), seed=5)
    b = net.blobs["data"]
    b.reshape(1, 3, 32, 32)
    pad = lambda x: np.pad(x, ((0, 0), (0, 0), (0, 15), (0, 1)), "constant")
    a = caffe.DeviceArray(_dev(src))
    b.load_device(a[..., ::-1])
    np.testing.assert_array_equal(np.array(b.data), pad(src[..., ::-1]))
    b.load_device(a[..., ::-1], flip=True)
    np.testing.assert_array_equal(np.array(b.data), pad(src))
    np.testing.assert_array_equal(a[..., ::-1].numpy(), src[..., ::-1])
    np.testing.assert_array_equal(a.numpy(), src)


def test_padding_of_a_smaller_second_load_is_zero(net):
    b = net.blobs["data"]
    b.reshape(1, 3, 48, 144)
    b.load_device(_dev(np.ones((1, 3, 48, 144), np.float32)))
    np.testing.assert_array_equal(np.array(b.data), np.ones((1, 3, 48, 144), np.float32))
    src = _rand((1, 3, 17, 31), seed=6)
    b.load_device(_dev(src))
    got = np.array(b.data)
    np.testing.assert_array_equal(got[:, :, :17, :31], src)
    assert not got[:, :, 17:, :].any() and not got[:, :, :17, 31:].any()


# ---- refusals -----------------------------------------------------------------------------------------------------------
class _NullSource(object):
    __cuda_array_interface__ = {"shape": (1, 3, 8, 8), "typestr": "<f4", "data": (0, False), "version": 2, "strides": None}


def test_refusals_leave_the_net_usable(net):
    b = net.blobs["data"]
    b.reshape(1, 3, 16, 16)
    good = _rand((1, 3, 8, 8), seed=1)
    before = caffe.alloc_counts()
    with pytest.raises(_lib.ShfError, match="conv1_1.*not a 4-D net input"):
        net.blobs["conv1_1"].load_device(_dev(good))
    with pytest.raises(_lib.ShfError, match="im_info.*not a 4-D net input"):
        net.blobs["im_info"].load_device(_dev(good))
    with pytest.raises(_lib.ShfError, match="NULL"):
        b.load_device(_NullSource())
    with pytest.raises(_lib.ShfError, match=r"\(1, 3, \.\.\.\), the source \(1, 4"):
        b.load_device(_dev(np.zeros((1, 4, 8, 8), np.float32)))
    with pytest.raises(_lib.ShfError, match="16 x 16 planes, the source has 17 x 8"):
        b.load_device(_dev(np.zeros((1, 3, 17, 8), np.float32)))
    with pytest.raises(_lib.ShfError, match="16 x 16 planes, the source has 8 x 17"):
        b.load_device(_dev(np.zeros((1, 3, 8, 17), np.float32)))
    t = _dev(good)
    with pytest.raises(_lib.ShfError, match="flip must be 0 or 1"):
        _lib.check(net._lib.shf_blob_load_device(net._h, b._i, C.c_void_p(t.data_ptr()), 1, 3, 8, 8, 2), "load")
    assert caffe.alloc_counts() == before          # refused before anything was allocated or launched
    b.load_device(t)
    np.testing.assert_array_equal(np.array(b.data), np.pad(good, ((0, 0), (0, 0), (0, 8), (0, 8)), "constant"))


# ---- Blob.device against Blob.data ----------------------------------------------------------------------------------------
def _forward_80x112(net, mode, seed=3):
    net.set_conv_mode(mode)
    data = H.synth_image_blob(80, 112, seed=seed)
    info = np.array([[75, 101, 1.25]], np.float32)
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    out = net.forward(data=data, im_info=info)
    return data, info, {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_every_blob_reads_the_same_on_the_device(net, mode):
    import torch
    _forward_80x112(net, mode)
    assert net.conv_mode == mode
    fused, read = set(), []
    # (in "f16x3" the forward ran the fused path's kernels: the first NHWC blob read on the device goes through ensure_plain)
    for name, b in net.blobs.items():
        try:
            d = b.device                                     # the device read FIRST
        except _lib.ShfError as e:
            assert name in str(e) and "fused into the detection tail" in str(e)
            fused.add(name)
            continue
        assert d.shape == b.shape and not d.flipped
        got = d.numpy()
        t = torch.as_tensor(d, device="cuda")                # zero-copy: the very pointer
        assert t.data_ptr() == d.ptr and tuple(t.shape) == b.shape and t.dtype == torch.float32
        np.testing.assert_array_equal(_bits(got), _bits(b.data), err_msg=name)
        read.append(name)
    assert fused == TAIL_FUSED
    assert {"data", "im_info", "conv1_1", "pool1", "conv4_fuse_final", "head_4", "bbox_pred_output", "cls_prob_reshape_output",
            "boxes", "cls_prob"} <= set(read)
    for name in fused:                                       # their host-side read-back is untouched
        assert np.isfinite(net.blobs[name].data).all()


def test_nhwc_intermediate_after_a_fast_forward(net):
    """One NHWC activation after a fused-path ("f16x3") forward, device read first: the per-layer kernels run once
    (ensure_plain) and the transposed image equals Blob.data; a blob read on the host first reads the same on the device."""
    _forward_80x112(net, "f16x3", seed=4)
    b = net.blobs["conv3_3"]
    d = b.device
    assert d.shape == (1, 256, 20, 28)
    got = d.numpy()
    assert np.abs(got).max() > 0
    np.testing.assert_array_equal(got, b.data)
    host_first = np.array(net.blobs["conv2_2"].data)
    np.testing.assert_array_equal(net.blobs["conv2_2"].device.numpy(), host_first)


def test_device_data_of_a_net_that_never_ran():
    msg = H.detector_msg(True)
    fresh = caffe.Net(None, prototxt_text=P.dumps(msg))
    with pytest.raises(_lib.ShfError, match="conv1_1.*never forwarded"):
        fresh.blobs["conv1_1"].device
    with pytest.raises(_lib.ShfError, match="data.*never written"):
        fresh.blobs["data"].device
    x = _rand((1, 3, 224, 224), seed=8)
    fresh.blobs["data"].data[...] = x                       # a host write: gpu_data() uploads it
    np.testing.assert_array_equal(fresh.blobs["data"].device.numpy(), x)


# ---- Net.forward with a device input ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_forward_with_a_torch_tensor_equals_the_host_input(net, mode):
    data, info, want = _forward_80x112(net, mode, seed=9)
    assert len(want["boxes"]) > 1
    net.blobs["data"].data[...] = 0                          # nothing of the host run is left in the blob
    net.forward(data=np.zeros_like(data), im_info=info)
    t = _dev(data)
    net.timing = {}
    try:
        got = net.forward(data=t, im_info=info)
        tm = net.timing
    finally:
        net.timing = None
    assert tm["calls"] == 1 and tm["input_copy_s"] > 0
    for k in ("boxes", "cls_prob"):
        np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(np.array(net.blobs["data"].data), data)     # Blob.data reads the loaded level back
    # a DeviceArray, and the blob's own device image (nothing is copied): the same outputs again
    got = net.forward(data=caffe.DeviceArray(t), im_info=info)
    np.testing.assert_array_equal(got["boxes"], want["boxes"])
    got = net.forward(data=net.blobs["data"].device, im_info=info)
    for k in ("boxes", "cls_prob"):
        np.testing.assert_array_equal(got[k], want[k])


def test_forward_shape_and_batch_mismatch(net):
    data, info, want = _forward_80x112(net, "fp32", seed=10)
    with pytest.raises(ValueError, match=r"could not broadcast input array from shape \(1,3,75,101\) into shape \(1,3,80,112\)"):
        net.forward(data=_dev(np.zeros((1, 3, 75, 101), np.float32)), im_info=info)
    with pytest.raises(Exception, match="Input is not batch sized"):
        net.forward(data=_dev(np.zeros((2, 3, 80, 112), np.float32)), im_info=info)
    with pytest.raises(Exception, match="Input blob arguments do not match net inputs."):
        net.forward(data=_dev(data))
    got = net.forward(data=_dev(data), im_info=info)        # the net is still usable
    np.testing.assert_array_equal(got["boxes"], want["boxes"])


# ---- state ----------------------------------------------------------------------------------------------------------------
def test_intermediate_read_after_load_device_is_refused(net):
    data, info, want = _forward_80x112(net, "f16x3", seed=11)
    net.blobs["data"].load_device(_dev(H.synth_image_blob(80, 112, seed=12)))
    with pytest.raises(_lib.ShfError, match=r"an input was reshaped after the last forward\(\)"):
        net.blobs["conv1_1"].data
    with pytest.raises(_lib.ShfError, match=r"an input was reshaped after the last forward\(\)"):
        net.blobs["conv1_1"].device
    net.blobs["data"].load_device(_dev(data))
    got = net.forward()
    np.testing.assert_array_equal(got["boxes"], want["boxes"])
    assert net.blobs["conv1_1"].data.shape == (1, 64, 80, 112)


# ---- forward_net ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
def test_forward_net_device_level_equals_host_level(net, mode, flip):
    from smallhardface_amd import test as T
    net.set_conv_mode(mode)
    level = H.synth_image_blob(75, 101, seed=13)           # pads to 80 x 112
    host = {"data": level[..., ::-1] if flip else level}
    dev = caffe.DeviceArray(_dev(level))
    devb = {"data": dev[..., ::-1] if flip else dev}
    want_p, want_b = T.forward_net(net, host, 1.25, pyramid=True, flip=flip)
    want_p, want_b = [np.array(p) for p in want_p], [np.array(b) for b in want_b]
    net.forward(data=np.zeros((1, 3, 80, 112), np.float32), im_info=np.array([[75, 101, 1.25]], np.float32))
    got_p, got_b = T.forward_net(net, devb, 1.25, pyramid=True, flip=flip)
    assert net.blobs["data"].shape == (1, 3, 80, 112)
    assert len(got_p) == len(want_p) == 1 and len(want_p[0]) > 1
    np.testing.assert_array_equal(got_p[0], want_p[0])
    np.testing.assert_array_equal(got_b[0], want_b[0])


# ---- levels and detect() ------------------------------------------------------------------------------------------------------
def test_device_levels_equal_host_levels():
    from smallhardface_amd import test as T
    im = np.random.default_rng(14).integers(0, 256, (61, 83, 3)).astype(np.uint8)
    scales = (0.5, 1.0, 1.37)
    host = T._get_image_blob_device(im, scales)
    dev = T._get_image_blob_device(im, scales, on_device=True)
    assert len(dev) == len(host) == 3
    for hb, db in zip(host, dev):
        assert isinstance(db["data"], caffe.DeviceArray) and not db["data"].flipped
        assert db["data"].shape == hb["data"].shape
        np.testing.assert_array_equal(db["data"].numpy(), hb["data"])
    assert dev[1]["data"].shape == (1, 3, 61, 83)


@pytest.mark.parametrize("method", ["BBOX_VOTE", "NMS"])
def test_detect_with_device_levels_equals_the_default_path(net, method, monkeypatch):
    from smallhardface_amd import test as T
    net.set_conv_mode("f16x3")
    cfg.TEST.SCALES = [100, 300]                            # levels 100 x 130 (exactly 2x down: the area path) and 300 x 390
    cfg.TEST.NMS_METHOD = method
    rng = np.random.default_rng(15)
    im, im2 = (rng.integers(0, 256, (200, 260, 3)).astype(np.uint8) for _ in range(2))
    monkeypatch.delenv("SHF_DEVICE_LEVELS", raising=False)
    monkeypatch.delenv("SHF_HOST_PREPROCESS", raising=False)
    want, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im)
    want2, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im2)
    monkeypatch.setenv("SHF_DEVICE_LEVELS", "1")
    got, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im)
    before = caffe.alloc_counts()
    got2, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im2)
    assert caffe.alloc_counts() == before                   # a second image of the same shape allocates nothing
    assert len(want) == len(got) == 1 and len(want[0]) > 0
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got2[0], want2[0])
    # the switch yields to SHF_HOST_PREPROCESS=1 and to a non-uint8 image (the numpy mirror: host blobs, bit-equal levels)
    monkeypatch.setenv("SHF_HOST_PREPROCESS", "1")
    mirror, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im)
    np.testing.assert_array_equal(mirror[0], want[0])
