"""Grouped Net.forward over lanes (run on an MI355X: ``pytest -m gpu``): Net.forward_group (C ABI shf_net_forward_group),
caffe.load_device_group (shf_blob_load_device_group -> csrc/blob_io.hip pad_flip_nchw_group_kernel), test.forward_net_group
and detect() under SHF_GROUPED_FORWARD=1.

Nothing here changes any arithmetic: the same units take one grouped pass instead of one forward each, and results are
bit-identical across groupings.  Every comparison is therefore ``assert_array_equal`` -- no tolerance.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import _lib, caffe
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import helpers as H
from tests.test_gpu_device_io import PAD_CASES

pytestmark = pytest.mark.gpu

SIZES = [(80, 112), (112, 80), (32, 48), (48, 32)]
MODES = ["f16x3", "fp32", "f64"]


def _new_net():
    msg = H.detector_msg(True)
    n = caffe.Net(None, prototxt_text=P.dumps(msg))
    H.load_params(n, O.synth_params(msg, seed=1234, cls_bias=1.0))
    return n


@pytest.fixture(scope="module")
def lanes():
    """The small detector graph of the GPU parity tests with seeded synthetic parameters, and 15 lanes of it."""
    root = _new_net()
    return [root] + [root.clone() for _ in range(15)]


@pytest.fixture(scope="module")
def single():
    """(mode, unit index) -> what forward() of a net that never takes part in a group returns for that unit; computed once."""
    net, cache = _new_net(), {}

    def get(mode, k, data=None, info=None):
        key = (mode, k)
        if key not in cache:
            net.set_conv_mode(mode)
            d, i = _unit(k) if data is None else (data, info)
            net.blobs["data"].reshape(*d.shape)
            net.blobs["im_info"].reshape(1, 3)
            out = {name: np.array(v) for name, v in net.forward(data=d, im_info=i).items()}
            if k < 4:      # an NHWC intermediate (read through ensure_plain after a fast forward) and a tail-fused blob
                out["conv3_3"] = np.array(net.blobs["conv3_3"].data)
                out["cls_prob_output"] = np.array(net.blobs["cls_prob_output"].data)
            cache[key] = out
        return cache[key]
    return get


def _unit(k):
    """Unit k of 16: the four sizes, then their mirrors, then both again from other seeds."""
    h, w = SIZES[k % 4]
    data = H.synth_image_blob(h, w, seed=50 + (k // 8) * 4 + k % 4)
    if (k // 4) % 2:
        data = np.ascontiguousarray(data[..., ::-1])
    return data, np.array([[h - 5, w - 11, 1.25]], np.float32)


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


def _inputs(members, first=0, scale=None):
    """Input dicts for units first .. : even members get host arrays, odd ones a torch tensor or a DeviceArray of it."""
    inputs = []
    for j, m in enumerate(members):
        data, info = _unit(first + j)
        if scale and j in scale:
            data = data * np.float32(scale[j])
        m.blobs["data"].reshape(*data.shape)
        m.blobs["im_info"].reshape(1, 3)
        if j % 2:
            t = _dev(data)
            data = caffe.DeviceArray(t) if j % 4 == 1 else t
        inputs.append({"data": data, "im_info": info})
    return inputs


def _check_outputs(members, outs, single, mode, first=0):
    some = 0
    for j, (m, out) in enumerate(zip(members, outs)):
        want = single(mode, first + j)
        assert set(out) == {"boxes", "cls_prob"}
        for name in ("boxes", "cls_prob"):
            assert out[name].shape == want[name].shape, (j, name)
            np.testing.assert_array_equal(out[name], want[name], err_msg="member %d %s" % (j, name))
            np.testing.assert_array_equal(m.blobs[name].data, want[name])
        some = max(some, len(want["cls_prob"]))
    assert some > 1


# ---- 1. the grouped load ----------------------------------------------------------------------------------------------------
GROUP5 = [PAD_CASES[7], PAD_CASES[1], PAD_CASES[5], PAD_CASES[6], PAD_CASES[3]]
assert GROUP5[0] == (7, 9, 7, 9) and GROUP5[1] == (16, 16, 16, 16) and GROUP5[2] == (16, 45, 16, 48)


@pytest.mark.parametrize("cases", [GROUP5, [PAD_CASES[6]], [PAD_CASES[i % len(PAD_CASES)] for i in range(16)]],
                         ids=["n5", "n1", "n16"])
def test_group_load_equals_np_pad(lanes, cases):
    nets = lanes[:len(cases)]
    flips = [bool((i * 5 + 1) % 3 % 2) for i in range(len(cases))]          # mixed
    assert len(cases) == 1 or (True in flips and False in flips)
    srcs, fills = [], []
    for i, (net, (h, w, HH, WW)) in enumerate(zip(nets, cases)):
        nn = 2 if i == 3 % len(cases) else 1                                  # one member with 2 x 3 planes
        net.blobs["data"].reshape(nn, 3, HH, WW)
        srcs.append(_rand((nn, 3, h, w), seed=h * 1000 + w + i))
        fills.append(np.full((nn, 3, HH, WW), 9.0, np.float32))
    caffe.load_device_group(nets, "data", [_dev(f) for f in fills])           # what the grow-only buffers "held before"
    for net, f in zip(nets, fills):
        np.testing.assert_array_equal(np.array(net.blobs["data"].data), f)
    caffe.load_device_group(nets, "data", [_dev(s) for s in srcs], flips)
    for net, s, f, (h, w, HH, WW) in zip(nets, srcs, flips, cases):
        want = np.pad(s[..., ::-1] if f else s, ((0, 0), (0, 0), (0, HH - h), (0, WW - w)), "constant")
        got = np.array(net.blobs["data"].data)
        np.testing.assert_array_equal(_bits(got), _bits(want))               # -0.0 stays -0.0, the padding is +0.0
    for net in nets:
        net.blobs["data"].reshape(1, 3, 32, 48)


def test_group_load_flipped_view_xor(lanes):
    src = _rand((1, 3, 17, 31), seed=5)
    pad = lambda x: np.pad(x, ((0, 0), (0, 0), (0, 15), (0, 1)), "constant")
    for net in lanes[:2]:
        net.blobs["data"].reshape(1, 3, 32, 32)
    a = caffe.DeviceArray(_dev(src))
    caffe.load_device_group(lanes[:2], "data", [a[..., ::-1], a[..., ::-1]], [False, True])
    np.testing.assert_array_equal(np.array(lanes[0].blobs["data"].data), pad(src[..., ::-1]))
    np.testing.assert_array_equal(np.array(lanes[1].blobs["data"].data), pad(src))
    own = lanes[0].blobs["data"].device
    with pytest.raises(ValueError, match="cannot mirror blob 'data' into itself"):
        caffe.load_device_group(lanes[:1], "data", [own], [True])
    caffe.load_device_group(lanes[:1], "data", [own])                          # its own image: left in place
    np.testing.assert_array_equal(np.array(lanes[0].blobs["data"].data), pad(src[..., ::-1]))


# ---- 2. forward_group == single forwards ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("mode", MODES)
def test_forward_group_equals_single_forwards(lanes, single, mode, n):
    root = lanes[0]
    root.set_conv_mode(mode)
    members = lanes[:n]
    outs = root.forward_group(members, _inputs(members))
    assert root.conv_mode == mode and len(outs) == n
    _check_outputs(members, outs, single, mode)
    j = 1 if n > 1 else 0
    want = single(mode, j)
    for name in ("conv3_3", "cls_prob_output"):
        got = np.array(members[j].blobs[name].data)
        assert np.abs(got).max() > 0
        np.testing.assert_array_equal(got, want[name], err_msg=name)
    assert not members[j]._dev_sources                                         # released after the call


def test_head_need_not_be_a_member(lanes, single):
    lanes[0].set_conv_mode("f16x3")
    members = lanes[1:3]
    outs = lanes[7].forward_group(members, _inputs(members, first=2))
    _check_outputs(members, outs, single, "f16x3", first=2)


def test_forward_group_input_checks_are_forwards(lanes):
    lanes[0].set_conv_mode("fp32")
    members = lanes[:2]
    good = _inputs(members)
    info = good[0]["im_info"]
    with pytest.raises(Exception, match="Input blob arguments do not match net inputs."):
        lanes[0].forward_group(members, [good[0], {"data": good[1]["data"]}])
    with pytest.raises(Exception, match="Input is not batch sized"):
        lanes[0].forward_group(members, [good[0], {"data": _dev(np.zeros((2, 3, 112, 80), np.float32)), "im_info": info}])
    with pytest.raises(ValueError, match=r"could not broadcast input array from shape \(1,3,75,101\) into shape \(1,3,112,80\)"):
        lanes[0].forward_group(members, [good[0], {"data": _dev(np.zeros((1, 3, 75, 101), np.float32)), "im_info": info}])
    with pytest.raises(ValueError, match="2 members but 1 input dicts"):
        lanes[0].forward_group(members, [good[0]])


# ---- 3. one launch per layer ------------------------------------------------------------------------------------------------
def test_one_launch_per_layer(lanes):
    root = lanes[0]
    root.set_conv_mode("f16x3")
    members = lanes[:4]
    host = [_unit(j) for j in range(4)]
    inputs = [{"data": d, "im_info": i} for d, i in host]
    for m, (d, _) in zip(members, host):
        m.blobs["data"].reshape(*d.shape)
        m.blobs["im_info"].reshape(1, 3)
    conv = lambda pr: {k: v["launches"] for k, v in pr.items() if k.startswith("conv_") or k in ("deconv_depthwise", "maxpool_kernel")}
    root.forward_group(members, inputs)
    root.prof_enable(True)
    try:
        root.prof_reset()
        root.forward_group(members, inputs)
        grouped = conv(root.prof_read())
        root.prof_reset()
        root.detect_begin()
        root.detect_add_levels(members, [(d, d.shape[2], d.shape[3], int(i[0, 0]), int(i[0, 1]), float(i[0, 2]), False)
                                         for d, i in host], 0.05)
        root.detect_finish()
        levels = conv(root.prof_read())
        root.prof_reset()
        root.forward(**inputs[0])
        one = conv(root.prof_read())
    finally:
        root.prof_enable(False)
        root.prof_reset()
    print("conv-class launches: grouped %d, add_levels %d, single forward %d"
          % (sum(grouped.values()), sum(levels.values()), sum(one.values())))
    assert sum(one.values()) > 10
    assert grouped == levels
    assert sum(grouped.values()) < 4 * sum(one.values())


# ---- 4. members are ordinary nets afterwards --------------------------------------------------------------------------------
def test_members_are_ordinary_nets_afterwards(lanes, single):
    from smallhardface_amd import test as T
    root = lanes[0]
    root.set_conv_mode("f16x3")
    members = lanes[:4]
    outs = root.forward_group(members, _inputs(members))
    np.testing.assert_array_equal(np.array(members[2].blobs["conv3_3"].data), single("f16x3", 2)["conv3_3"])
    _check_outputs(members, outs, single, "f16x3")                             # the others (and member 2's outputs) untouched
    # a plain forward() on member 1 with a new shape
    data, info = H.synth_image_blob(48, 64, seed=77), np.array([[45, 60, 0.75]], np.float32)
    want = single("f16x3", 100, data, info)
    members[1].blobs["data"].reshape(*data.shape)
    got = members[1].forward(data=data, im_info=info)
    for name in ("boxes", "cls_prob"):
        np.testing.assert_array_equal(got[name], want[name])
    # a fused pass on the root afterwards equals a fresh net's: the activation-exponent slots were left zeroed
    units = [(d, d.shape[2], d.shape[3], int(i[0, 0]), int(i[0, 1]), float(i[0, 2]), bool(k % 2))
             for k, (d, i) in enumerate(_unit(j) for j in range(4))]
    fresh = _new_net()
    fresh.set_conv_mode("f16x3")
    a, b = T.detect_fused(root, units, thresh=0.05)[0], T.detect_fused(fresh, units, thresh=0.05)[0]
    assert len(b) > 0
    np.testing.assert_array_equal(a, b)


# ---- 5. range guard ---------------------------------------------------------------------------------------------------------
def test_range_guard_redoes_the_whole_group_in_fp32(lanes, single):
    root = lanes[0]
    root.set_conv_mode("f16x3")
    members = lanes[:4]
    # member 2's input x 2e5: conv1_1's outputs are far beyond 65504 (the synthetic first layer has a gain of ~0.1)
    inputs = _inputs(members, scale={2: 2.0e5})
    before = root.range_fallbacks
    outs = root.forward_group(members, inputs)
    assert root.range_fallbacks == before + 1 and root.conv_mode == "f16x3"
    for j, (m, out) in enumerate(zip(members, outs)):
        d, i = _unit(j)
        if j == 2:
            d = d * np.float32(2.0e5)
        want = single("fp32", 200 + j, d, i) if j == 2 else single("fp32", j)
        for name in ("boxes", "cls_prob"):
            np.testing.assert_array_equal(out[name], want[name], err_msg="member %d %s" % (j, name))
            assert np.isfinite(out[name]).all()
        for name in ("conv1_1", "conv3_3", "conv5_3", "cls_prob_reshape_output", "bbox_pred_output"):
            assert np.isfinite(m.blobs[name].data).all(), (j, name)
    np.testing.assert_array_equal(np.array(members[1].blobs["conv3_3"].data), single("fp32", 1)["conv3_3"])
    # the next group is clean again, in the mode that was set
    n0 = root.range_fallbacks
    outs = root.forward_group(members, _inputs(members))
    assert root.range_fallbacks == n0
    _check_outputs(members, outs, single, "f16x3")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
class _NullSource(object):
    __cuda_array_interface__ = {"shape": (1, 3, 8, 8), "typestr": "<f4", "data": (0, False), "version": 2, "strides": None}


def test_refusals_leave_the_nets_usable(lanes, single):
    root = lanes[0]
    root.set_conv_mode("f16x3")
    members = lanes[:4]
    root.forward_group(members, _inputs(members))
    other = _new_net()
    stranger = other.clone()
    good = _dev(_rand((1, 3, 8, 8), seed=1))
    big = _dev(np.zeros((1, 3, 49, 32), np.float32))
    before = caffe.alloc_counts()
    with pytest.raises(_lib.ShfError, match="0 members"):
        root.forward_group([])
    with pytest.raises(_lib.ShfError, match="17 members"):
        root.forward_group(lanes + [lanes[0]])
    with pytest.raises(_lib.ShfError, match="members 0 and 2 are the same net"):
        root.forward_group([lanes[0], lanes[1], lanes[0]])
    with pytest.raises(_lib.ShfError, match="member 1 does not share"):
        root.forward_group([lanes[0], stranger])
    with pytest.raises(_lib.ShfError, match="member 1 does not share"):
        caffe.load_device_group([lanes[0], stranger], "data", [good, good])
    with pytest.raises(_lib.ShfError, match="member 1: .*NULL source"):
        caffe.load_device_group(members, "data", [good, _NullSource(), good, good])
    # member 3 holds 48 x 32 planes
    with pytest.raises(_lib.ShfError, match="member 3: .*holds 48 x 32 planes, the source has 49 x 32"):
        caffe.load_device_group(members, "data", [good, good, good, big])
    with pytest.raises(_lib.ShfError, match=r"member 2: .*is \(1, 3, \.\.\.\), the source \(1, 4"):
        caffe.load_device_group(members, "data", [good, good, _dev(np.zeros((1, 4, 8, 8), np.float32)), good])
    assert caffe.alloc_counts() == before          # refused before anything was allocated or launched
    outs = root.forward_group(members, _inputs(members))
    _check_outputs(members, outs, single, "f16x3")


# ---- 7. no allocation on repeat ---------------------------------------------------------------------------------------------
def test_no_allocation_on_repeat(lanes, single):
    root = lanes[0]
    root.set_conv_mode("f16x3")
    root.forward_group(lanes, _inputs(lanes))
    before = caffe.alloc_counts()
    outs = root.forward_group(lanes, _inputs(lanes))
    assert caffe.alloc_counts() == before
    _check_outputs(lanes, outs, single, "f16x3")


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_net():
    n = _new_net()
    n.set_conv_mode("f16x3")
    return n


def _detect_all_ways(net, im, monkeypatch):
    from smallhardface_amd import test as T
    for k in ("SHF_DEVICE_LEVELS", "SHF_HOST_PREPROCESS", "SHF_GROUPED_FORWARD"):
        monkeypatch.delenv(k, raising=False)
    want, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im)
    monkeypatch.setenv("SHF_GROUPED_FORWARD", "1")
    host, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im)
    monkeypatch.setenv("SHF_DEVICE_LEVELS", "1")
    dev, _ = T.detect(net, None, thresh=0.05, pyramid=True, im=im)
    monkeypatch.delenv("SHF_GROUPED_FORWARD")
    monkeypatch.delenv("SHF_DEVICE_LEVELS")
    assert len(want) == len(host) == len(dev) == 1 and len(want[0]) > 0
    np.testing.assert_array_equal(host[0], want[0])
    np.testing.assert_array_equal(dev[0], want[0])
    return want


@pytest.mark.parametrize("method", ["BBOX_VOTE", "NMS"])
@pytest.mark.parametrize("flip", [True, False], ids=["flip", "plain"])
def test_detect_grouped_equals_the_default_path(driver_net, flip, method, monkeypatch):
    from smallhardface_amd import test as T
    cfg.TEST.SCALES = [100, 200, 300]
    cfg.TEST.FLIP = flip
    cfg.TEST.NMS_METHOD = method
    im = np.random.default_rng(21).integers(0, 256, (96, 128, 3)).astype(np.uint8)
    want = _detect_all_ways(driver_net, im, monkeypatch)
    assert (6 if flip else 3) <= len(driver_net._group_lanes) <= 16          # cached on the net, grown on demand
    fused = T.detect_fused(driver_net, list(T.pyramid_units(im)), thresh=0.05)
    assert want[0].shape == fused[0].shape
    np.testing.assert_array_equal(np.asarray(want[0], dtype=np.float64), fused[0])


def test_detect_grouped_with_two_passes(driver_net, monkeypatch):
    from smallhardface_amd import test as T
    cfg.TEST.SCALES = [60, 80, 100, 120, 140, 160, 180, 200, 220]             # x flip: 18 units, passes of 16 and 2
    cfg.TEST.FLIP = True
    assert [len(c) for c in T.group_units(len(cfg.TEST.SCALES), True)] == [16, 2]
    im = np.random.default_rng(22).integers(0, 256, (96, 128, 3)).astype(np.uint8)
    _detect_all_ways(driver_net, im, monkeypatch)
    assert len(driver_net._group_lanes) == 16


# ---- 9. one forward path: forward() is a group of one ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x3", "fp32"])
def test_group_of_one_launches_what_forward_launches(lanes, mode):
    """Per-class launch counts of forward() and of forward_group([root]) on the same host inputs, each after one warm call:
    equal in every class but d2h_copy (only the group fills the proposal outputs' host mirrors itself, behind one
    synchronisation; after forward() each Blob.data copies its own)."""
    root = lanes[0]
    root.set_conv_mode(mode)
    data, info = _unit(2)
    assert data.shape[2:] == (32, 48)
    root.blobs["data"].reshape(*data.shape)
    root.blobs["im_info"].reshape(1, 3)
    inp = {"data": data, "im_info": info}

    def counts(run):
        run()
        root.prof_reset()
        run()
        return {k: v["launches"] for k, v in root.prof_read().items() if k != "d2h_copy"}
    root.prof_enable(True)
    try:
        one = counts(lambda: root.forward(**inp))
        grouped = counts(lambda: root.forward_group([root], [inp]))
    finally:
        root.prof_enable(False)
        root.prof_reset()
    print("launches per class (%s): forward %r" % (mode, {k: v for k, v in one.items() if v}))
    print("launches per class (%s): group of one %r" % (mode, {k: v for k, v in grouped.items() if v}))
    assert sum(one.values()) > 10 and one["h2d_copy"] > 0
    assert grouped == one


def test_pipelined_head_forwards_alone_and_refuses_a_group(single):
    """check_group is the group's alone: a head with shf_net_set_pipeline enabled still runs forward(), on its own stream."""
    net = _new_net()                    # (not a lane of the module's: set_pipeline replaces the net's stream)
    net.set_conv_mode("f16x3")
    data, info = _unit(2)
    want = single("f16x3", 2)
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    net.set_pipeline(True)
    out = net.forward(data=data, im_info=info)
    for name in ("boxes", "cls_prob"):
        np.testing.assert_array_equal(out[name], want[name], err_msg=name)
    assert len(want["cls_prob"]) > 1
    with pytest.raises(_lib.ShfError, match="shf_net_set_pipeline enabled"):
        net.forward_group([net])
    net.set_pipeline(False)
    out = net.forward_group([net])[0]
    for name in ("boxes", "cls_prob"):
        np.testing.assert_array_equal(out[name], want[name], err_msg=name)
