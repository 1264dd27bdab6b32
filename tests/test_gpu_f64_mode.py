"""Conv mode "f64" (shf_net_set_conv_mode 5): out = fl32(bias + sum a*w) with the products and the sum in binary64
(csrc/conv_f64.h, the binary64 instantiation of the tail's logits kernel, the binary64 depthwise deconvolution).

Bounds.  A product of two fp32 values is exact in binary64, so against the float64 numpy result `ref` formed from the same
fp32 inputs only the two summation orders (each at most (K + 1) 2^-53 sum|a w|) and the one rounding to fp32 differ:

    |got - fl32(ref)| <= ulp32(ref) + 2 (K + 1) 2^-53 sum|a w|

On integer data with every partial sum below 2^24 nothing rounds at all: the result is exact, which also proves the f64
MFMA's fragment maps, the zero fill of the K tail and the masking of the edge tiles.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd.config import cfg
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bars of tests/test_gpu_parity.py (test_detector_end_to_end holds the fp32 mode to them)
SCORE_TOL = 1e-4
BOX_TOL = 1e-3

# (Cin, Cout, k, dilation, H, W, first): `first` = the layer reads the NCHW net input itself (the first-layer class);
# otherwise an exact 1x1 identity layer turns the input into the NHWC activation the layer under test reads
INT_SHAPES = [
    (3, 64, 3, 1, 5, 7, True),        # the NCHW first layer, K = 27: seven K steps, the last one zero-filled
    (8, 6, 3, 1, 1, 1, False),        # one pixel, Cout below one MFMA tile (direct class)
    (64, 64, 3, 1, 17, 33, False),    # MFMA class, ragged tiles in H and W, several blocks
    (64, 128, 3, 2, 16, 16, False),   # dilation 2, two cout tiles
    (128, 128, 3, 4, 9, 20, False),   # dilation 4, a map barely larger than the halo
    (128, 12, 1, 1, 17, 33, False),   # 1x1, Cout 12 (direct class)
    (6, 20, 1, 1, 3, 3, False),       # 1x1, K = 6: a zero-filled K step, Cout 20 = one MFMA tile + 4
]
RANDOM_SHAPES = INT_SHAPES + [(512, 512, 3, 1, 8, 8, False)]   # K = 4608, all-positive inputs: no cancellation hides an error


def _conv_txt(name, bottom, nout, k, dil, relu):
    s = ('layer { name: "%s" type: "Convolution" bottom: "%s" top: "%s" convolution_param { num_output: %d '
         'kernel_size: %d pad: %d dilation: %d } }\n' % (name, bottom, name, nout, k, dil if k == 3 else 0, dil))
    if relu:
        s += 'layer { name: "%s_relu" type: "ReLU" bottom: "%s" top: "%s" }\n' % (name, name, name)
    return s


def _f64_net(txt):
    from smallhardface_amd import caffe
    net = caffe.Net(None, prototxt_text=txt)
    net.set_conv_mode("f64")
    assert net.conv_mode == "f64"
    return net


def _one_layer_net(cin, cout, k, dil, h, w, first, relu):
    layers = "" if first else _conv_txt("c0", "data", cin, 1, 1, False)
    layers += _conv_txt("c1", "data" if first else "c0", cout, k, dil, relu)
    net = _f64_net(H.single_layer_net(layers, cin, h, w))
    if not first:
        net.params["c0"][0].data[...] = np.eye(cin, dtype=np.float32).reshape(cin, cin, 1, 1)
        net.params["c0"][1].data[...] = 0
    return net


def _conv_ref(x, w, b, dil, dtype):
    """(sum a*w + b, sum |a*w|) of a stride-1 "same" convolution in `dtype`; x (C, H, W), w (Co, C, k, k)."""
    k = w.shape[2]
    pad = dil * (k // 2)
    xp = np.pad(x.astype(dtype), ((0, 0), (pad, pad), (pad, pad)))
    wd = w.astype(dtype)
    Hh, Ww = x.shape[1:]
    out = np.zeros((w.shape[0], Hh, Ww), dtype)
    mag = np.zeros((w.shape[0], Hh, Ww), dtype)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, ky * dil:ky * dil + Hh, kx * dil:kx * dil + Ww]
            out += np.einsum("oc,chw->ohw", wd[:, :, ky, kx], win)
            mag += np.einsum("oc,chw->ohw", np.abs(wd[:, :, ky, kx]), np.abs(win))
    return out + b.astype(dtype)[:, None, None], mag


def _assert_within_f64_bound(got, ref, mag, K, relu, what):
    """|got - fl32(ref)| <= ulp32(ref) + 2 (K + 1) 2^-53 sum|a w| for every element (figures printed before the assertion)."""
    r32 = ref.astype(np.float32)
    bound = np.spacing(np.abs(r32)).astype(np.float64) + 2.0 * (K + 1) * 2.0 ** -53 * mag
    want = np.maximum(r32, 0) if relu else r32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = int(np.argmax(err - bound))
    print("%s: K %d, %d elements, %d not bit-equal to fl32(ref), max err %.3e (bound there %.3e)"
          % (what, K, err.size, int((got != want).sum()), float(err.flat[worst]), float(bound.flat[worst])))
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (what, float(err.flat[worst]), float(bound.flat[worst]))


def _forward(net, data, info=None):
    h, w = data.shape[2:]
    info = np.array([[h, w, 1]], np.float32) if info is None else info
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(*info.shape)
    return net.forward(data=data, im_info=info)


# ---- 1. exact on integers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("cin,cout,k,dil,h,w,first", INT_SHAPES)
def test_integer_data_is_exact(cin, cout, k, dil, h, w, first, relu):
    rng = np.random.default_rng(cin * 1000 + cout + 7 * dil + h)
    net = _one_layer_net(cin, cout, k, dil, h, w, first, relu)
    wt = rng.integers(-8, 9, (cout, cin, k, k)).astype(np.float32)
    bs = rng.integers(-8, 9, (cout,)).astype(np.float32)
    data = rng.integers(-8, 9, (1, cin, h, w)).astype(np.float32)
    net.params["c1"][0].data[...] = wt
    net.params["c1"][1].data[...] = bs
    out = _forward(net, data)
    ref, mag = _conv_ref(data[0].astype(np.int64), wt.astype(np.int64), bs.astype(np.int64), dil, np.int64)
    assert int(mag.max()) + 8 < 2 ** 24
    if relu:
        ref = np.maximum(ref, 0)
    else:
        assert (ref < 0).any()
    np.testing.assert_array_equal(out["c1"][0].astype(np.int64), ref)
    np.testing.assert_array_equal(out["c1"][0], ref.astype(np.float32))
    if not first:   # the 1x1 identity through the first-layer class: the input itself
        np.testing.assert_array_equal(net.blobs["c0"].data, data)


# ---- 2. random data, per element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k,dil,h,w,first", RANDOM_SHAPES)
def test_random_data_per_element_bound(cin, cout, k, dil, h, w, first):
    rng = np.random.default_rng(cin + 31 * cout + dil)
    relu = (cin + cout) % 3 != 0
    net = _one_layer_net(cin, cout, k, dil, h, w, first, relu)
    wt = rng.normal(0, 1.0 / np.sqrt(cin * k * k), (cout, cin, k, k)).astype(np.float32)
    bs = rng.normal(0, 0.5, (cout,)).astype(np.float32)
    data = rng.normal(0, 1, (1, cin, h, w)).astype(np.float32)
    if cin == 512:
        data, wt = np.abs(data) + 0.5, np.abs(wt)
    net.params["c1"][0].data[...] = wt
    net.params["c1"][1].data[...] = bs
    out = _forward(net, data)
    ref, mag = _conv_ref(data[0], wt, bs, dil, np.float64)
    _assert_within_f64_bound(out["c1"][0], ref, mag, cin * k * k, relu, "conv %d->%d k%d d%d %dx%d" % (cin, cout, k, dil, h, w))


# ---- 3. deconvolution and tail predictors ---------------------------------------------------------------------------------
def test_depthwise_deconvolution_per_element_bound():
    C_, h, w = 12, 5, 7
    txt = H.single_layer_net(
        _conv_txt("c0", "data", C_, 1, 1, False) +
        'layer { name: "up" type: "Deconvolution" bottom: "c0" top: "up" convolution_param { kernel_size: 4 stride: 2 '
        'num_output: %d group: %d pad: 1 } }\n' % (C_, C_), C_, h, w)
    net = _f64_net(txt)
    rng = np.random.default_rng(11)
    net.params["c0"][0].data[...] = np.eye(C_, dtype=np.float32).reshape(C_, C_, 1, 1)
    net.params["c0"][1].data[...] = 0
    wt = rng.normal(0, 0.5, (C_, 1, 4, 4)).astype(np.float32)
    bs = rng.normal(0, 0.5, (C_,)).astype(np.float32)
    net.params["up"][0].data[...] = wt
    net.params["up"][1].data[...] = bs
    data = rng.normal(0, 1, (1, C_, h, w)).astype(np.float32)
    out = _forward(net, data)
    # out[c, 2 iy - 1 + a, 2 ix - 1 + b] += in[c, iy, ix] * w[c, 0, a, b] (col2im), on a canvas padded by one
    ref = np.zeros((C_, 2 * h + 2, 2 * w + 2))
    mag = np.zeros_like(ref)
    x = data[0].astype(np.float64)
    for a in range(4):
        for b in range(4):
            t = x * wt[:, 0, a, b].astype(np.float64)[:, None, None]
            ref[:, a:a + 2 * h:2, b:b + 2 * w:2] += t
            mag[:, a:a + 2 * h:2, b:b + 2 * w:2] += np.abs(t)
    ref = ref[:, 1:-1, 1:-1] + bs.astype(np.float64)[:, None, None]
    mag = mag[:, 1:-1, 1:-1]
    assert out["up"].shape == (1, C_, 2 * h, 2 * w)
    _assert_within_f64_bound(out["up"][0], ref, mag, 4, False, "deconv k4 s2 p1")   # (at most 2 x 2 taps reach an output)


def test_tail_predictors_per_element_bound():
    """Two 128-channel feature maps at 5x7 under three per-head predictor pairs (A = 3), read through the predictors' tops."""
    h, w = 5, 7
    txt = H.mini_detector(_conv_txt("f0", "data", 128, 1, 1, True) + _conv_txt("f1", "data", 128, 3, 1, True),
                          ["f0", "f1", "f0"], 8, 3, h, w)
    net = _f64_net(txt)
    rng = np.random.default_rng(5)
    for name, blobs in net.params.items():
        blobs[0].data[...] = rng.normal(0, 0.05 if "_" in name else 0.4, blobs[0].shape).astype(np.float32)
        blobs[1].data[...] = rng.normal(0, 0.3, blobs[1].shape).astype(np.float32)
    data = rng.normal(0, 1, (1, 3, h, w)).astype(np.float32)
    _forward(net, data, np.array([[8 * h, 8 * w, 1]], np.float32))
    feats = [np.array(net.blobs[n].data[0]) for n in ("f0", "f1", "f0")]
    for i, f in enumerate(feats):
        assert f.shape == (128, h, w) and (f > 0).any()
        for pname, nout in (("cls_score_%d" % i, 2), ("bbox_pred_%d" % i, 4)):
            wt = np.array(net.params[pname][0].data)
            bs = np.array(net.params[pname][1].data)
            ref, mag = _conv_ref(f, wt, bs, 1, np.float64)
            got = np.array(net.blobs[pname + "_output"].data)
            assert got.shape == (1, nout, h, w)
            _assert_within_f64_bound(got[0], ref, mag, 128, False, pname)


# ---- 4 - 6: the detector template with synthetic weights -------------------------------------------------------------------
def _detector_pair(**kw):
    old = os.environ.pop("SHF_CONV_MODE", None)
    try:
        return H.make_pair(H.detector_msg(True), **kw)
    finally:
        if old is not None:
            os.environ["SHF_CONV_MODE"] = old


@pytest.fixture(scope="module")
def detector():
    """(gpu net, oracle net) on the dilated-heads template, seeded synthetic weights; the net starts in fp32 mode."""
    return _detector_pair()


@pytest.fixture(scope="module")
def scoring_detector():
    """The same with the class bias tests/test_gpu_parity.py uses where detections must pass the 0.05 cut."""
    return _detector_pair(cls_bias=1.0)


def _unit(h, w, seed):
    return (H.synth_image_blob(h, w, seed=seed), h, w, h, w, 1.0, False)


def test_grouping_does_not_change_arithmetic(scoring_detector):
    import torch
    from smallhardface_amd import test as T
    gnet, _ = scoring_detector
    gnet.set_conv_mode("f64")
    thresh = 0.05
    units = [_unit(16, 16, 1), _unit(32, 48, 2), _unit(48, 32, 3)]
    fd = T.FusedDetector(gnet, n_lanes=3, mode="group")
    buf = torch.empty((40000, 5), dtype=torch.float32, device="cuda")
    # one grouped pass, every unit's rows in its member's own list
    fd.lanes[0].detect_add_levels(fd.lanes[:3], units, thresh, per_member_lists=True)
    fd.lanes[0].sync()
    grouped = []
    for m in range(3):
        n = fd.lanes[m].detect_export(buf.data_ptr(), buf.shape[0])
        grouped.append(buf[:n].cpu().numpy())
    for m, u in enumerate(units):
        # one single-unit pass
        gnet.detect_begin()
        gnet.detect_add_level(*u, thresh)
        n = gnet.detect_export(buf.data_ptr(), buf.shape[0])
        single = buf[:n].cpu().numpy()
        # Net.forward(): the proposal layer's outputs, cut like forward_net / detect() cut them (scale 1, no flip)
        out = _forward(gnet, u[0])
        keep = out["cls_prob"][:, 1] > thresh
        fwd = np.hstack([out["boxes"][keep, 1:5] / np.float32(1.0), out["cls_prob"][keep, 1:2]]).astype(np.float32)
        assert len(single) > 0
        np.testing.assert_array_equal(grouped[m], single)
        np.testing.assert_array_equal(single, fwd)
    # the merged detections of the image: grouped pass == unit by unit, in both merge methods
    old = cfg.TEST.NMS_METHOD
    try:
        for method in ("BBOX_VOTE", "NMS"):
            cfg.TEST.NMS_METHOD = method
            a = fd.detect(units, thresh=thresh)[0]
            b = T.detect_fused(gnet, units, thresh=thresh)[0]
            assert len(a) > 0
            np.testing.assert_array_equal(a, b)
    finally:
        cfg.TEST.NMS_METHOD = old
        gnet.set_conv_mode("fp32")


def test_whole_net_against_the_oracle(detector):
    """tests/test_gpu_parity.py test_detector_end_to_end, case (64, 80, im (61, 77)), with its bars, in f64 mode."""
    gnet, onet = detector
    gnet.set_conv_mode("f64")
    try:
        h, w, im = 64, 80, (61, 77)
        data = H.synth_image_blob(h, w, seed=4)
        info = np.array([[im[0], im[1], 0.75]], np.float32)
        go, oo = H.run_both(gnet, onet, data, info)
        for n in ["conv1_1", "conv1_2", "pool1", "conv2_2", "conv3_3", "conv4_3", "pool4", "conv5_3", "conv5_256",
                  "conv5_256_up", "conv4_256", "conv4_fuse", "conv4_fuse_final", "head_1", "head_2", "head_4"]:
            a, b = gnet.blobs[n].data, onet.blobs[n].data
            assert a.shape == b.shape, n
            print(n, H.rel_err(a, b))
            assert H.rel_err(a, b) < 5e-5, n
        gp = gnet.blobs["cls_prob_reshape_output"].data
        gd = gnet.blobs["bbox_pred_output"].data
        assert np.abs(gp - onet.blobs["cls_prob_reshape_output"].data).max() < SCORE_TOL
        assert np.abs(gd - onet.blobs["bbox_pred_output"].data).max() < 1e-3
        pb, pp = O.proposal_forward(gp, gd, info)
        gb, gs = go["boxes"], go["cls_prob"]
        assert gb.shape == pb.shape and gs.shape == pp.shape
        np.testing.assert_array_equal(gs, pp)
        assert np.abs(gb - pb).max() < BOX_TOL
        ob, os_ = oo["boxes"], oo["cls_prob"]
        n = min(len(ob), len(gb))
        assert abs(len(ob) - len(gb)) <= max(2, 0.01 * len(ob))
        assert np.abs(np.sort(gs[:, 1])[::-1][:n] - np.sort(os_[:, 1])[::-1][:n]).max() < SCORE_TOL
        for name in ["cls_score_1_output", "bbox_pred_4_output"]:
            a, b = gnet.blobs[name].data, onet.blobs[name].data
            assert a.shape == b.shape and np.abs(a - b).max() < 2e-4 * max(1.0, float(np.abs(b).max())), name
    finally:
        gnet.set_conv_mode("fp32")


def test_mode_cycle_leaves_the_other_modes_untouched(detector):
    gnet, _ = detector
    lane = gnet.clone()
    data = H.synth_image_blob(48, 64, seed=9)
    info = np.array([[48, 64, 1.0]], np.float32)

    def run(mode):
        gnet.set_conv_mode(mode)
        assert gnet.conv_mode == mode and lane.conv_mode == mode   # (shared by a net and its lanes)
        outs = []
        for net in (gnet, lane):
            o = _forward(net, data, info)
            outs.append((o["boxes"].copy(), o["cls_prob"].copy()))
        return outs

    def same(a, b):
        for (ab, ap), (bb, bp) in zip(a, b):
            np.testing.assert_array_equal(ab, bb)
            np.testing.assert_array_equal(ap, bp)

    try:
        before16 = run("f16x3")
        before32 = run("fp32")
        falls = gnet.range_fallbacks
        gnet.set_layer_products({"conv3_3": 1})     # no effect in f64 mode
        first64 = run("f64")
        gnet.set_layer_products({"conv3_3": 0})
        c33 = np.array(gnet.blobs["conv3_3"].data)   # an intermediate blob is readable after an f64 forward
        assert gnet.range_fallbacks == falls
        after16 = run("f16x3")
        second64 = run("f64")
        assert gnet.range_fallbacks == falls
        after32 = run("fp32")
        c33_32 = np.array(gnet.blobs["conv3_3"].data)
        same(before32, after32)
        same(before16, after16)
        same(first64, second64)
        same(first64[:1], first64[1:])               # the lane computes what the net computes
        assert len(first64[0][0]) > 0
        assert c33.shape == c33_32.shape and np.isfinite(c33).all() and c33.max() > 0
        assert H.rel_err(c33, c33_32) < 5e-5
    finally:
        gnet.set_conv_mode("fp32")


def test_env_starts_a_fresh_process_in_f64_mode():
    code = ("from smallhardface_amd import caffe\n"
            "from tests import helpers as H\n"
            "net = caffe.Net(None, prototxt_text=H.single_layer_net('layer { name: \"c1\" type: \"Convolution\" bottom: "
            "\"data\" top: \"c1\" convolution_param { num_output: 16 kernel_size: 3 pad: 1 } }\\n', 3, 5, 7))\n"
            "print('MODE', net.conv_mode)\n")
    env = dict(os.environ, SHF_CONV_MODE="5")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "MODE f64" in r.stdout
