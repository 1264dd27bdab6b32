"""BatchNorm and Scale as far as a machine without a GPU can see them: the fp32 references of tests/norm_cases.py against a
binary64 evaluation, the oracle net's walk over the ResNet-style graph, the fold's binary64 statement against the layers one
after the other -- for the very seeds the GPU tests use --, and the channel-affine kernels (csrc/norm.hip) compiled for
gfx950 with the build recipe's flags: no private segment, no spilled register, no LDS."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd import weights as W
from tests import fusion_cases as F
from tests import helpers as H
from tests import norm_cases as N

F32 = np.float32
U32 = 2.0 ** -24        # unit roundoff of fp32
ACT_TOL = 2e-5          # tests/test_gpu_parity.py


def _x(C=12, h=5, w=7, seed=0):
    return np.random.default_rng(seed).normal(0.3, 2.0, (2, C, h, w)).astype(F32)


def test_batch_norm_literal_and_operation_order():
    x = np.array([1.0, -2.0, 0.1, 7.0], F32).reshape(1, 2, 1, 2)
    blobs = [np.array([3.0, -1.5], F32), np.array([12.0, 0.75], F32), np.array([3.0], F32)]
    sf = F32(1) / F32(3)
    m = np.array([F32(3) * sf, F32(-1.5) * sf], F32)
    d = np.sqrt(np.array([F32(12) * sf + F32(1e-5), F32(0.75) * sf + F32(1e-5)], F32))
    want = np.array([(F32(1) - m[0]) / d[0], (F32(-2) - m[0]) / d[0], (F32(0.1) - m[1]) / d[1], (F32(7) - m[1]) / d[1]], F32)
    got = N.batch_norm(x, blobs)
    assert got.dtype == F32
    np.testing.assert_array_equal(got.reshape(-1), want)
    # blob2 == 0: the statistics were never accumulated -- sf = 0, y = x / sqrt(eps)
    blobs[2][0] = 0
    np.testing.assert_array_equal(N.batch_norm(x, blobs, 0.25), (x / F32(0.5)).astype(F32))
    # the product with 1 / blob2 is NOT a division by blob2
    b3 = [np.array([1.0], F32), np.array([1.0], F32), np.array([999.98], F32)]
    assert N.bn_vectors(b3)[0][0] == F32(1) * (F32(1) / F32(999.98))


def test_scale_literal_rounds_twice():
    x = np.array([0.1, -3.0, 2.0 ** 24, 5.0], F32).reshape(1, 2, 2, 1)
    g, b = np.array([0.3, -2.0], F32), np.array([1.0, 0.5], F32)
    want = np.array([F32(F32(0.1) * F32(0.3)) + F32(1), F32(F32(-3) * F32(0.3)) + F32(1), F32(-2.0 ** 25) + F32(0.5), F32(-10) + F32(0.5)], F32)
    np.testing.assert_array_equal(N.scale(x, g, b).reshape(-1), want)
    np.testing.assert_array_equal(N.scale(x, g).reshape(-1), np.array([F32(0.1) * F32(0.3), F32(-3) * F32(0.3), -2.0 ** 25, -10], F32))
    assert np.signbit(N.scale(np.array([[[[-0.0]]]], F32), [1.0])[0, 0, 0, 0])          # no bias_term: no add, -0 stays -0


@pytest.mark.parametrize("factor", [N.FACTOR, 1.0, 0.0])
def test_references_against_binary64_within_three_roundings(factor):
    """Every fp32 reference against the same step evaluated in binary64, within 3 roundings (3 * 2^-24, relative).  The
    per-channel vectors: m = blob0 * sf carries the rounding of sf and of the product (2); d = sqrt(blob1 * sf + eps) those
    of sf, the product and the add, halved by the root, and the root's own (2.5).  Per element, on the fp32 vectors the layer
    itself uses: BatchNorm is a subtraction and a division (2), Scale a product and an add (2, the add's relative to the larger
    of its operands)."""
    x = _x()
    rng = np.random.default_rng(3)
    bn = N.norm_blobs("BatchNorm", x, rng, factor=factor)
    sc = N.norm_blobs("Scale", x, rng)
    m, d = N.bn_vectors(bn)
    m64, d64 = N.bn_vectors64(bn)
    assert (np.abs(m - m64) <= 3 * U32 * np.abs(m64)).all() and (np.abs(d - d64) <= 3 * U32 * d64).all()
    got = N.batch_norm(x, bn)
    ref = (x.astype(np.float64) - m.astype(np.float64).reshape(1, -1, 1, 1)) / d.astype(np.float64).reshape(1, -1, 1, 1)
    err = np.abs(got.astype(np.float64) - ref)
    print("batch_norm: worst err / (2^-24 |ref|) %.3f" % float((err / (U32 * np.abs(ref) + 1e-300)).max()))
    assert (err <= 3 * U32 * np.abs(ref)).all()
    prod = got.astype(np.float64) * sc[0].astype(np.float64).reshape(1, -1, 1, 1)
    ref2 = prod + sc[1].astype(np.float64).reshape(1, -1, 1, 1)
    err2 = np.abs(N.scale(got, sc[0], sc[1]).astype(np.float64) - ref2)
    assert (err2 <= 3 * U32 * np.maximum(np.abs(prod), np.abs(ref2))).all()
    assert (np.abs(N.scale(got, sc[0]).astype(np.float64) - prod) <= U32 * np.abs(prod)).all()
    # the chain in binary64, rounded once, is within one rounding of the binary64 value
    c64 = N.chain64(x, bn, sc)
    r64 = N.chain64(x, bn, sc, rounded=False)
    assert (np.abs(c64 - r64) <= U32 * np.abs(r64) + 1e-45).all()
    assert (sc[0] < 0).any() and (sc[0] > 0).any() and (sc[1] < 0).any() and (sc[1] > 0).any()


def test_parameter_synthesiser_is_trained_like():
    msg = N.resblock(32, 48)
    data = H.synth_image_blob(32, 48, seed=4)
    params = N.synth_norm_params(msg, data, seed=22)
    assert [b.shape for b in params["bn_conv1"]] == [(64,), (64,), (1,)] and params["bn_conv1"][2][0] == F32(N.FACTOR)
    assert [b.shape for b in params["scale_res2a_branch2c"]] == [(256,), (256,)] and len(params["res2a_branch1"]) == 1
    assert len(params["conv1"]) == 2 and "bn_pre" in params and "res2a_relu" not in params
    ch = W.infer_channels(msg)
    assert ch["res2a"] == 256 and ch[N.RES_PROBE] == 128
    net = N.NormOracleNet(msg, params=params)
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    net.forward(data=data, im_info=np.array([[32, 48, 1]], F32))
    y = net.snapshots[("bn_conv1", "conv1")]
    # normalised by its own statistics: per-channel mean within the spread, deviation near 1
    assert np.abs(y.mean(axis=(0, 2, 3))).max() < 1.5 and 0.6 < y.std(axis=(0, 2, 3)).min() and y.std(axis=(0, 2, 3)).max() < 1.6
    with pytest.raises(NotImplementedError):          # why the oracle net lives in tests/norm_cases.py
        F.FusionOracleNet(msg, params=params).forward()


def test_the_oracle_net_walks_the_resblock():
    msg = N.resblock(32, 48)
    data, info = H.synth_image_blob(32, 48, seed=4), np.array([[32, 48, 1]], F32)
    params = N.synth_norm_params(msg, data, info, seed=22)
    net = N.NormOracleNet(msg, params=params)
    net.blobs["data"].reshape(*data.shape)
    net.blobs["im_info"].reshape(1, 3)
    out = net.forward(data=data, im_info=info)
    s, b = net.snapshots, {k: v.data for k, v in net.blobs.items()}
    assert b["conv1"].shape == (1, 64, 16, 24) and b["pool1"].shape == (1, 64, 8, 12) and b["res2a"].shape == (1, 256, 8, 12)
    assert sorted(out) == ["boxes", "cls_prob"] and out["boxes"].shape[1] == 5
    # an in-place layer replaces its blob: each snapshot is its layer applied to the one before
    conv = O.convolution(data, params["conv1"][0], params["conv1"][1], pad=3, stride=2)
    np.testing.assert_array_equal(s[("conv1", "conv1")], conv)
    np.testing.assert_array_equal(s[("bn_conv1", "conv1")], N.batch_norm(conv, params["bn_conv1"]))
    np.testing.assert_array_equal(s[("scale_conv1", "conv1")], N.scale(s[("bn_conv1", "conv1")], *params["scale_conv1"]))
    np.testing.assert_array_equal(b["conv1"], F.relu(s[("scale_conv1", "conv1")]))
    summed = F.eltwise([b["res2a_branch1"], b["res2a_branch2c"]])
    np.testing.assert_array_equal(s[("res2a", "res2a")], summed)
    np.testing.assert_array_equal(b["res2a"], N.chain32(F.relu(summed), params["bn_pre"], params["scale_pre"], slope=0.0))
    assert (s[("scale_pre", "res2a")] < 0).any() and (b["res2a"] >= 0).all() and (b["res2a_branch2c"] < 0).any()


@pytest.mark.parametrize("case", sorted(N.FOLD_CASES))
def test_fold_against_the_layers_one_after_the_other(case):
    """Net B (the bare convolution with ``norm_cases.fold`` of A's blobs) against net A layer by layer, both on the oracle, for
    every variant and seed of the GPU tests.  The two differ by the roundings of W_eff / b_eff against those of the separate
    layers.  Measured rel_err (helpers.rel_err on the ReLU's top), worst variant per case: c1x1 6.8e-7, c3x3 6.6e-7,
    first3 3.7e-7, stem7 8.0e-7; whole resblock, every blob: 1.8e-6 -- all under ACT_TOL / 2 = 1e-5, so the device keeps the
    other half."""
    worst = 0.0
    for bias, bn, sc in N.FOLD_VARIANTS:
        msg_a, pa, msg_b, pb, data = N.fold_pair(case, bias, bn, sc)
        outs = []
        for msg, params in ((msg_a, pa), (msg_b, pb)):
            net = N.NormOracleNet(msg, params=params)
            net.blobs["data"].reshape(*data.shape)
            net.blobs["im_info"].reshape(1, 3)
            outs.append(net.forward(data=data, im_info=np.array([[data.shape[2], data.shape[3], 1]], F32))["c"])
        assert outs[0].shape == outs[1].shape and (outs[0] > 0).any() and (outs[0] == 0).any()
        err = H.rel_err(outs[1], outs[0])
        print("%s bias %d bn %d sc %d: rel_err %.3g" % (case, bias, bn, sc, err))
        worst = max(worst, err)
    assert worst < ACT_TOL / 2, worst


def test_fold_on_the_resblock_for_the_gpu_tests_seed():
    """The whole graph of test 8 (parameter seed 22, image seed 4) with every foldable convolution replaced by its folded
    twin: every named blob within ACT_TOL / 2 of the layer-by-layer walk."""
    msg = N.resblock(64, 96)
    data, info = H.synth_image_blob(64, 96, seed=4), np.array([[61, 93, 0.75]], F32)
    params = N.synth_norm_params(msg, data, info, seed=22)
    a = N.NormOracleNet(msg, params=params)
    folded = dict(params)
    for c in N.RES_FOLDED:
        w, b = N.fold(params[c][0], params[c][1] if len(params[c]) > 1 else None, params["bn_" + c], params["scale_" + c])
        folded[c] = [w, b]
        folded["bn_" + c] = [np.zeros_like(params["bn_" + c][0]), np.ones_like(params["bn_" + c][1]) - F32(N.EPS), np.ones(1, F32)]
        folded["scale_" + c] = [np.ones_like(params["scale_" + c][0]), np.zeros_like(params["scale_" + c][1])]
    txt = N.resblock_text(64, 96).replace(" bias_term: false", "")
    b = N.NormOracleNet(P.parse(txt), params=folded)
    worst = 0.0
    for net in (a, b):
        net.blobs["data"].reshape(*data.shape)
        net.blobs["im_info"].reshape(1, 3)
        net.forward(data=data, im_info=info)
    for name in N.RES_BLOBS:
        worst = max(worst, H.rel_err(b.blobs[name].data, a.blobs[name].data))
    print("resblock folded against layered: worst rel_err %.3g" % worst)
    assert worst < ACT_TOL / 2, worst


def test_the_channel_affine_kernels_build_for_gfx950_without_scratch_spills_or_lds(tmp_path):
    """norm.hip compiled for the device with the build recipe's own flags, and the compiler's resource-usage remarks read:
    the vector and the scalar form, each in fp32 and in binary64."""
    from smallhardface_amd import build as B
    extra = dict(B.SOURCES)["norm.hip"]
    assert "-ffp-contract=off" in extra                              # the product and the add of a Scale round separately
    cmd = [B.HIPCC, "--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           os.path.join(B.CSRC, "norm.hip"), "-o", str(tmp_path / "norm.o"),
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
    assert len(kernels) == 4 and all("channel_affine_kernel" in k for k in kernels), sorted(kernels)
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] == 0, (name, k)
        # in flight per thread: four rows x one quad of activations (16 registers) and four per-channel quads (16; in binary64
        # mean and denominator are 8 registers each: 24), the rest addresses and the division's temporaries (binary64: pairs).
        # Twice the loads in flight is the budget: 64 registers in fp32 (eight waves per SIMD), 96 in binary64 (five).
        f64 = "Lb1EEEv" in name
        assert 0 < k["VGPRs"] <= (96 if f64 else 64), (name, k)
