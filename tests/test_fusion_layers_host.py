"""Eltwise, Crop and the free-standing ReLU as far as a machine without a GPU can see them: the numpy references of
tests/fusion_cases.py against hand-written literals, the parameter generator on a graph that holds the new layers, the
oracle net's walk over that graph, and the combine kernels (csrc/eltwise.hip) compiled for gfx950 with the build recipe's
flags -- no private segment, no spilled register, no LDS."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from smallhardface_amd import weights as W
from tests import fusion_cases as F

F32 = np.float32


def _a(*rows):
    return np.array(rows, F32).reshape(1, 2, 2, 3)


# two 1 x 2 x 2 x 3 bottoms with mixed signs, a tie (element 4) and values that do not survive a fused multiply-add unchanged
A = _a([1, -2, 3], [0.5, 4, -6], [7, 8, -9], [10, 0.1, 12])
B = _a([4, 5, -6], [0.25, 4, 2], [-7, 3, 9], [1, 0.3, -12])


def test_eltwise_sum_with_coefficients_literal():
    got = F.eltwise([A, B], "SUM", [2, -1])
    want = _a([-2, -9, 12], [0.75, 4, -14], [21, 13, -27], [19, None, 36])
    # 2 * 0.1f - 0.3f in fp32, each step rounded: not the real number -0.1
    want[0, 1, 1, 1] = F32(F32(0) + F32(2) * F32(0.1)) + F32(-1) * F32(0.3)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == F32
    # coeff absent = all ones; the order of the bottoms is the order of the adds
    np.testing.assert_array_equal(F.eltwise([A, B]), (A + B).astype(F32))
    big = [np.full((1, 1, 1, 1), v, F32) for v in (2.0 ** 24, 1.0, 1.0, -2.0 ** 24)]
    assert F.eltwise(big)[0, 0, 0, 0] == 0.0                          # (2^24 + 1) + 1 = 2^24 in fp32 ...
    assert F.eltwise(big[::-1])[0, 0, 0, 0] == 2.0                    # ... while -2^24 + 1 + 1 is exact
    assert F.eltwise([big[1], big[2], big[0], big[3]])[0, 0, 0, 0] == 2.0


def test_eltwise_prod_and_max_literal():
    np.testing.assert_array_equal(F.eltwise([A, B], "PROD"),
                                  _a([4, -10, -18], [0.125, 16, -12], [-49, 24, -81], [10, F32(0.1) * F32(0.3), -144]))
    np.testing.assert_array_equal(F.eltwise([A, B], "MAX"), _a([4, 5, 3], [0.5, 4, 2], [7, 8, 9], [10, 0.3, 12]))
    np.testing.assert_array_equal(F.eltwise([A, B, -A], "MAX"), _a([4, 5, 3], [0.5, 4, 6], [7, 8, 9], [10, 0.3, 12]))
    np.testing.assert_array_equal(F.eltwise([A, B, A], "PROD"), ((A * B).astype(F32) * A).astype(F32))
    with pytest.raises(AssertionError):
        F.eltwise([A, B], "MAX", [1, 1])
    with pytest.raises(AssertionError):
        F.eltwise([A, B], "SUM", [1])


X = np.arange(1 * 4 * 3 * 4, dtype=F32).reshape(1, 4, 3, 4)       # value = 12 c + 4 y + x


@pytest.mark.parametrize("axis,offset,ref_shape,want", [
    (2, (), (1, 9, 2, 3), X[:, :, 0:2, 0:3]),                   # no offset: the corner
    (2, (1,), (1, 9, 2, 3), X[:, :, 1:3, 1:4]),                 # one offset for both axes
    (2, (1, 0), (1, 9, 2, 4), X[:, :, 1:3, 0:4]),               # one per cropped axis
    (3, (2,), (9, 9, 9, 2), X[:, :, :, 2:4]),                   # the last axis only: the rest of the reference's shape is ignored
    (1, (1, 0, 1), (1, 2, 3, 3), X[:, 1:3, :, 1:4]),            # channels too
    (1, (2,), (1, 2, 1, 2), X[:, 2:4, 2:3, 2:4]),
])
def test_crop_literal(axis, offset, ref_shape, want):
    got = F.crop(X, ref_shape, axis, offset)
    np.testing.assert_array_equal(got, want)
    assert got.flags["C_CONTIGUOUS"] and got.dtype == F32
    if axis == 2 and offset == (1,):
        assert got[0, 0].tolist() == [[5, 6, 7], [9, 10, 11]] and got[0, 3, 1, 2] == 47


def test_crop_refuses_what_does_not_fit():
    with pytest.raises(AssertionError):
        F.crop(X, (1, 4, 3, 4), 2, (1,))
    with pytest.raises(AssertionError):
        F.crop(X, (1, 4, 2, 2), 2, (1, 1, 1))


def test_relu_literal():
    x = np.array([-2.0, -0.0, 0.0, 3.0, -0.3], F32)
    np.testing.assert_array_equal(F.relu(x), np.array([0, 0, 0, 3, 0], F32))
    np.testing.assert_array_equal(F.relu(x, 0.1), np.array([F32(0.1) * F32(-2), 0, 0, 3, F32(0.1) * F32(-0.3)], F32))
    np.testing.assert_array_equal(F.relu(x), O.relu(x))
    assert np.isnan(F.relu(np.array([np.nan], F32))[0])


def test_parameters_and_channels_on_the_m1_shaped_graph():
    msg = F.m1_shaped(64, 96)
    ch = W.infer_channels(msg)
    assert ch["conv5_128_up"] == ch["conv5_128_crop"] == ch["conv4_fuse"] == 128 and ch["m1_out"] == 256
    params = W.synth_params(msg, seed=3, cls_bias=1.0)
    assert params["conv4_fuse_final"][0].shape == (128, 128, 3, 3) and params["m1_3x3"][0].shape == (128, 128, 3, 3)
    assert params["cls_score_m1"][0].shape == (4, 256, 1, 1) and params["bbox_pred_m1"][0].shape == (8, 256, 1, 1)
    assert params["conv5_128_up"][0].shape == (128, 1, 4, 4) and len(params["conv5_128_up"]) == 1
    assert not set(params) & {"conv5_128_crop", "conv4_fuse", "m1_out", "m1_out_relu"}
    types = [str(L.get("type")) for L in msg.getall("layer")]
    assert types.count("Eltwise") == 1 and types.count("Crop") == 1 and types.count("Deconvolution") == 1
    with pytest.raises(NotImplementedError):          # why the references live in tests/fusion_cases.py
        O.OracleNet(msg, params=params).forward()


def test_the_oracle_net_walks_the_new_layers():
    """A small graph: the blobs are what the references give on the net's own bottoms, a Concat's members keep their values
    when an in-place ReLU rewrites the top, and a non-in-place ReLU leaves its bottom alone."""
    from tests import helpers as H
    txt = H.single_layer_net(
        F.conv_layer("a", "data", 8, 1) + F.pool_layer("p", "a") + F.conv_layer("b", "p", 8, 1) + F.deconv_layer("up", "b", 8) +
        F.crop_layer("upc", "up", "a", axis=2, offset=(1, 0)) + F.eltwise_layer("s", ["a", "upc"], coeff=[0.5, -2]) +
        F.relu_layer("s_relu", "s", slope=0.25) + F.relu_layer("r", "a", top="r") + F.concat_layer("cc", ["r", "s"]) +
        F.relu_layer("cc_relu", "cc"), 4, 5, 7)
    msg = P.parse(txt)
    net = F.FusionOracleNet(msg, params=W.synth_params(msg, seed=5))
    x = np.random.default_rng(0).normal(0, 1, (1, 4, 5, 7)).astype(F32)
    net.forward(data=x, im_info=np.array([[5, 7, 1]], F32))
    b = {k: v.data for k, v in net.blobs.items()}
    assert b["up"].shape == (1, 8, 6, 8) and b["upc"].shape == b["a"].shape == (1, 8, 5, 7)
    np.testing.assert_array_equal(b["upc"], b["up"][:, :, 1:6, 0:7])
    pre = net.snapshots[("s", "s")]
    np.testing.assert_array_equal(pre, F.eltwise([b["a"], b["upc"]], "SUM", [0.5, -2]))
    np.testing.assert_array_equal(b["s"], F.relu(pre, 0.25))
    assert (pre < 0).any() and (b["a"] < 0).any()
    np.testing.assert_array_equal(b["r"], F.relu(b["a"]))
    np.testing.assert_array_equal(b["cc"], F.relu(np.concatenate([b["r"], b["s"]], axis=1)))
    assert (b["s"] < 0).any() and (b["cc"] >= 0).all()               # the member kept its negative values


def test_the_combine_kernels_build_for_gfx950_without_scratch_spills_or_lds(tmp_path):
    """eltwise.hip compiled for the device with the build recipe's own flags, and the compiler's resource-usage remarks read:
    the vector and the scalar form, each with fp32 and with binary64 accumulation."""
    from smallhardface_amd import build as B
    extra = dict(B.SOURCES)["eltwise.hip"]
    assert "-ffp-contract=off" in extra                              # coeff * x and the add round separately
    cmd = [B.HIPCC, "--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           os.path.join(B.CSRC, "eltwise.hip"), "-o", str(tmp_path / "eltwise.o"),
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
    assert len(kernels) == 4 and all("combine_group_kernel" in k for k in kernels), sorted(kernels)
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] == 0, (name, k)
        # four rows x four inputs x one quad of loads in flight are 64 registers: five waves per SIMD or more
        assert 0 < k["VGPRs"] <= 96, (name, k)
