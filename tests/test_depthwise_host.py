"""The references and graphs of tests/depthwise_cases.py on their own (no GPU): what tests/test_gpu_depthwise.py holds the
depthwise kernel (csrc/conv_dw.hip) to.

1. The three references of a layer case agree: `O.convolution(group=Cin)`, the dense block-diagonal `O.convolution` and the
   binary64 tap loop -- exactly on integer grids, to 5e-7 (relative to the largest value) on normal ones.
2. Output sizes, the dense-twin selection and the graph texts parse; the MobileNet-shaped graph has the shapes it claims.
3. What keeps the end-to-end test honest, pinned by the chosen seed: the oracle with folded parameters stays within
   ACT_TOL / 4 of the unfolded oracle on every blob of `mbnet_mini`; on each of the three units no foreground score lies
   within 2 SCORE_TOL of the threshold, no box side within 0.01 px (ten BOX_TOL) of the min-size cut, no two rows tie.
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import depthwise_cases as D
from tests import general_conv_cases as G
from tests import helpers as H
from tests import modules_cases as MC

ACT_TOL = 2e-5
SCORE_TOL = 1e-4
BOX_TOL = 1e-3


@pytest.mark.parametrize("case", D.LAYER_CASES, ids=D.case_id)
def test_the_three_references_agree(case):
    cin, m, k, s, p, d, h, w = case
    for bias in (True, False):
        data, wt, bs = D.int_inputs(case, bias)
        _, perm = D.g_params(case, wt, bs)
        x = data[:, perm]
        grouped = D.oracle_layer(case, x, wt, bs, False)
        dense = O.convolution(x, D.dense_weights(wt, cin, m), bs, pad=p, stride=s, dil=d).astype(np.float64)
        naive, mag = D.naive_depthwise(x[0], wt, bs, s, p, d, m)
        assert grouped.shape == (1, cin * m) + D.out_size(case)
        np.testing.assert_array_equal(grouped, dense)
        np.testing.assert_array_equal(grouped[0], naive)
        assert np.abs(grouped).max() <= k * k * 8 + 8 and (grouped < 0).any()
        data, wt, bs = D.random_inputs(case, bias)
        x = data[:, perm]
        grouped = D.oracle_layer(case, x, wt, bs, False)
        dense = O.convolution(x, D.dense_weights(wt, cin, m), bs, pad=p, stride=s, dil=d).astype(np.float64)
        naive, mag = D.naive_depthwise(x[0], wt, bs, s, p, d, m)
        assert H.rel_err(grouped, dense) < 5e-7 and H.rel_err(grouped[0], naive) < 5e-7
        assert (mag >= np.abs(naive - (0 if bs is None else bs.astype(np.float64)[:, None, None])) - 1e-12).all()


def test_cases_and_texts():
    assert len(D.LAYER_CASES) == 20 and len(set(D.LAYER_CASES)) == 20
    for case in D.LAYER_CASES:
        ho, wo = D.out_size(case)
        assert ho >= 1 and wo >= 1, case
        for bias, relu in D.VARIANTS:
            msg = P.parse(D.layer_net_text(case, bias, relu, dense_twin=True))
            g = [L for L in msg.getall("layer") if str(L.get("name")) == "g"][0]
            cp = g.get("convolution_param")
            assert int(cp.get("group")) == case[0] and int(cp.get("num_output")) == D.cout(case)
    assert D.out_size((32, 1, 3, 2, 1, 1, 8, 10)) == (4, 5) and D.out_size((8, 1, 3, 3, 0, 1, 10, 10)) == (3, 3)
    assert D.out_size((8, 1, 2, 2, 0, 1, 6, 7)) == (3, 3) and D.out_size((8, 1, 3, 1, 1, 2, 7, 7)) == (5, 5)
    # the dense twins that run the general-geometry kernel: strided, 5x5 / 7x7, pad != dilation, valid, even kernels
    assert (32, 1, 3, 2, 1, 1, 9, 11) in D.DENSE_TWIN_CASES and (32, 1, 3, 1, 1, 1, 9, 11) not in D.DENSE_TWIN_CASES
    assert (8, 1, 3, 1, 2, 2, 7, 7) not in D.DENSE_TWIN_CASES and (16, 1, 1, 1, 0, 1, 4, 5) not in D.DENSE_TWIN_CASES
    assert all(c[0] <= 64 for c in D.DENSE_TWIN_CASES) and len(D.DENSE_TWIN_CASES) == 12
    w = D.dense_weights(np.arange(6 * 9, dtype=np.float32).reshape(6, 1, 3, 3), 2, 3)
    assert w.shape == (6, 2, 3, 3) and (w[:3, 1] == 0).all() and (w[3:, 0] == 0).all() and (w[4, 1] == np.arange(36, 45).reshape(3, 3)).all()
    for C in (12, 6):
        assert "group: %d" % C in D.concat_net_text(C)
        P.parse(D.concat_net_text(C))
    P.parse(D.neighbours_text(13, 19))
    for C in (32, 5):
        msg_a, pa, msg_b, pb, data = D.fold_pair(C, False, True)
        assert len(pa["g"]) == 1 and len(pb["g"]) == 2 and pb["g"][0].shape == (C, 1, 3, 3) and "g_bn" in pa and "g_sc" in pa


def test_mbnet_shapes():
    data, info = D.mbnet_unit(*D.MB_SIZE)
    onet = D.forwarded(D.mbnet_oracle(), data, info)
    for name, hw in D.mbnet_map_sizes(*D.MB_SIZE).items():
        assert onet.blobs[name].data.shape[2:] == hw, name
    assert onet.blobs["f8"].data.shape == (1, 128, 8, 12) and onet.blobs["f16"].data.shape == (1, 128, 4, 6)
    p = D.mbnet_params()
    for name in D.MB_DW_LAYERS:
        assert p[name][0].shape[1] == 1 and len(p[name]) == 1 and len(p["bn_" + name]) == 3 and len(p["scale_" + name]) == 2
    assert MC.levels_of(onet) == ["8", "16"]


def test_mbnet_tolerance_room_and_margins():
    for j, (h, w) in enumerate(D.MB_GROUP_SIZES):
        data, info = D.mbnet_unit(h, w)
        onet = D.forwarded(D.mbnet_oracle(h, w), data, info)
        if j == 0:
            bnet = D.forwarded(D.mbnet_oracle(h, w, bare=True), data, info)
            for name in D.MB_BLOBS:
                e = H.rel_err(bnet.blobs[name].data, onet.blobs[name].data)
                assert e < ACT_TOL / 4, (name, e)
        for m, (d_score, d_side, ties) in MC.oracle_margins(onet, info, D.MB_MODULES, D.MB_MIN_SIZE, D.MB_THRESH).items():
            rows = len(onet.blobs["cls_prob_" + m].data)
            print("unit %d module %s: %d rows, score margin %.3g, side margin %.3g" % (j, m, rows, d_score, d_side))
            assert d_score > 2 * SCORE_TOL and d_side > 10 * BOX_TOL and not ties and rows > 1, (j, m, d_score, d_side, ties, rows)


def test_the_depthwise_kernels_build_for_gfx950_without_scratch_spills_or_lds(tmp_path):
    """conv_dw.hip compiled for the device with the build recipe's own flags, and the compiler's resource-usage remarks read:
    vector and scalar form x fp32 and binary64 x the generic, the 3x3 stride-1 and the 3x3 stride-2 form."""
    import os
    import re
    import subprocess
    from smallhardface_amd import build as B
    extra = dict(B.SOURCES)["conv_dw.hip"]
    assert "-ffp-contract=off" in extra                              # the chain is compiled as written
    cmd = [B.HIPCC, "--offload-arch=" + B.ARCH, "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
           os.path.join(B.CSRC, "conv_dw.hip"), "-o", str(tmp_path / "conv_dw.o"),
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
    assert len(kernels) == 12 and all("conv_dw_kernel" in k for k in kernels), sorted(kernels)
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0 and k["LDS Size"] == 0, (name, k)
        # the widest form holds a strip's input in registers: 9 rows x 3 columns x one quad (108), nine weight quads (36) and
        # the accumulators (16; binary64: 32) -- every form stays inside the 256 a block of 256 threads may use
        assert 0 < k["VGPRs"] <= 256, (name, k)
