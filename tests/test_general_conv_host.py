"""The references of the general-geometry convolution tests, on the CPU (no GPU needed; the device side:
tests/test_gpu_general_conv.py).  Cases and graphs: tests/general_conv_cases.py.

1. On the integer grids `O.convolution` equals a naive loop over the taps exactly and every sum of magnitudes stays below
   2^24: the reference alone satisfies the equality the device test asserts.
2. On the random grids `O.convolution` (fp32 BLAS) lies within ACT_TOL of the same loop in float64: the reference alone
   satisfies the bound the device test asserts.
3. The feeder layers hand the grid on unchanged: the oracle net's input of `g` is the selected channels of `data`, bit for bit.
4. The S3FD-shaped graph: map sizes, output names, and -- for each of the group's three input sizes -- no anchor score of the
   oracle within 2 SCORE_TOL of the score threshold and no two rows tied (what the end-to-end comparison of row sets hinges on).
"""
import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import general_conv_cases as G
from tests import modules_cases as MC

ACT_TOL = 2e-5          # tests/test_gpu_parity.py
SCORE_TOL = 1e-4


def rel_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(1e-12, np.abs(b).max()))


@pytest.mark.parametrize("case_first", G.ALL_CASES, ids=G.case_id)
def test_integer_reference_is_exact(case_first):
    case, first = case_first
    cin, cout, k, s, p, d, h, w = case
    for bias, relu in G.VARIANTS:
        data, wt, bs = G.int_inputs(case, first, bias)
        _, perm = G.feeder_params(cin, first)
        x = data[:, perm]
        ref, mag = G.naive_conv(x[0].astype(np.int64), wt.astype(np.int64), None if bs is None else bs.astype(np.int64), s, p, d, np.int64)
        assert int(mag.max()) + 8 < 2 ** 24
        assert ref.shape == (cout,) + G.out_size(case)
        if relu:
            ref = np.maximum(ref, 0)
        else:
            assert (ref < 0).any()
        np.testing.assert_array_equal(G.oracle_layer(case, x, wt, bs, relu)[0], ref.astype(np.float64))


@pytest.mark.parametrize("case_first", G.ALL_CASES, ids=G.case_id)
def test_random_reference_within_the_bound(case_first):
    case, first = case_first
    cin, cout, k, s, p, d, h, w = case
    data, wt, bs = G.random_inputs(case, first, True)
    _, perm = G.feeder_params(cin, first)
    x = data[:, perm]
    ref, _ = G.naive_conv(x[0], wt, bs, s, p, d, np.float64)
    e = rel_err(G.oracle_layer(case, x, wt, bs, False)[0], ref)
    print("%s: oracle vs float64 %.3g" % (G.case_id(case_first), e))
    assert e < ACT_TOL / 10


@pytest.mark.parametrize("case_first", [cf for cf in G.ALL_CASES if cf[0][0] in (5, 40, 32, 3)][:5], ids=G.case_id)
def test_feeders_hand_the_grid_on_unchanged(case_first):
    case, first = case_first
    data, wt, bs = G.int_inputs(case, first, True)
    params, perm = G.g_params(case, first, wt, bs)
    msg = P.parse(G.layer_net_text(case, first, True, False))
    onet = O.OracleNet(msg, params=params)
    out = onet.forward(data=data, im_info=np.zeros((1, 3), np.float32))
    bottom = G.feeder_txt(case[0], first)[1]
    np.testing.assert_array_equal(onet.blobs[bottom].data, data[:, perm])
    np.testing.assert_array_equal(out["g"].astype(np.float64), G.oracle_layer(case, data[:, perm], wt, bs, False))
    if bottom == "sel":
        assert sorted(np.unique(params["sel"][0]).tolist()) == [0.0, 1.0] and (params["sel"][0].sum(axis=(1, 2, 3)) == 1).all()
        assert len(set(perm.tolist())) == case[0] and not np.array_equal(perm, np.arange(case[0]))


@pytest.mark.parametrize("size", G.S3FD_GROUP_SIZES, ids=lambda s: "%dx%d" % s)
def test_s3fd_oracle_rows_do_not_hinge_on_the_last_digits(size):
    h, w = size
    onet = G.s3fd_oracle(h, w)
    data, info = G.s3fd_unit(h, w)
    onet.blobs["data"].reshape(*data.shape)
    onet.blobs["im_info"].reshape(1, 3)
    out = onet.forward(data=data, im_info=info)
    assert sorted(out.keys()) == sorted("%s_%s" % (k, m) for m in G.S3FD_MODULES for k in ("boxes", "cls_prob"))
    for name, hw in G.s3fd_map_sizes(h, w).items():
        assert onet.blobs[name].data.shape[2:] == hw, name
    for m, (d_score, _, ties) in MC.oracle_margins(onet, info, G.S3FD_MODULES, G.S3FD_MIN_SIZE, G.S3FD_THRESH).items():
        print("%dx%d module %s: nearest score %.3g from the threshold, %d rows" % (h, w, m, d_score, len(out["cls_prob_" + m])))
        assert d_score > 2 * SCORE_TOL and not ties, (m, d_score, ties)
        assert len(out["cls_prob_" + m]) > 1, m
