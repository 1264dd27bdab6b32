"""The references and graphs of tests/pooling_cases.py on their own (no GPU): ``pool_ref`` against ``oracle.max_pool``, against
values worked out by hand and against a transcription of Caffe's size formula; the integer grids stay exact; the detector's text
parses and its oracle forward yields rows."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import prototxt as P
from tests import pooling_cases as K

F32 = np.float32
F64 = np.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


SQUARE_MAX = [c for c in K.WINDOW_CASES if c[1] == "MAX" and c[2] == c[3] and c[4] == c[5] and c[6] == c[7]]


@pytest.mark.parametrize("case", SQUARE_MAX + [(8, "MAX", 2, 2, 2, 2, 0, 0, 7, 9, False), (8, "MAX", 3, 3, 2, 2, 1, 1, 8, 10, False)], ids=K.case_id)
def test_max_equals_the_oracle_on_square_windows(case):
    C, m, kh, kw, sh, sw, ph, pw, h, w, gl = case
    x = K.random_grid((2, C, h, w), seed=C + h)
    got, _ = K.case_ref(case, x)
    want = O.max_pool(x, kh, sh, ph)
    assert got.shape == want.shape
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_ave_with_a_unit_kernel_is_the_identity():
    x = K.random_grid((1, 5, 4, 7), seed=3)
    for f64 in (False, True):
        got, mag = K.pool_ref(x, "AVE", 1, 1, 1, 1, 0, 0, False, f64)
        np.testing.assert_array_equal(_bits(got), _bits(x))
        np.testing.assert_array_equal(mag, np.abs(x.astype(F64)))


def test_a_padded_corner_by_hand():
    """3x3 stride 2 pad 1 on 4 x 4: the corner window covers rows / columns -1 .. 1, divisor 9 over the four values inside; the
    last window (start 3, end min(6, 5) = 5) covers 2 x 2 of the padded map, one value inside: divisor 4."""
    x = np.arange(16, dtype=F32).reshape(1, 1, 4, 4)
    got, mag = K.pool_ref(x, "AVE", 3, 3, 2, 2, 1, 1, False)
    assert got.shape == (1, 1, 3, 3)
    assert got[0, 0, 0, 0] == F32(F32(0 + 1 + 4 + 5) / F32(9)) and mag[0, 0, 0, 0] == 10
    assert got[0, 0, 1, 1] == F32(F32(sum(range(16)) - 0 - 1 - 2 - 3 - 4 - 8 - 12) / F32(9))
    assert got[0, 0, 2, 2] == F32(15.0 / 4.0) and got[0, 0, 0, 2] == F32(F32(3 + 7) / F32(6))
    one, _ = K.pool_ref(np.full((1, 1, 1, 1), 3, F32), "AVE", 3, 3, 1, 1, 1, 1, False)
    assert one.shape == (1, 1, 1, 1) and one[0, 0, 0, 0] == F32(3) / F32(9)
    top, _ = K.pool_ref(x, "MAX", 3, 3, 2, 2, 1, 1, False)
    np.testing.assert_array_equal(top[0, 0], [[5, 7, 7], [13, 15, 15], [13, 15, 15]])


def test_divisors_of_the_ceil_sized_windows():
    """AVE 2x2/2 on 7 x 9: the last row's windows hold 2 values (divisor 2), the corner one value (divisor 1)."""
    x = np.ones((1, 1, 7, 9), F32)
    x[0, 0, 6, 8] = 5
    got, _ = K.pool_ref(x, "AVE", 2, 2, 2, 2, 0, 0, False)
    assert got.shape == (1, 1, 4, 5) and (got[0, 0, :3, :4] == 1).all() and got[0, 0, 3, 4] == 5 and got[0, 0, 3, 0] == 1
    # the drop rule on both axes: 2x2/2 pad 1 on 3 x 5 would be 3 x 4 by the ceil formula
    assert K.out_size(3, 5, 2, 2, 2, 2, 1, 1) == (2, 3)


def _caffe_size(n, k, s, p, any_pad):
    """pooling_layer.cpp's Reshape for one axis, transcribed."""
    o = int(math.ceil(float(n + 2 * p - k) / s)) + 1
    if any_pad and (o - 1) * s >= n + p:
        o -= 1
    return o


def test_output_sizes_over_a_sweep():
    n = 0
    for h in range(1, 12):
        for k in range(1, 6):
            for s in range(1, 4):
                for p in range(0, k):
                    if h + 2 * p < k or (s > k and not p):      # (no pad and a stride beyond the kernel: Caffe's last window may be empty)
                        continue
                    for pw in (0, p):
                        want = (_caffe_size(h, k, s, p, p or pw), _caffe_size(h + 1, k, s, pw, p or pw))
                        if h + 1 + 2 * pw < k:
                            continue
                        assert K.out_size(h, h + 1, k, k, s, s, p, pw) == want, (h, k, s, p, pw)
                        x = np.ones((1, 1, h, h + 1), F32)
                        assert K.pool_ref(x, "AVE", k, k, s, s, p, pw, False)[0].shape[2:] == want
                        n += 1
    assert n > 500


@pytest.mark.parametrize("case", K.ALL_CASES, ids=K.case_id)
def test_integer_grids_stay_exact(case):
    """max |sum| < 2^24: fp32 in any order, binary64 and the tree all give the same integer before the division."""
    x = K.case_inputs(case, "int")[:, K.layer_params(case)[1]]
    top, mag = K.case_ref(case, x)
    assert mag.max() < 2.0 ** 24 and np.abs(x).max() <= 4 and (x == np.round(x)).all()
    top64, _ = K.case_ref(case, x, f64=True)
    assert top.shape == (K.batch(case), case[0]) + K.case_out_size(case)
    if case[1] == "MAX":
        np.testing.assert_array_equal(_bits(top), _bits(top64))
    else:
        assert (np.abs(top.astype(F64) - top64.astype(F64)) <= np.spacing(np.abs(top64))).all()


def test_random_grids_are_fp16_values():
    x = K.random_grid((1, 16, 9, 11), seed=2)
    np.testing.assert_array_equal(x, x.astype(np.float16).astype(F32))
    nz = np.abs(x[x != 0])
    assert nz.min() >= 2.0 ** -8 and nz.max() / nz.min() > 1000 and nz.max() < 60000


def test_tree_chain_and_threshold():
    assert K.tree_chain(33, 67) == 35 + 6 and K.tree_chain(3, 6) == 1 + 6
    assert [K.above_t(c) for c in K.GLOBAL_CASES[:6]] == [False, False, False, True, True, True]
    assert any(K.above_t(c) for c in K.GLOBAL_CASES) and all(not K.above_t(c) for c in K.WINDOW_CASES)


def test_layer_texts_parse():
    for case in K.ALL_CASES:
        msg = P.parse(K.layer_net_text(case))
        pool = [L for L in msg.getall("layer") if str(L.get("type")) == "Pooling"]
        assert len(pool) == 1 and K.pool_spec(pool[0]) == tuple(case[1:8]) + (case[10],), K.case_id(case)
    for txt in (K.concat_net_text(12), K.concat_net_text(6), K.fold_net_text("AVE"), K.fold_net_text("MAX"), K.exponent_net_text(),
                K.global_net_text(7, 9), K.group_net_text(7, 9)):
        assert len(P.parse(txt).getall("layer")) >= 2


def test_pool_mini_parses_and_its_oracle_yields_rows():
    msg = K.pool_mini()
    types = [str(L.get("type")) for L in msg.getall("layer")]
    assert types.count("Pooling") == 4 and types.count("Eltwise") == 1 and types.count("Concat") == 2 and types.count("Python") == 1
    assert P.dumps(P.parse(P.dumps(msg))) == P.dumps(msg)
    h, w = K.PM_GROUP_SIZES[1]
    data, info = K.pool_mini_unit(h, w)
    onet = K.forwarded(K.pool_mini_oracle(h, w), data, info)
    for name, hw in K.pool_mini_map_sizes(h, w).items():
        assert onet.blobs[name].data.shape[2:] == hw, name
    assert onet.blobs["cat1"].data.shape[1] == 48 and onet.blobs["i_cat"].data.shape[1] == 128
    # the AVE layers really average: the transition's pooled map against numpy's mean on the even part of the map
    tr, tp = onet.blobs["tr"].data, onet.blobs["tr_pool"].data
    hh, ww = tr.shape[2] // 2, tr.shape[3] // 2
    mean = tr[:, :, :2 * hh, :2 * ww].astype(F64).reshape(1, -1, hh, 2, ww, 2).mean(axis=(3, 5))
    assert np.abs(tp[:, :, :hh, :ww] - mean).max() <= 1e-6 * np.abs(mean).max()
    rows = onet.blobs["cls_prob_16"].data
    assert len(rows) > 1 and onet.blobs["boxes_16"].data.shape == (len(rows), 5)
