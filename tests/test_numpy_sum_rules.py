"""The two numpy summation rules that the device bbox_vote restates (csrc/merge.hip), pinned on the CPU.

bbox_vote (lib/test.py:209) divides np.sum(det_accu[:, 0:4], axis=0) by np.sum(det_accu[:, -1:]):
  * the axis-0 sum of the (m, 4) products is a plain sequential sum, row after row;
  * the full sum of the strided score column goes through numpy's buffered reduction: the column is copied into
    buffers of NPY_BUFSIZE = 8192 elements, each buffer is summed pairwise (PW_BLOCKSIZE = 128, 8 accumulators),
    and the buffer sums are added in order onto the identity 0.
If a numpy upgrade changes either rule, these tests fail here instead of as an unexplained mismatch on the GPU."""
import numpy as np
import pytest

F32 = np.float32


def pairwise(a):
    """numpy's pairwise_sum (umath/loops_utils.h.src) on a 1-D float32 array, in float32."""
    n = len(a)
    if n < 8:
        r = F32(0)
        for x in a:
            r = F32(r + x)
        return r
    if n <= 128:
        r = [F32(x) for x in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = F32(r[j] + a[i + j])
            i += 8
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        for x in a[i:]:
            res = F32(res + x)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(pairwise(a[:n2]) + pairwise(a[n2:]))


def blocked(a, block=8192):
    res = F32(0)
    for s in range(0, len(a), block):
        res = F32(res + pairwise(a[s:s + block]))
    return res


@pytest.mark.parametrize("m", [100, 8192, 8193, 9000, 20000])
def test_strided_score_sum_is_blocked_pairwise(m):
    a = np.random.default_rng(m).uniform(0.05, 1, (m, 5)).astype(F32)
    got = np.sum(a[:, -1:])
    assert got.dtype == F32
    assert got == blocked(a[:, 4])


@pytest.mark.parametrize("m", [9000, 20000])
def test_blocked_sum_is_not_one_pairwise_sum(m):
    """The blocking matters: past 8192 elements one pairwise sum over the whole column is a different rounding
    (for some inputs; the two agree on others)."""
    cols = [np.random.default_rng(s).uniform(0.05, 1, (m, 5)).astype(F32)[:, -1:] for s in range(8)]
    assert all(np.sum(c) == blocked(c[:, 0]) for c in cols)
    assert any(np.sum(c) != pairwise(c[:, 0]) for c in cols)


@pytest.mark.parametrize("m", [100, 8192, 8193, 20000])
def test_axis0_box_sum_is_sequential(m):
    a = np.random.default_rng(m + 1).uniform(0, 2000, (m, 5)).astype(F32)
    want = a[0, 0:4].copy()
    for i in range(1, m):
        want = (want + a[i, 0:4]).astype(F32)
    np.testing.assert_array_equal(np.sum(a[:, 0:4], axis=0), want)
