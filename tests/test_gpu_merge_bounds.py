"""The box-merge kernels at their size boundaries, against the oracle, exactly.

  sort            csrc/tail.hip bitonic sort: one LDS chunk of SORT_CH = 16384 keys, or global steps + local merges
  greedy scan     csrc/merge.hip greedy_scan_kernel: 64-box words, 16 waves x SCAN_PRE words fetched ahead, a
                  4096-word LDS bitmap (262144 boxes, refused beyond)
  vote            csrc/merge.hip vote_accumulate_kernel: the member list spans words past 64, pairwise_array recurses
                  past 128, clusters past VOTE_CAP = 1024 go to vote_one_serial, numpy's score sum is blocked past 8192
  score keys      make_keys_kernel and the tail decode's keys: the sign of the score

nms / bbox_vote restate lib/nms and lib/test.py op for op, so every comparison is exact.  Inputs are built so that the
oracle stays cheap: nms(d, 1.0) suppresses nothing (IoU never exceeds 1), vote clusters are dense (one oracle turn per
cluster), and the long chains are run through the oracle once per threshold."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from smallhardface_amd import caffe
from smallhardface_amd._lib import ShfError
from smallhardface_amd.nms import bbox_vote, nms
from tests import helpers as H

pytestmark = pytest.mark.gpu

BOX_TOL = 1e-3   # px, as in test_gpu_golden.py: device expf vs numpy's float32 exp
SCAN_LIMIT = 262144


def vote_oracle(d, thr):
    with np.errstate(divide="ignore", invalid="ignore"):   # (clusters whose signed scores sum to 0: inf / nan, as on the device)
        return np.asarray(O.bbox_vote(d, thr), dtype=np.float64)


def int_boxes(rng, n, span=1000):
    """Boxes with small integer corners: areas and intersections are exact in fp32, so IoU <= 1 holds exactly."""
    xy = rng.integers(0, span, (n, 2))
    wh = rng.integers(1, 100, (n, 2))
    return np.hstack([xy, xy + wh]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# sort: n around every 64-box word, LDS chunk and global-step boundary; nothing suppressed, so keep == canonical order
# ---------------------------------------------------------------------------------------------------------------------
SORT_NS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 32769, 65537]


def sort_scores(rng, n, pattern):
    if pattern == "distinct":
        return (rng.permutation(n) + 1).astype(np.float32) / np.float32(n)
    if pattern == "ties":      # 8 values: tied runs cross word, chunk and global-step boundaries
        return (rng.integers(1, 9, n) / 8).astype(np.float32)
    if pattern == "equal":
        return np.full(n, 0.5, np.float32)
    assert pattern == "signed"  # distinct values of both signs, with +0.0 and -0.0 in the middle
    s = (rng.permutation(n) - n // 2).astype(np.float32) / np.float32(n)
    s[rng.integers(0, n, max(n // 16, 1))] = -0.0
    s[rng.integers(0, n, max(n // 16, 1))] = 0.0
    return s


@pytest.mark.parametrize("pattern", ["distinct", "ties", "equal", "signed"])
@pytest.mark.parametrize("n", SORT_NS)
def test_sort_at_chunk_boundaries(n, pattern):
    rng = np.random.default_rng(n * 7 + len(pattern))
    d = np.hstack([int_boxes(rng, n), sort_scores(rng, n, pattern)[:, None]])
    np.testing.assert_array_equal(np.asarray(nms(d, 1.0), dtype=np.int64), O.canonical_order(d[:, 4]))


# ---------------------------------------------------------------------------------------------------------------------
# greedy scan: a row of 100x100 boxes where only neighbours overlap above the threshold and scores fall along the row.
# Greedy keeps every other box, so each 64-box word depends on the one before it.
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_NS = [63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 20000]
# box spacing per threshold: neighbour IoU (100-s)/(100+s) above it, two apart (100-2s)/(100+2s) below it
CHAIN_STEP = {0.3: 40, 0.4: 30, 0.7: 13}


def chain(n, thr):
    x = np.arange(n, dtype=np.float64) * CHAIN_STEP[thr]
    z = np.zeros(n)
    return np.stack([x, z, x + 99, z + 99, np.linspace(1.0, 0.01, n)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def chain_oracle(n, thr, vote):
    d = chain(n, thr)
    return vote_oracle(d, thr) if vote else O.nms(d, thr)


@pytest.mark.parametrize("thr", sorted(CHAIN_STEP))
@pytest.mark.parametrize("n", CHAIN_NS)
def test_greedy_scan_chain(n, thr):
    d = chain(n, thr)
    want = chain_oracle(n, thr, False)
    assert len(want) == (n + 1) // 2          # the input is the chain it claims to be
    np.testing.assert_array_equal(np.asarray(nms(d, thr), dtype=np.int64), want)
    # the same boxes in a random row order: scores are distinct, so the oracle's keep maps through the permutation
    # and its vote rows do not change (the oracle itself is O(n^2) on a chain: run once per length and threshold)
    p = np.random.default_rng(n).permutation(n)
    inv = np.argsort(p)
    np.testing.assert_array_equal(np.asarray(nms(d[p], thr), dtype=np.int64), inv[want])
    if n == 20000 and thr != 0.4:
        return   # (host time: the vote oracle's np.delete is quadratic on a chain; 0.4 covers the length)
    wv = chain_oracle(n, thr, True)
    assert len(wv) == n // 2 + n % 2          # pairs, and the last box alone when n is odd (kept: nothing after it)
    np.testing.assert_array_equal(bbox_vote(d, thr), wv)
    np.testing.assert_array_equal(bbox_vote(d[p], thr), wv)


def test_scan_capacity_refused_before_any_work():
    """More boxes than the scan bitmap holds: a clean error naming the limit, raised before the merge context grows a
    buffer (the IoU mask alone would be 8.6 GB at this n), and the context still serves the next call."""
    rng = np.random.default_rng(5)
    small = np.hstack([int_boxes(rng, 500), rng.uniform(0.05, 1, (500, 1)).astype(np.float32)])
    np.testing.assert_array_equal(np.asarray(nms(small, 0.4), dtype=np.int64), O.nms(small, 0.4))
    big = np.hstack([int_boxes(rng, SCAN_LIMIT + 1, 50000),
                     rng.uniform(0.05, 1, (SCAN_LIMIT + 1, 1)).astype(np.float32)])
    before = caffe.alloc_counts()[0]
    with pytest.raises(ShfError, match=str(SCAN_LIMIT)):
        nms(big, 0.4)
    with pytest.raises(ShfError, match=str(SCAN_LIMIT)):
        bbox_vote(big, 0.4)
    assert caffe.alloc_counts()[0] == before   # no device buffer was grown for the refused calls
    np.testing.assert_array_equal(np.asarray(nms(small, 0.3), dtype=np.int64), O.nms(small, 0.3))
    np.testing.assert_array_equal(bbox_vote(small, 0.4), vote_oracle(small, 0.4))


# ---------------------------------------------------------------------------------------------------------------------
# vote: dense clusters of m jittered copies of one box (every pair has IoU >= 0.92), far apart from each other
# ---------------------------------------------------------------------------------------------------------------------
CLUSTER_MS = [2, 63, 64, 65, 127, 128, 129, 130, 1000, 1023, 1024, 1025, 4096, 8192, 8193, 9000, 20000]


def jitter_cluster(rng, m, k, lo, hi):
    x0, y0 = 1000.0 * (k % 16), 1000.0 * (k // 16)
    xy = np.array([x0, y0, x0 + 200, y0 + 200]) + rng.uniform(-2, 2, (m, 4))
    return np.hstack([xy, rng.uniform(lo, hi, (m, 1))]).astype(np.float32)


def lone(k, score):
    x0, y0 = 1000.0 * (k % 16), 1000.0 * (k // 16)
    return np.array([[x0, y0, x0 + 50, y0 + 50, score]], np.float32)


def cluster_case(m, variant):
    rng = np.random.default_rng(m * 4 + len(variant))
    if variant == "head_first":       # sorted rows: the head is input row 0
        d = jitter_cluster(rng, m, 0, 0.05, 1.0)
        return d[O.canonical_order(d[:, 4])]
    if variant == "negative":         # all scores < 0: the reported max is the largest negative one
        d = np.vstack([jitter_cluster(rng, m, 0, -1.0, -0.05), lone(1, -2.0)])
        return d[rng.permutation(len(d))]
    if variant == "shuffled":         # head anywhere; a lone box in the middle (dropped) and one at the end (kept)
        d = np.vstack([jitter_cluster(rng, m, 0, 0.1, 1.0), lone(1, 0.5)])
        return np.vstack([d[rng.permutation(len(d))], lone(2, 0.01)])
    assert variant == "interleaved"   # 3-5 clusters mixed in input and score order: members spread over many words
    sizes = [m] + list(rng.choice(CLUSTER_MS, 2 + m % 3))
    d = np.vstack([jitter_cluster(rng, s, k, 0.1, 1.0) for k, s in enumerate(sizes)] + [lone(len(sizes), 0.5)])
    return np.vstack([d[rng.permutation(len(d))], lone(len(sizes) + 1, 0.01)])


@pytest.mark.parametrize("variant", ["head_first", "shuffled", "interleaved", "negative"])
@pytest.mark.parametrize("m", CLUSTER_MS)
def test_vote_cluster_sizes(m, variant):
    d = cluster_case(m, variant)
    want = vote_oracle(d, 0.4)
    np.testing.assert_array_equal(bbox_vote(d, 0.4), want)
    np.testing.assert_array_equal(np.asarray(nms(d, 0.4), dtype=np.int64), O.nms(d, 0.4))


# ---------------------------------------------------------------------------------------------------------------------
# signs: nms / bbox_vote are drop-ins for any (N, 5) array, and the proposal layer takes the probabilities it is given
# ---------------------------------------------------------------------------------------------------------------------
def signed_case(kind, n=3000):
    rng = np.random.default_rng(len(kind))
    c = rng.integers(0, 1500, (n, 2))
    s = rng.integers(20, 80, (n, 2))
    if kind == "mixed":
        sc = rng.uniform(-1, 1, n)
    elif kind == "negative":
        sc = rng.uniform(-1, -1e-3, n)
    else:
        assert kind == "zeros"   # +0.0 and -0.0 tie, by input index
        sc = rng.choice(np.array([0.0, -0.0, 0.25, -0.25], np.float32), n)
    return np.hstack([c, c + s, sc[:, None]]).astype(np.float32)


@pytest.mark.parametrize("kind", ["mixed", "negative", "zeros"])
def test_signed_scores(kind):
    d = signed_case(kind)
    np.testing.assert_array_equal(np.asarray(nms(d, 1.0), dtype=np.int64), O.canonical_order(d[:, 4]))
    for thr in (0.3, 0.7):
        np.testing.assert_array_equal(np.asarray(nms(d, thr), dtype=np.int64), O.nms(d, thr))
        np.testing.assert_array_equal(bbox_vote(d, thr), vote_oracle(d, thr))


@pytest.fixture(scope="module")
def net():
    from smallhardface_amd import prototxt as P
    return caffe.Net(None, prototxt_text=P.dumps(H.detector_msg(True)))


def proposal_inputs(rng, h, w, fg):
    sc = np.concatenate([1 - fg, fg], 0)[None].astype(np.float32)
    dl = rng.normal(0, 0.2, (1, 12, h, w)).astype(np.float32)
    return sc, dl, np.array([[h * 8, w * 8, 1.0]], np.float32)


def check_proposal(net, sc, dl, ii, topn, thr):
    net.set_proposal_cfg(topn, thr, 0.0)
    boxes, probs, _ = net.debug_proposal(sc, dl, ii)
    ob, op = O.proposal_forward(sc, dl, ii, O.ProposalParams(pre_nms_topN=topn, score_thresh=thr))
    assert boxes.shape == ob.shape
    np.testing.assert_array_equal(probs, op)
    assert np.abs(boxes - ob).max() < BOX_TOL
    return probs


def test_proposal_best_anchor_below_threshold_with_negative_scores(net):
    """Nothing reaches score_thresh: the layer keeps the single best anchor (proposal_layer.py:182-188), and 'best'
    is the largest score even when most scores are negative and some are -0.0."""
    rng = np.random.default_rng(21)
    h, w = 6, 7
    fg = rng.uniform(-0.5, 0.0015, (3, h, w)).astype(np.float32)
    fg.reshape(-1)[rng.integers(0, fg.size, 12)] = -0.0
    assert (fg > 0).any() and (fg < 0).any()
    probs = check_proposal(net, *proposal_inputs(rng, h, w, fg), 10000, 0.002)
    assert probs.shape == (1, 2) and probs[0, 1] == fg.max()


@pytest.mark.parametrize("cands,topn", [(16384, 10000), (16385, 10000), (16385, 20000), (32769, 20000),
                                        (32769, 40000)])
def test_tail_sort_across_chunk_boundary(net, cands, topn):
    """`cands` anchors at or above score_thresh (the tail sorts exactly those keys: one LDS chunk at 16384, global
    steps beyond), on 8 tied score values so that tied runs cross the pre_nms_topN cut and every chunk boundary."""
    rng = np.random.default_rng(cands + topn)
    h = w = 75 if cands < 32768 else 105
    total = 3 * h * w
    fg = rng.uniform(0.0, 0.0015, total).astype(np.float32)
    on = rng.permutation(total)[:cands]
    fg[on] = (rng.integers(1, 9, cands) / 8).astype(np.float32)
    probs = check_proposal(net, *proposal_inputs(rng, h, w, fg.reshape(h, w, 3).transpose(2, 0, 1)), topn, 0.002)
    assert len(probs) == min(cands, topn)
