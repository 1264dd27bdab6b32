"""The table of tests/buffer_history_cases.py, checked without a GPU before any GPU time is spent on it: the sequence's shape
and size rules, the family's oracle at every size (so no size is refused for a kernel extent or a pooling geometry, and every
recorded blob exists), the largest size of the graph's own tests, and more than one row in every cls_prob* output at the
family's threshold settings."""
import numpy as np
import pytest

from tests import buffer_history_cases as B

_ORACLES = {}


def _oracle(key, size):
    if (key, size) not in _ORACLES:
        _ORACLES[(key, size)] = B.CASES[key].oracle(*size)
    return _ORACLES[(key, size)]


def test_the_table_names_every_key_of_the_scenarios():
    assert len(B.KEYS) == 16 and len(set(B.KEYS)) == 16
    for keys in (B.EXTRA_KEYS, B.GROUP_KEYS, B.FORM_KEYS, B.LOOSE):
        assert set(keys) <= set(B.KEYS)
    assert all(B.CASES[k].group_sizes and len(B.CASES[k].group_sizes) == 3 for k in B.GROUP_KEYS)
    assert B.MODE_WALK[0] == B.MODE_WALK[-1] == "fp32" and set(B.MODE_WALK) == set(B.MODES + B.EXTRA_MODES)


@pytest.mark.parametrize("key", B.KEYS)
def test_sequence_shape_and_size_rules(key):
    case = B.CASES[key]
    a, b, c = case.sizes
    area = lambda s: s[0] * s[1]      # noqa: E731
    assert case.sequence("fp32") == case.sequence("f16x3") == [a, b, a, c, b]
    assert case.sequence("bf16") == case.sequence("f64") == [a, b, a]
    assert case.modes == B.MODES + (B.EXTRA_MODES if key in B.EXTRA_KEYS else ())
    assert area(c) >= B.MIN_GROWTH * area(a), (a, c)                     # past DevBuf's 1/8 of slack: a reallocation
    assert area(b) < area(a) and b[0] <= a[0] and b[1] <= a[1], (a, b)
    if key not in B.LOOSE:
        assert b[0] < a[0] and b[1] < a[1], (a, b)
        assert c[0] > a[0] and c[1] > a[1], (a, c)
    for s in case.distinct_sizes("fp32"):
        assert s[0] <= case.largest[0] and s[1] <= case.largest[1], (s, case.largest)
    if key in ("resblock", "m1", "chain"):                               # "two smaller ragged sizes": odd in both directions
        assert all(v % 2 == 1 for s in (a, b) for v in s)


@pytest.mark.parametrize("key", B.KEYS)
def test_the_oracle_forwards_at_every_size_with_more_than_one_row(key):
    case = B.CASES[key]
    for size in case.distinct_sizes("fp32"):
        onet = _oracle(key, size)
        for name in case.blobs + case.last:
            assert name in onet.blobs and np.isfinite(onet.blobs[name].data).all(), (size, name)
            assert onet.blobs[name].data.size > 0, (size, name)
        assert tuple(onet.blobs["data"].data.shape[2:]) == size
        rows = {o: len(onet.blobs[o].data) for o in onet.outputs if o.startswith("cls_prob")}
        assert all(n > 1 for n in rows.values()), (size, rows)
        assert rows or key == "pool_group"                               # (the one graph without a proposal tail)


def test_pool_group_sizes_lie_on_both_sides_of_the_walk_form():
    from tests import pooling_cases as K
    assert sorted(h * w > K.GLOBAL_T for h, w in B.CASES["pool_group"].sizes) == [False, True, True]


def test_slim_sizes_are_one_tile_four_ragged_tiles_and_nine():
    """The slim form is the planner's choice at every size (it goes by the layer's channels): what the sizes cross is the tile
    count -- 9 x 17 is 2 x 2 ragged 8 x 16 tiles, 8 x 16 exactly one, 23 x 40 is 3 x 3."""
    plans = [B.slim_plan(*s) for s in B.CASES["slim"].sizes]
    assert [p["grid"] for p in plans] == [4, 1, 9] and [p["slim"] for p in plans] == [1, 1, 1], plans


def test_units_are_a_function_of_the_size_alone():
    for key in ("template_dd", "fam16", "slim", "pool_group"):
        case = B.CASES[key]
        (_, n1, d1, i1), (_, n2, d2, i2) = case.setup(*case.sizes[1]), case.setup(*case.sizes[1])
        np.testing.assert_array_equal(d1, d2)
        np.testing.assert_array_equal(i1, i2)
        assert sorted(n1.params) == sorted(n2.params)
        for name in n1.params:
            for x, y in zip(n1.params[name], n2.params[name]):
                np.testing.assert_array_equal(x, y)
