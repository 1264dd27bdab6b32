"""The grouped forward's unit ordering and chunking (smallhardface_amd.test.group_units): pure Python, no GPU.

detect() feeds the net level i, then level i flipped (lib/test.py:141-158); concatenating the per-unit results in that order
is what makes the grouped detections those of the ungrouped loop, so the order and the completeness are pinned here."""
import pytest

from smallhardface_amd import _lib
from smallhardface_amd.test import GROUP_UNITS, group_units


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("n_levels", [1, 5, 8, 9])
def test_group_units_order_and_chunks(n_levels, flip):
    chunks = group_units(n_levels, flip)
    flat = [u for ch in chunks for u in ch]
    # the reference's loop, written out
    want = []
    for i in range(n_levels):
        want.append((i, False))
        if flip:
            want.append((i, True))
    assert flat == want                                   # nothing dropped, nothing repeated, the reference's order
    assert all(1 <= len(ch) <= 16 for ch in chunks)
    assert [len(ch) for ch in chunks[:-1]] == [16] * (len(chunks) - 1)     # only the last chunk is short
    assert len(chunks) == (len(want) + 15) // 16


def test_group_units_chunk_sizes():
    assert GROUP_UNITS == 16
    assert [len(c) for c in group_units(9, True)] == [16, 2]
    assert [len(c) for c in group_units(8, True)] == [16]
    assert [len(c) for c in group_units(9, False)] == [9]
    assert [len(c) for c in group_units(5, True, max_group=4)] == [4, 4, 2]
    assert group_units(5, True, max_group=4)[1] == [(2, False), (2, True), (3, False), (3, True)]
    assert group_units(0, True) == []
    with pytest.raises(ValueError):
        group_units(3, True, max_group=0)


def test_the_two_entry_points_are_declared():
    names = _lib.declared_symbols()
    assert "shf_net_forward_group" in names and "shf_blob_load_device_group" in names
