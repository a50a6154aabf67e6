"""tests/ampc_round_ref.py pinned on the reference's own answers and on its arithmetic written out (no GPU)."""
import math

import numpy as np
import pytest

from tests import ampc_round_ref as rref


def test_bloom_known_answer_of_the_reference():
    """crates/bloom/src/lib.rs:198-216"""
    f = rref.Bloom(rref.bloom_num_bits(100, 0.01))
    assert f.num_bits == 120
    for k in range(1, 6):
        f.insert(k)
    assert [f.contains(k) for k in range(1, 11)] == [True] * 5 + [False] * 5
    assert f.count() == 5 and int(f.words().view(np.uint64)[0]) | (int(f.words()[1]) << 64) == sum(1 << i for i in f.ones)


@pytest.mark.parametrize("items,fp,want", [(100, 0.01, 120), (1, 0.05, 1), (10 ** 8, 0.05, 77940303), (3 * 10 ** 8, 0.01, 359439690)])
def test_bloom_num_bits(items, fp, want):
    """ceil(items * ln(fp) / (-8 * ln(2)^2)); the quotients are 119.81, 0.78, 77940302.87 and 359439689.15: no rounding of a logarithm moves
    their ceilings"""
    assert rref.bloom_num_bits(items, fp) == want
    assert want == math.ceil(items * math.log(fp) / (-8 * math.log(2) ** 2))


def test_the_high_half_is_ignored_by_a_sketch_and_kept_by_an_exact_set():
    a, b = 5 | (1 << 64), 5 | (2 << 64)
    assert rref.bloom_slot(a, 4099) == rref.bloom_slot(b, 4099) == (5 * rref.LARGE_PRIME % (1 << 64)) % 4099
    e = rref.Exact([a])
    assert e.contains(a) and not e.contains(b)


def test_updated_nodes_policy():
    """add() turns an exact set into a sketch of all of its ids past 16 384; Exact u Exact past it keeps the LEFT ids only
    (updated_nodes.rs:48-58); a union with a sketch inserts the exact ids"""
    u = rref.UpdatedNodes(100_000)
    for k in range(rref.SKETCH_THRESHOLD):
        u.add(k + 1)
    assert u.inner.kind == "exact"
    u.add(10 ** 9)
    assert u.inner.kind == "sketch" and all(u.contains(k) for k in (1, 777, rref.SKETCH_THRESHOLD, 10 ** 9))
    left, right = rref.UpdatedNodes(100_000, rref.Exact(range(1, 9001))), rref.UpdatedNodes(100_000, rref.Exact(range(20_001, 28_001)))
    both = left.union(right)
    assert both.inner.kind == "sketch" and both.inner.num_bits == rref.bloom_num_bits(100_000, 0.01)
    want = rref.Bloom(both.inner.num_bits)
    for k in range(1, 9001):
        want.insert(k)
    assert both.inner.ones == want.ones
    small = rref.UpdatedNodes(100_000, rref.Exact([5, 6])).union(rref.UpdatedNodes(100_000, rref.Exact([6, 7])))
    assert small.inner.kind == "exact" and small.inner.ids == {5, 6, 7}
    mixed = rref.UpdatedNodes(100_000, rref.Exact([123456789])).union(both)
    assert mixed.inner.ones == want.ones | {rref.bloom_slot(123456789, want.num_bits)}
