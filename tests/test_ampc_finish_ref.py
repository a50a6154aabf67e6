"""tests/ampc_finish_ref.py pinned by hand-made cases (no GPU): the model tests/test_ampc_finish.py compares the device with."""
import math
import struct

import numpy as np

from tests import ampc_finish_ref as fref

INF = math.inf
NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]


def test_ties_rank_by_id():
    """2.0, 2.0, 1.0: the two equal values rank in id order, whichever way the ids were listed, and the id order is 128-bit"""
    ids, vals, ranks = fref.finish({30: 2.0, 10: 2.0, 20: 1.0}, 1.0)
    assert ids == [10, 20, 30] and vals.tolist() == [2.0, 1.0, 2.0] and ranks == [0, 2, 1]
    lo, hi = 7, 7 | (1 << 64)  # one low half: only the high word tells them apart
    ids, vals, ranks = fref.finish({hi: 2.0, lo: 2.0, 3 | (1 << 64): 2.0}, 1.0)
    assert ids == [lo, 3 | (1 << 64), hi] and ranks == [0, 1, 2]


def test_total_cmp_order():
    """+NaN > +inf > 1 > +0.0 > -0.0 > -1 > -inf > -NaN, where IEEE comparison knows neither the NaNs nor the two zeros apart"""
    order = [POS_NAN, INF, 1.0, 0.0, -0.0, -1.0, -INF, NEG_NAN]
    keys = [fref.total_key(v) for v in order]
    assert keys == sorted(keys, reverse=True) and len(set(keys)) == len(keys)
    assert fref.bits(NEG_NAN) >> 63 == 1 and fref.bits(POS_NAN) >> 63 == 0
    model = {100 - i: v for i, v in enumerate(order)}  # descending values on descending ids: the values decide, not the ids
    ids, vals, ranks = fref.finish(model, 1.0)
    assert [ranks[ids.index(100 - i)] for i in range(len(order))] == list(range(len(order)))
    # subnormals order by magnitude on both sides of the zeros
    tiny = 5e-324
    assert fref.total_key(tiny) > fref.total_key(0.0) > fref.total_key(-0.0) > fref.total_key(-tiny)


def test_quotient_is_taken_before_the_order():
    """a divisor of -1.0 reverses the order, 0.0 folds everything onto inf / NaN (then the ids decide within each), inf onto zeros"""
    model = {1: 1.0, 2: 2.0, 3: -3.0, 4: 0.0}
    assert fref.finish(model, -1.0)[2] == [2, 3, 0, 1]  # quotients -1, -2, 3, -0.0
    ids, vals, ranks = fref.finish(model, 0.0)  # inf, inf, -inf, NaN
    assert [fref.bits(v) for v in vals[:3]] == [fref.bits(INF), fref.bits(INF), fref.bits(-INF)] and math.isnan(vals[3])
    assert ranks[0] < ranks[1] < ranks[2]  # the two infinities by id, -inf below them; the NaN goes where its sign puts it
    assert fref.finish(model, INF)[2] == [0, 1, 3, 2]  # +0.0, +0.0, -0.0, +0.0: the zeros' signs and then the ids
    third = fref.finish({1: 1.0}, 3.0)[1][0]
    assert fref.bits(third) == fref.bits(np.float64(1.0) / np.float64(3.0)) == 0x3FD5555555555555


def test_top_k_vectors_of_the_reference():
    """webgraph/centrality/mod.rs test_top_k_reversed: values 0 .. 9 on ids 0 .. 9, the largest first; test_top_k's ascending lists are
    the same vectors under a divisor of -1.0"""
    model = {i: float(i) for i in range(10)}
    ids, vals, _ = fref.finish(model, 1.0)
    assert fref.top(ids, vals, 5) == [(9, 9.0), (8, 8.0), (7, 7.0), (6, 6.0), (5, 5.0)]
    assert fref.top(ids, vals, 3) == [(9, 9.0), (8, 8.0), (7, 7.0)]
    assert fref.top(ids, vals, 0) == []
    assert len(fref.top(ids, vals, 11)) == 10
    ids, vals, _ = fref.finish(model, -1.0)
    assert [k for k, _ in fref.top(ids, vals, 5)] == [0, 1, 2, 3, 4]
    assert [k for k, _ in fref.top(ids, vals, 3)] == [0, 1, 2]


def test_ranks_are_a_permutation_and_top_follows_them():
    rng = np.random.default_rng(3)
    model = {int(k): float(v) for k, v in zip(rng.integers(0, 1 << 62, 200), rng.integers(0, 5, 200))}
    ids, vals, ranks = fref.finish(model, 3.0)
    assert sorted(ranks) == list(range(len(ids)))
    by_rank = sorted(range(len(ids)), key=lambda j: ranks[j])
    assert fref.top(ids, vals, 50) == [(ids[j], vals[j]) for j in by_rank[:50]]
