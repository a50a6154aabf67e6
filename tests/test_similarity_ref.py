"""The host restatement of the inbound similarity (tests/inbound_similarity_ref.py) against values worked out by hand, the identities the
device code rests on, and its vectorised form against the literal one.  No GPU."""
import json
import os

import numpy as np

from tests import graphs
from tests import inbound_similarity_ref as sref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similarity_cases.json")


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g, graphs.dense_from_tuples([tuple(e) for e in g["edges"]])


def test_golden_values():
    g, (ids, row_ptr, src) = _golden()
    bv = sref.bitvecs(ids, row_ptr, src)
    ints = sref.id_ints(ids)
    for case in g["cases"]:
        ss = 1.0 if case["self_score"] is None else case["self_score"]
        got = sref.literal(ids, row_ptr, src, case["liked"], case["disliked"], case["normalized"], ss, bv=bv)
        want = np.array([case["expect"][str(v)] for v in ints], dtype=np.float64)
        assert got.tobytes() == want.tobytes(), (case["name"], got, want)
    a, b = (bv[v] for v in g["gated_pair"])
    assert a.intersection_size(b) == g["gated_pair_exact_intersection"] > 0  # a non-empty intersection ...
    assert 4 * a.intersect_ones(b) < max(a.ones, b.ones) and a.sim(b) == 0.0  # ... that the bloom gate zeroes
    assert bv[103].ones == 2 and len(bv[103].ranks) == 3  # 1 and 65 share a bit
    assert bv[1].sqrt_len == 0.0 and bv[100].sim(bv[1]) == 0.0  # no in-links


def test_bloom_fold_identity():
    """word = h % 16 and bit = h % 64 of one product: the word is determined by the bit, the 16 words fold into one u64 with the same
    ones and the same intersections"""
    rng = np.random.default_rng(3)
    vecs = [sref.BitVec(int(x) | (int(y) << 64) for x, y in zip(rng.integers(0, 1 << 63, k), rng.integers(0, 1 << 20, k))) for k in (0, 1, 5, 40, 300, 2000)]
    for x in rng.integers(0, 1 << 63, 1000).tolist():
        a, b = sref.bloom_hash(x)
        assert a == b % 16
    for v in vecs:
        m = v.fold()
        assert bin(m).count("1") == v.ones
        assert m == sum(1 << p for p in {sref.bloom_hash(r)[1] for r in v.ranks})
        for w in vecs:
            assert bin(m & w.fold()).count("1") == v.intersect_ones(w)


def test_integer_gate_is_the_ratio_test():
    for m in range(1, 1025):
        for i in range(0, m + 1):
            assert (float(i) / float(m) < 0.25) == (4 * i < m), (i, m)


def test_numpy_form_equals_the_literal_one():
    g, gold = _golden()
    cases = [(gold, [100, 101, 100, 7], [101, 999], True, 0.25), (gold, [100], [], False, 1.0), (gold, [], [102, 100], False, 1.0)]
    lcg = graphs.dense_from_tuples(graphs.lcg_graph())
    cases += [(lcg, list(range(1, 40)) + [5, 1 << 70], [5, 9, 300], n, s) for n, s in ((False, 1.0), (True, 0.5))]
    tail = graphs.dense_from_tuples([(f, t) for f, t, _ in graphs.tailed_graph()])
    tids = sref.id_ints(tail[0])
    cases += [(tail, tids[:20], tids[10:13], True, 1.0)]
    for (ids, row_ptr, src), liked, disliked, normalized, ss in cases:
        a = sref.literal(ids, row_ptr, src, liked, disliked, normalized, ss)
        b = sref.numpy_scores(ids, row_ptr, src, liked, disliked, normalized, ss)
        assert a.tobytes() == b.tobytes()
        bv = sref.bitvecs(ids, row_ptr, src)
        length, bloom, _ = sref.numpy_state(ids, row_ptr, src)
        ints = sref.id_ints(ids)
        assert [int(x) for x in bloom] == [bv[v].fold() for v in ints] and [int(x) for x in length] == [len(bv[v].ranks) for v in ints]


def test_top_order():
    ids = graphs.dense_from_tuples([(1, 2), (2, 3), (3, 4)])[0]
    order = sref.top_order(ids, [0.5, 0.0, 0.5, 1.0], 10, skip=[4])
    assert order == [(0.5, 3), (0.5, 1), (0.0, 2)]
