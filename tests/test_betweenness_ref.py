"""The two host restatements of Betweenness::calculate in tests/betweenness_ref.py agree with each other and with the reference's own
known answer (no GPU)."""
import json
import os

import numpy as np

from tests import betweenness_ref as bref
from tests import graphs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "betweenness_cases.json")


def _csr(tuples):
    """(n, row_ptr, src) by destination over the distinct edges, node k = the k-th smallest id"""
    ids = sorted({a for a, _ in tuples} | {b for _, b in tuples})
    at = {v: i for i, v in enumerate(ids)}
    edges = sorted({(at[b], at[a]) for a, b in tuples})
    n = len(ids)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    for dst, _ in edges:
        row_ptr[dst + 1] += 1
    return ids, n, np.cumsum(row_ptr), np.array([s for _, s in edges], dtype=np.int64)


def test_known_answer_of_the_reference():
    with open(GOLDEN) as f:
        case = json.load(f)["cases"][0]
    nid = case["nodes"]
    ids, n, row_ptr, src = _csr([(nid[a], nid[b]) for a, b in case["edges"]])
    for fn in (bref.literal, bref.numpy):
        res = fn(n, row_ptr, src, range(n))
        vals = res.values()
        assert {k: vals[ids.index(v)] for k, v in nid.items()} == case["expect"]
        assert res.max_dist == case["max_dist"]


def test_the_two_restatements_agree():
    for tuples, srcs in ((graphs.lcg_graph(), None), (graphs.lcg_graph(n=600, m=700, seed=5), None), (graphs.lcg_graph(n=150, m=500, seed=9), [0, 3, 77])):
        ids, n, row_ptr, src = _csr([(a, b) for a, b, *_ in tuples])
        srcs = range(n) if srcs is None else srcs
        a, b = bref.literal(n, row_ptr, src, srcs), bref.numpy(n, row_ptr, src, srcs)
        tol = bref.rtol(n, row_ptr, src, a)
        assert a.max_dist == b.max_dist and np.array_equal(a.reached, b.reached)
        for k in range(len(a.sources)):
            assert np.array_equal(a.dist[k], b.dist[k])
            assert [int(x) for x in b.sigma[k]] == a.sigma[k]
            assert np.allclose(a.delta[k], b.delta[k], rtol=tol, atol=0.0)
        assert np.allclose(a.sums, b.sums, rtol=tol, atol=0.0)
        assert np.array_equal(a.sums == 0.0, b.sums == 0.0)


def test_diamond_chain_counts_are_integers():
    k = 60
    t = []
    for i in range(k):
        a, d = 1 + 3 * i, 4 + 3 * i
        t += [(a, a + 1), (a, a + 2), (a + 1, d), (a + 2, d)]
    ids, n, row_ptr, src = _csr(t)
    for fn in (bref.literal, bref.numpy):
        res = fn(n, row_ptr, src, [0])
        assert int(res.sigma[0][n - 1]) == 2 ** k and res.max_dist == 2 * k
