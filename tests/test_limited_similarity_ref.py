"""The host restatement of the limited inbound similarity (tests/limited_similarity_ref.py) against values worked out by hand
(tests/golden/limited_similarity_cases.json), and its numpy form against the literal one.  No GPU."""
import json
import os

import numpy as np

from tests import graphs
from tests import inbound_similarity_ref as sref
from tests import limited_similarity_ref as lref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "limited_similarity_cases.json")


def test_golden_values():
    with open(GOLDEN) as f:
        g = json.load(f)
    graph = graphs.dense_from_tuples([tuple(e) for e in g["edges"]])
    ints = sref.id_ints(graph[0])
    for case in g["cases"]:
        keys = [tuple(k) for k in case["keys"]]
        bv = lref.bitvecs(*graph, keys, case["limit"])
        got = lref.literal(*graph, keys, case["limit"], case["liked"], case["disliked"], case["normalized"], case["self_score"], bv=bv)
        want = np.array([case["expect"].get(str(v), case["rest"]) for v in ints], dtype=np.float64)
        assert got.tobytes() == want.tobytes(), (case["name"], got, want)
        assert {str(v): len(bv[v].ranks) for v in ints if len(bv[v].ranks)} == case["len"], case["name"]


def test_numpy_form_equals_the_literal_one():
    """on the LCG graph with a few self links added, with and without keys (equal keys among them), for limits below, at and above the
    in-degrees, and for limit 0"""
    tuples = graphs.lcg_graph() + [(v, v) for v in (3, 50, 120, 199)]
    graph = graphs.dense_from_tuples(tuples)
    ids = graph[0]
    ints = sref.id_ints(ids)
    indeg = np.diff(np.asarray(graph[1], dtype=np.int64))
    assert indeg.max() > 8 > indeg.min()
    key_sets = ([], [(v, (v * 7919) % 13) for v in ints[::2]] + [(1 << 80, 0)])
    liked, disliked = ints[:20] + [3, 1 << 70], [5, 50, 300]
    for keys in key_sets:
        kb = lref.key_by_sid(ids, keys)
        for limit in (0, 1, 2, 5, int(indeg.max()), 1024):
            bv = lref.bitvecs(*graph, keys, limit)
            cut = lref.cut_graph(*graph, kb, limit)
            for normalized, ss in ((False, 1.0), (True, 0.5)):
                a = lref.literal(*graph, keys, limit, liked, disliked, normalized, ss, bv=bv)
                b = lref.numpy_scores(cut, liked, disliked, normalized, ss)
                assert a.tobytes() == b.tobytes(), (limit, normalized)
            last = (liked + disliked)[16:]
            counts, bloom, length = lref.numpy_export(cut, last)
            assert np.array_equal(counts, sref.counts(bv, ids, last)), limit
            assert [int(x) for x in bloom] == [bv[v].fold() for v in ints] and [int(x) for x in length] == [len(bv[v].ranks) for v in ints]
            if limit:
                assert int(length.max()) <= limit and all(v not in bv[v].ranks for v in ints)  # cut, and no self link left
    # the keys matter: some cut list differs between the two key sets
    a = lref.cut_graph(*graph, lref.key_by_sid(ids, key_sets[0]), 2)
    b = lref.cut_graph(*graph, lref.key_by_sid(ids, key_sets[1]), 2)
    assert np.array_equal(a[1], b[1]) and not np.array_equal(np.sort(a[2]), np.sort(b[2]))
