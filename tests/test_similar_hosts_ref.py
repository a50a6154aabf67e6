"""tests/similar_hosts_ref.py against answers written by hand (tests/golden/similar_hosts_cases.json), its numpy form against its literal
form, and the reference's own it_favors_liked_hosts graph: the restatement tests/test_similar_hosts.py measures hb_similar_hosts with is
checked before it is used.  CPU only."""
import json
import math
import os

import numpy as np

from tests import graphs
from tests import links_ref as lref
from tests import similar_hosts_ref as sref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similar_hosts_cases.json")


def _doc():
    with open(GOLDEN) as f:
        return json.load(f)


def test_literal_against_hand_made_answers():
    doc = _doc()
    graph = graphs.dense_from_tuples([tuple(e) for e in doc["edges"]])
    got = sref.literal(*graph, [], doc["liked"], 1024)
    assert (got["nb"], got["apply"], got["bound"], got["taken"]) == (doc["nb"], doc["apply"], doc["bound"], doc["taken"])
    assert [list(e) for e in got["candidates"]] == doc["candidates"]
    assert (got["forward_entries"], got["distinct_targets"]) == (doc["forward_entries"], doc["distinct_targets"])
    terms = [t for v in doc["order"] for t in doc["terms"][str(v)]]
    assert (got["gated"], got["intersected"]) == (sum(1 for t in terms if t == 0), sum(1 for t in terms if t != 0))
    score = {}
    for v, terms in doc["terms"].items():
        s = 0.0
        for t in terms:
            s += 0.0 if t == 0 else float(t[0]) / (math.sqrt(float(t[1])) * math.sqrt(float(t[2])))
        score[int(v)] = max(s / float(doc["N"]), 0.0)
    assert [v for v, _ in got["top"]] == doc["order"]
    assert [s for _, s in got["top"]] == [score[v] for v in doc["order"]]
    assert score[22] == score[24] and score[23] == 0.0 and score[20] > score[21] > score[22] > 0.0
    for k in (1, 4, 5, 6):  # k below, at and above the candidate count
        assert [v for v, _ in sref.literal(*graph, [], doc["liked"], k)["top"]] == doc["order"][:k]
    # a duplicate counts in N and in the sum, an unknown id in N only
    single = dict(sref.literal(*graph, [], [10], 1024)["top"])
    double = dict(sref.literal(*graph, [], [10, 10, 99], 1024)["top"])
    assert double[20] == (single[20] + single[20]) / 3.0


def test_the_references_own_graph_keeps_e_above_d():
    fav = _doc()["favors_liked"]
    graph = graphs.dense_from_tuples([tuple(e) for e in fav["edges"]])
    top = sref.literal(*graph, [], fav["liked"], 1024)["top"]
    score = dict(top)
    assert fav["e"] in score and score[fav["e"]] > score.get(fav["d"], 0.0)
    assert [v for v, _ in top][0] == fav["e"]


def test_numpy_form_equals_the_literal_one():
    tuples = graphs.lcg_graph() + [(7, 7), (9, 9)]
    graph = graphs.dense_from_tuples(tuples)
    nodes = lref.id_ints(graph[0])
    n = len(nodes)
    state = sref.numpy_state(*graph)
    for mod in (3, 1 << 40):
        key = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) % np.uint64(mod)
        keys = [(nodes[i], int(key[i])) for i in range(n)]
        for liked in ([5], [17, 100, 17, 4242], nodes[:40], nodes[3:9] + [nodes[3]]):
            for k in (1, 50, 1024):
                want = sref.literal(*graph, keys, liked, k)
                got = sref.numpy_form(state, key, liked, k)
                assert got["candidates"] == want["candidates"] and (got["nb"], got["apply"], got["bound"], got["taken"]) == (
                    want["nb"], want["apply"], want["bound"], want["taken"])
                assert [v for v, _ in got["top"]] == [v for v, _ in want["top"]]
                assert [s for _, s in got["top"]] == [s for _, s in want["top"]]
                assert all(got[f] == want[f] for f in ("forward_entries", "distinct_targets", "gated", "intersected"))
