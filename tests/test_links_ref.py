"""tests/links_ref.py against hand-made answers (tests/golden/links_cases.json), and its numpy form against its literal form on the LCG
graph the other operators' tests use.  CPU only: these are the references tests/test_links.py holds hb_backlinks to."""
import json
import os

import numpy as np

from tests import graphs
from tests import links_ref as lref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "links_cases.json")


def _hash64(salt, nodes):
    m = (1 << 64) - 1
    out = []
    for v in nodes:
        z = (int(v) * 0x9E3779B97F4A7C15 + (int(salt) + 1) * 0xD1B54A32D192ED03) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        out.append(z ^ (z >> 31))
    return out


def test_literal_form_against_hand_made_answers():
    with open(GOLDEN) as f:
        gold = json.load(f)
    graph = graphs.dense_from_tuples([tuple(e) for e in gold["edges"]])
    assert lref.id_ints(graph[0]) == [1, 2, 3, 4, 5, 6]
    keys = [tuple(k) for k in gold["keys"]]
    key_of = {int(v): int(k) for v, k in gold["key_of"].items()}
    assert key_of[4] == lref.U64_MAX and key_of[2] == key_of[3]  # a missing key, equal keys
    assert len(gold["queries"]) != len(set(gold["queries"]))  # a duplicate query
    for case in gold["cases"]:
        lists, degrees, unknown_keys, unknown = lref.literal(*graph, keys, gold["queries"], case["limit"], case["keep_self"])
        assert [[u for u, _ in lst] for lst in lists] == case["lists"], case
        assert [[k for _, k in lst] for lst in lists] == [[key_of[u] for u in lst] for lst in case["lists"]], case
        assert degrees == case["degrees"], case
        assert unknown_keys == gold["unknown_keys"] and unknown == gold["unknown_queries"]
    limits = [c["limit"] for c in gold["cases"] if not c["keep_self"]]
    assert 1 in limits and 2 in limits and max(limits) > max(gold["cases"][0]["degrees"])  # L = 1, 2 and L above the degree


def test_numpy_form_equals_the_literal_form_on_the_lcg_graph():
    tuples = graphs.lcg_graph() + [(7, 7), (50, 50), (199, 199)]  # and three self links
    ids, row_ptr, src = graphs.dense_from_tuples(tuples)
    nodes = lref.id_ints(ids)
    n = len(nodes)
    rng = np.random.default_rng(3)
    for salt, listed in ((0, n), (1, n - 40), (2, 0)):
        key = np.full(n, lref.U64_MAX, dtype=np.uint64)
        pick = np.sort(rng.choice(n, listed, replace=False))
        hashed = [k % 11 if salt else k for k in _hash64(salt, nodes)]  # salt 1: ties all over
        key[pick] = np.array([hashed[i] for i in pick.tolist()], dtype=np.uint64)
        keys = [(nodes[i], int(key[i])) for i in pick.tolist()]
        qs = np.concatenate((np.arange(n), rng.integers(0, n, 30)))  # every node, and duplicates
        for limit in (1, 2, 5, 6, 7, 1024):
            for keep_self in (False, True):
                lists, degrees, _, unknown = lref.literal(ids, row_ptr, src, keys, [nodes[i] for i in qs.tolist()], limit, keep_self)
                off, frm, k, deg = lref.numpy_form(row_ptr, src, key, qs, limit, keep_self)
                assert unknown == 0 and deg.tolist() == degrees
                assert np.diff(off).tolist() == [len(lst) for lst in lists]
                assert [nodes[i] for i in frm.tolist()] == [u for lst in lists for u, _ in lst]
                assert k.tolist() == [kk for lst in lists for _, kk in lst]
    assert max(degrees) > 7 > min(degrees)  # the limits above cut some lists and not others
