"""The restatement of hb_score_hosts (tests/score_hosts_ref.py) against the hand-written cases of tests/golden/score_hosts_cases.json,
and its numpy form against its literal form.  No GPU.

The expected values of the golden file were written out term by term (count / (sqrt(len_a) x sqrt(len_v)), sums from +0.0 in caller
order, D + (sum_liked - sum_disliked)); the grouping and the order case carry their terms, and the tests below show that the other
grouping / the other order gives other bits - so neither case can turn vacuous."""
import json
import math
import os

import numpy as np

from tests import graphs
from tests import limited_similarity_ref as lref
from tests import score_hosts_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_hosts_cases.json")


def load():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g, graphs.dense_from_tuples([tuple(e) for e in g["edges"]])


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _term(count, la, lv):
    return float(count) / (math.sqrt(float(la)) * math.sqrt(float(lv)))


def test_golden_cases_through_the_literal_form():
    g, graph = load()
    bv = ref.tables(*graph, [], 512)
    names = {c["name"] for c in g["cases"]}
    assert {"grouping", "order", "normalised with L = 0", "negative s", "self on the liked side", "self on the disliked side", "self on both sides",
            "custom self score", "unknown node equal to an unknown anchor", "gated pair with a common in-neighbour"} <= names
    for case in g["cases"]:
        (got,), st = ref.literal(bv, [case])
        assert np.array_equal(_bits(got), _bits(case["expect"])), (case["name"], got, case["expect"])
        assert [st[k] for k in ref.CLASSES] == case["classes"], case["name"]
        assert st["pairs"] == sum(case["classes"]) == (len(case["liked"]) + len(case["disliked"])) * len(case["nodes"])
    (all_at_once, st) = ref.literal(bv, g["cases"])
    assert [a.tobytes() for a in all_at_once] == [np.array(c["expect"], dtype=np.float64).tobytes() for c in g["cases"]]
    assert st["requests"] == len(g["cases"]) and st["unknown_anchors"] == 1 and st["unknown_nodes"] == 2


def test_the_grouping_case_tells_the_two_groupings_apart():
    g, _ = load()
    case = next(c for c in g["cases"] if c["name"] == "grouping")
    sl = sum((_term(*t) for t in case["terms_liked"]), 0.0)
    sd = sum((_term(*t) for t in case["terms_disliked"]), 0.0)
    d = float(len(case["disliked"]))
    assert d + (sl - sd) != (d + sl) - sd
    assert case["expect"] == [d + (sl - sd)]


def test_the_order_case_tells_two_orders_apart():
    g, graph = load()
    case = next(c for c in g["cases"] if c["name"] == "order")
    terms = [_term(*t) for t in case["terms_liked"]]
    other = [terms[i] for i in case["other_order"]]
    assert sum(terms, 0.0) != sum(other, 0.0)
    assert case["expect"] == [sum(terms, 0.0)]
    # the other order is the ascending-NodeID one: a sum in slot order instead of caller order answers with it
    assert [case["liked"][i] for i in case["other_order"]] == sorted(case["liked"])


def test_the_negative_case_is_negative_before_the_clamp():
    g, _ = load()
    case = next(c for c in g["cases"] if c["name"] == "negative s")
    assert case["raw"] < 0.0 and case["expect"] == [0.0]


def test_numpy_form_equals_the_literal_form():
    g, graph = load()
    cut = lref.cut_graph(*graph, None, 512)
    a, sa = ref.literal(ref.tables(*graph, [], 512), g["cases"])
    b, sb = ref.numpy_form(cut, g["cases"])
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b] and sa == sb
    # a graph with cuts, keys, self links, unknown ids and duplicates
    t = graphs.lcg_graph() + [(v, v) for v in (3, 50, 120)]
    graph = graphs.dense_from_tuples(t)
    ints = ref.sref.id_ints(graph[0])
    keys = [(v, (v * 7) % 5) for v in ints[::2]]
    reqs = [dict(liked=ints[:6] + [ints[2], 1 << 70], disliked=[ints[9], 3], nodes=ints[::9] + [1 << 70, 1 << 71, 3, 3], normalized=True),
            dict(liked=[], disliked=[50], nodes=[50, 51], self_score=2.5),
            dict(liked=ints[20:23], nodes=[]),
            dict(nodes=ints[:4])]
    for limit in (2, 5, 512):
        a, sa = ref.literal(ref.tables(*graph, keys, limit), reqs)
        b, sb = ref.numpy_form(lref.cut_graph(*graph, lref.key_by_sid(graph[0], keys), limit), reqs)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b], limit
        assert sa == sb, limit
        c, sc = ref.numpy_form(ref.cut_for(*graph, lref.key_by_sid(graph[0], keys), limit, reqs), reqs)  # the lists of the named hosts alone
        assert [x.tobytes() for x in a] == [x.tobytes() for x in c] and sa == sc, limit
        assert sa["pairs"] == sum(sa[k] for k in ref.CLASSES)
