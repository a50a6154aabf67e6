"""tests/forwardlinks_ref.py against answers written by hand (tests/golden/forwardlinks_cases.json), and its numpy form against its
literal form: the restatement tests/test_forwardlinks.py measures hb_forwardlinks with is checked before it is used.  CPU only."""
import json
import os

import numpy as np

from tests import forwardlinks_ref as fref
from tests import graphs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forwardlinks_cases.json")


def test_literal_against_hand_made_answers():
    with open(GOLDEN) as f:
        doc = json.load(f)
    graph = graphs.dense_from_tuples([tuple(e) for e in doc["edges"]])
    keys = [tuple(k) for k in doc["keys"]]
    assert len(doc["cases"]) == 4
    for case in doc["cases"]:
        lists, degrees, unknown_keys, unknown = fref.literal(*graph, keys, case["queries"], case["limit"], case["keep_self"])
        assert [[list(e) for e in lst] for lst in lists] == case["lists"], case
        assert degrees == case["degrees"] and unknown_keys == doc["unknown_keys"] and unknown == case["unknown"], case


def test_out_csr_is_the_transpose():
    ids, row_ptr, src = graphs.dense_from_tuples(graphs.lcg_graph() + [(7, 7), (9, 9)])
    out_ptr, dst = fref.out_csr(row_ptr, src)
    forward = {(u, int(v)) for u in range(len(ids)) for v in dst[out_ptr[u]:out_ptr[u + 1]]}
    backward = {(int(u), v) for v in range(len(ids)) for u in src[int(row_ptr[v]):int(row_ptr[v + 1])]}
    assert forward == backward and len(dst) == len(src) == len(forward)
    assert all(np.all(np.diff(dst[out_ptr[u]:out_ptr[u + 1]]) > 0) for u in range(len(ids)))


def test_numpy_form_equals_the_literal_one():
    graph = graphs.dense_from_tuples(graphs.lcg_graph() + [(7, 7), (9, 9), (1000, 1)])  # two self links, a node without in-links
    nodes = fref.id_ints(graph[0])
    n = len(nodes)
    out_ptr, dst = fref.out_csr(graph[1], graph[2])
    assert int(np.diff(out_ptr).max()) >= 9
    for mod in (3, 1 << 40):  # ties all over / hardly any
        key = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) % np.uint64(mod)
        key[::7] = fref.U64_MAX
        keys = [(nodes[i], int(key[i])) for i in range(n) if int(key[i]) != fref.U64_MAX]
        qsids = np.concatenate((np.arange(n), [6, 6, 8]))
        for limit in (1, 2, 5, 1024):
            for keep_self in (False, True):
                lists, degrees, _, _ = fref.literal(*graph, keys, [nodes[int(s)] for s in qsids], limit, keep_self)
                off, to, k, deg = fref.numpy_form(out_ptr, dst, key, qsids, limit, keep_self)
                assert deg.tolist() == degrees
                assert [[nodes[int(v)] for v in to[int(a):int(b)]] for a, b in zip(off[:-1], off[1:])] == [[v for v, _ in lst] for lst in lists]
                assert k.tolist() == [kk for lst in lists for _, kk in lst]
