"""The restatement tests/nearest_seed_ref.py against hand-written answers (tests/golden/nearest_seed_cases.json): a copy (0.0 included),
a first backlink without a value while the second has one, a self link skipped, a tie, a key of u64::MAX, duplicates in the orig list,
unknown ids, rounds on a chain - and its numpy form against the literal one."""
import json
import os

import numpy as np
import pytest

from tests import graphs
from tests import nearest_seed_ref as nref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nearest_seed_cases.json")
with open(GOLDEN) as f:
    CASES = json.load(f)["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hand_written_answers(case):
    graph = graphs.dense_from_tuples([tuple(e) for e in case["edges"]])
    seeds, values, stats = nref.literal(*graph, [tuple(e) for e in case["orig"]], [tuple(e) for e in case["keys"]], case["discount"], case["rounds"])
    assert seeds == {int(k): v for k, v in case["seeds"].items()}
    want = {int(k): float(v) for k, v in case["values"].items()}
    assert set(values) == set(want)
    assert {k: np.float64(v).view(np.uint64) for k, v in values.items()} == {k: np.float64(v).view(np.uint64) for k, v in want.items()}
    assert stats == case["stats"]


def test_every_rule_has_a_case():
    names = " / ".join(c["name"] for c in CASES)
    for rule in ("0.0 included", "second has one", "self link", "tie", "u64::MAX", "duplicates", "unknown ids", "rounds = 3"):
        assert rule in names, rule


def test_top_order_breaks_ties_by_ascending_node():
    assert nref.top_order({5: 0.5, 3: 0.5, 9: 0.75, 4: 0.0}, 3) == [(9, 0.75), (3, 0.5), (5, 0.5)]


@pytest.mark.parametrize("rounds,discount", [(1, 0.5), (2, 0.3), (255, 0.5), (3, 0.0)])
def test_numpy_form_is_the_literal_one(rounds, discount):
    ids, row_ptr, src = graphs.dense_from_tuples(graphs.lcg_graph())
    nodes = nref.id_ints(ids)
    n = len(nodes)
    rng = np.random.default_rng(rounds)
    key_by_sid = rng.integers(0, 4, n, dtype=np.uint64)  # many ties
    key_by_sid[::9] = np.uint64(nref.U64_MAX)
    orig_sids = list(range(0, n, 7)) + [0, 7]
    orig_vals = [float(v) for v in rng.random(len(orig_sids))]
    seeds, values, stats = nref.literal(ids, row_ptr, src, [(nodes[s], v) for s, v in zip(orig_sids, orig_vals)],
                                        [(nodes[s], int(k)) for s, k in enumerate(key_by_sid.tolist()) if k != nref.U64_MAX], discount, rounds)
    seed, val, has, filled, rounds_run = nref.numpy_form(ids, row_ptr, src, orig_sids, orig_vals, key_by_sid, discount, rounds)
    assert {nodes[v]: nodes[int(s)] for v, s in enumerate(seed) if s >= 0} == seeds
    assert {nodes[v]: np.float64(val[v]).view(np.uint64) for v in np.flatnonzero(has)} == {k: np.float64(v).view(np.uint64) for k, v in values.items()}
    assert filled == stats["filled"] and rounds_run == stats["rounds_run"]
