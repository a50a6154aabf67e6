"""Pins of tests/ampc_ref.py (the restatement the GPU tests of the AMPC value tables compare with) from answers the reference
itself holds: the expected values of its own unit tests, and hand-written cases of what its operators do at the IEEE corners
(tests/golden/ampc_value_cases.json).  No GPU."""
import json
import math
import os
import struct

import numpy as np

from tests import ampc_ref as ref

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ampc_value_cases.json")
OPS = {"U64_ADD": ref.U64_ADD, "U64_MIN": ref.U64_MIN, "F32_ADD": ref.F32_ADD, "F64_ADD": ref.F64_ADD, "KAHAN_ADD": ref.KAHAN_ADD}


def load_cases():
    with open(CASES) as f:
        return json.load(f)["cases"]


def model_value(kind, v):
    """a value of the JSON file as the model keeps it"""
    if kind == "U64":
        return int(v)
    if kind == "F32":
        return np.float32(float(v))
    if kind == "F64":
        return float(v)
    return (float(v[0]), float(v[1]))


def bits(kind, v):
    """the bit pattern of a model value as the JSON file writes it; any NaN is "nan" (neither IEEE 754 nor Rust fixes a NaN's sign
    and payload, and the model's are the host CPU's)"""
    if kind == "U64":
        return "0x%016x" % v
    if kind == "KAHAN":
        return [bits("F64", v[0]), bits("F64", v[1])]
    if math.isnan(float(v)):
        return "nan"
    if kind == "F32":
        return "0x%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0]
    return "0x%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def test_kahan_sum_of_the_reference_unit_test():
    # kahan_sum.rs:88-105
    k = ref.KAHAN_DEFAULT
    assert k[0] == 0.0
    for x in (10000.0, math.pi, math.e, math.pi, math.e, math.pi, math.e):
        k = ref.kahan_add(k, x)
    assert k[0] == 10017.579623446147


def test_dht_conn_unit_test():
    # dht_conn.rs:490-509: set, batch_set, upsert(U64Add), batch_upsert(U64Add)
    t = {}
    ref.batch_set(t, [0], [0])
    assert ref.batch_get(t, [0]) == [0]
    ref.batch_set(t, [1, 2], [0, 0])
    assert sorted(zip([1, 2], ref.batch_get(t, [1, 2]))) == [(1, 0), (2, 0)]
    assert ref.batch_upsert(t, ref.U64_ADD, [0], [1]) == [ref.MERGED]
    assert ref.batch_get(t, [0]) == [1]
    ref.batch_upsert(t, ref.U64_ADD, [1, 2], [1, 1])
    assert sorted(zip([0, 1, 2], ref.batch_get(t, [0, 1, 2]))) == [(0, 1), (1, 1), (2, 1)]
    assert ref.batch_get(t, [3]) == [None]


def test_hand_written_cases():
    cases = load_cases()
    # every corner the cases are there for is there
    names = " | ".join(c["name"] for c in cases)
    for word in ("NaN", "-0.0 + +0.0", "inf + -inf", "equal value", "wraps", "ignores new.err", "depends on the order"):
        assert word in names, word
    for c in cases:
        kind, op = c["kind"], OPS[c["op"]]
        t = {}
        ref.batch_set(t, [k for k, _ in c["stored"]], [model_value(kind, v) for _, v in c["stored"]])
        acts = ref.batch_upsert(t, op, [k for k, _ in c["batch"]], [model_value(kind, v) for _, v in c["batch"]])
        assert acts == c["actions"], c["name"]
        assert sorted(t) == sorted(k for k, _ in c["final"]), c["name"]
        for k, want in c["final"]:
            assert bits(kind, t[k]) == want, (c["name"], k)


def test_update_distances_takes_the_minimum_of_the_batch_first():
    # shortest_path/mapper.rs:70-81: two edges into one node in one batch give ONE upsert with the smaller distance
    prev, nxt = {1: 0, 2: 5}, {1: 0, 2: 5, 3: 9}
    keys, acts = ref.update_distances(prev, nxt, [(2, 3), (1, 3), (7, 4), (1, 2)])
    assert keys == [3, 2] and acts == [ref.MERGED, ref.MERGED]  # node 7 has no distance yet: its edge is skipped
    assert nxt == {1: 0, 2: 1, 3: 1}


def test_update_centralities_on_a_two_node_case():
    # mapper.rs:157-209: only nodes in both counter tables, only a growing size, the Kahan sum of prev + d / (round + 1), a set
    a, b = ref.hll_of(1), ref.hll_of(1)
    for x in range(2, 30):
        ref.hbo.hll_add(b, x)
    sa, sb = (int(s) for s in ref.hbo.hll_sizes(np.stack([a, b])))
    assert sb > sa
    prev_c, next_c = {1: a, 2: b, 3: a}, {1: b, 2: a, 4: b}
    prev_v, next_v = {1: (1.0, 0.0)}, {2: (9.0, 0.0)}
    assert ref.update_centralities(prev_c, next_c, prev_v, next_v, [1, 2, 3, 4, 1], 1) == 1
    assert next_v == {1: ref.kahan_add((1.0, 0.0), (sb - sa) / 2.0), 2: (9.0, 0.0)}  # 2 shrank (saturating), 3 and 4 are in one table only
