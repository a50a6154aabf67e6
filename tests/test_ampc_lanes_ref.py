"""tests/ampc_lanes_ref.py against answers derived by hand and against the per-source models it batches (tests/ampc_round_ref.py,
tests/ampc_approx_ref.py): the model the GPU tests of tests/test_ampc_lanes.py compare with must itself be right, and the claim the lane
tables rest on - the batched job returns, bit for bit, what the per-source job returns - must hold in the models first.  No GPU."""
import math

import numpy as np
import pytest

from tests import ampc_approx_ref as aref
from tests import ampc_lanes_ref as lref
from tests import ampc_round_ref as rref
from tests.test_ampc_round import two_workers
from tests.test_ampc_values import harmonic_graphs

INF, NAN_BITS = math.inf, 0x7FF8000000000000
NONE = lref.NONE


def workers_of(which):
    edges = dict(harmonic_graphs())[which]
    if which == "rmat":
        edges = edges[:600]
    sink = (1 << 90) | 5
    edges = edges + [(edges[0][0], sink), (edges[-1][0], sink)]
    nodes = sorted({x for e in edges for x in e})
    return two_workers(edges, nodes), nodes, sink


def bits_of(result):
    return {k: aref.bits(v) for k, v in result.items()}


@pytest.mark.parametrize("which", ["fixture", "rmat"])
def test_model_batched_job_equals_the_per_source_job(which):
    """batch sizes 1, 2, 3 and 64 over 67 sources (a sink, a source twice within a batch and in two batches): after every batch every lane
    equals the per-source job's table, at the end the centralities equal the per-source job's bit for bit"""
    workers, nodes, sink = workers_of(which)
    rng = np.random.default_rng(3)
    sources = [nodes[int(i)] for i in rng.integers(0, len(nodes), 67)]
    sources[1], sources[2], sources[5], sources[66] = sink, sources[0], sources[0], sources[0]
    for max_distance in (1, 7):
        per_source = {s: aref.run_job(rref.shortest_path_job(workers, s, max_distance)) for s in set(sources)}
        want = aref.run_job(aref.approx_harmonic_job(workers, sources, 2658, max_distance))
        for k in (1, 2, 3, 64):
            job = lref.approx_harmonic_job(workers, sources, 2658, max_distance, k)
            seen = 0
            while True:
                try:
                    _, _, _, table, batch = next(job)
                except StopIteration as done:
                    got = done.value
                    break
                assert batch == sources[seen:seen + k]
                for lane, s in enumerate(batch):
                    assert lref.lane_of(table, lane) == per_source[s], (k, seen, lane)
                for lane in range(len(batch), lref.LANES):
                    assert lref.lane_of(table, lane) == {}
                seen += len(batch)
            assert seen == len(sources)
            assert got.keys() == want.keys() and bits_of(got) == bits_of(want), (which, max_distance, k)


def test_path_graph_by_hand():
    """a -> b -> c with sources [a, b] in one batch: lanes {a: [0, -], b: [1, 0], c: [2, 1]}; num_samples = 3 is norm = 1/2: a = inf,
    b = 1/2 then inf (err NaN), c = 1/4 + 1/2 - tests/test_ampc_approx_ref.py's answers"""
    a, b, c = 10, 20 | (1 << 64), 30
    workers = [([a, b], [(a, b)]), ([c], [(b, c)])]
    table = aref.run_job(lref.shortest_paths_job(workers, [a, b], 5))
    assert {k: r[:2].tolist() for k, r in table.items()} == {a: [0, NONE], b: [1, 0], c: [2, 1]}
    assert all((r[2:] == NONE).all() for r in table.values())
    job = lref.approx_harmonic_job(workers, [a, b], 3, 5, 2)
    cent, folded, inserted, _, _ = next(job)
    assert (folded, inserted) == (5, 3)
    assert {n: aref.kahan_bits(k) for n, k in cent.items()} == {a: aref.kahan_bits((INF, 0.0)), b: (aref.bits(INF), NAN_BITS), c: aref.kahan_bits((0.75, 0.0))}
    assert aref.run_job(job) == {a: INF, b: INF, c: 0.75}
    assert aref.run_job(lref.approx_harmonic_job(workers, [a, b], 3, 5, 2, skip_zero=True)) == {b: 0.5, c: 0.75}
    assert aref.run_job(lref.approx_harmonic_job(workers, [a, b], 3, 1, 2, skip_zero=True)) == {b: 0.5, c: 0.5}
    # one round of the first table by hand: a's row reaches b, b's own lane stays 0
    prev = lref.first_table([a, b])
    nxt = {k: r.copy() for k, r in prev.items()}
    changed = rref.Exact([a, b])
    assert lref.round_lane_distances(prev, nxt, [(a, b), (b, c)], changed) == (2, 1, 1)
    assert nxt[b][:2].tolist() == [1, 0] and nxt[c][:2].tolist() == [NONE, 1]


def test_saturation():
    """253 + 1 = 254, 254 + 1 = none, none stays; a candidate row without a lane is NoChange on a present key and Inserted on an absent one"""
    assert lref.step(lref.row({0: 253, 1: 254, 2: 0, 63: 7})).tolist() == lref.row({0: 254, 2: 1, 63: 8}).tolist()
    assert lref.step(lref.row()).tolist() == lref.row().tolist()
    table = {1: lref.row({0: 5})}
    none = lref.step(lref.row({3: 254}))
    assert (none == NONE).all()
    assert lref.batch_upsert(table, [1, 2], [none, none]) == [lref.NO_CHANGE, lref.INSERTED]
    assert table[1].tolist() == lref.row({0: 5}).tolist() and (table[2] == NONE).all()
    # the actions of the operator: an equal row, one byte lower, one byte higher, a fresh key; pairs of one key apply in order
    assert lref.batch_upsert(table, [1, 1, 1, 9, 1], [lref.row({0: 5}), lref.row({0: 4}), lref.row({0: 6}), lref.row({1: 1}), lref.row({0: 4, 9: 0})]) == [
        lref.NO_CHANGE, lref.MERGED, lref.NO_CHANGE, lref.INSERTED, lref.MERGED]
    assert table[1].tolist() == lref.row({0: 4, 9: 0}).tolist()
    rows, found = lref.batch_get(table, [1, 77])
    assert found == [True, False] and (rows[1] == NONE).all()
    # the fold ignores lanes at or above n_lanes and lanes without a distance; a key with nothing to fold is not inserted
    cent = {}
    assert lref.fold_lanes(cent, {5: lref.row({0: 254, 2: 0, 3: 1}), 6: lref.row({2: 0}), 7: lref.row({3: 4})}, 1.0, 3, skip_zero=True) == (1, 1)
    assert cent == {5: (1.0 / 254.0, 0.0)}


def test_a_source_listed_twice():
    """two lanes of one source hold the same distances, the first table has ONE row for it with two zeros, and its term is folded twice"""
    a, b = 10, 20
    workers = [([a, b], [(a, b)])]
    first = lref.first_table([a, b, a])
    assert sorted(first) == [a, b] and first[a][:3].tolist() == [0, NONE, 0] and first[b][:3].tolist() == [NONE, 0, NONE]
    table = aref.run_job(lref.shortest_paths_job(workers, [a, b, a], 5))
    assert lref.lane_of(table, 0) == lref.lane_of(table, 2) == {a: 0, b: 1} and lref.lane_of(table, 1) == {b: 0}
    got = aref.run_job(lref.approx_harmonic_job(workers, [a, b, a], 5, 5, 3, skip_zero=True))
    assert got == aref.run_job(aref.approx_harmonic_job(workers, [a, b, a], 5, 5, skip_zero=True)) == {b: 0.5}


def test_contraction_fixture_as_six_lanes():
    """the contraction case of tests/ampc_approx_ref.py as six lanes of one row: the same bits as six per-source folds"""
    norm = 1.0 / (aref.CONTRACTION_NUM_SAMPLES - 1)
    cent, want = {}, {}
    assert lref.fold_lanes(cent, {42: lref.row(dict(enumerate(aref.CONTRACTION_DISTANCES)))}, norm, 6) == (6, 1)
    for d in aref.CONTRACTION_DISTANCES:
        aref.fold(want, {42: d}, norm)
    assert cent == want and cent[42][1] == -(2.0 ** -65)
    # descending order is another sum
    down = {}
    for d in reversed(aref.CONTRACTION_DISTANCES):
        aref.fold(down, {42: d}, norm)
    assert aref.kahan_bits(down[42]) != aref.kahan_bits(cent[42])
