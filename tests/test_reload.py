"""A second (and third) load on a context that has used all five operators - hb_run, hb_sampled_harmonic, hb_distances, hb_betweenness,
hb_inbound_similarity.  Everything the first graph left on the context (device buffers, sizes, row indices, the sampler's candidates, the
operators' results) must be gone after hb_load_*: graph A is the larger one, so every size kept from it is too large for graph B and
every row index out of range.  The comparisons are the sibling tests' own (tests/test_gpu.py, test_sampled_harmonic.py,
test_distances.py, test_betweenness.py, test_similarity.py): bit-exact lists, equal distance arrays, betweenness within its rule."""
import functools

import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib
from stract_amd.harmonic import EdgeListGraph
from tests import distance_ref as dref
from tests import graphs
from tests import inbound_similarity_ref as sref
from tests import sample_ref as ref
from tests import test_betweenness as tb
from tests import test_distances as td
from tests import test_sampled_harmonic as ts
from tests import test_similarity as tsim

pytestmark = pytest.mark.gpu

GRAPHS = {"A": dict(n=300, m=2400, seed=7), "B": dict(n=70, m=300, seed=3)}
FRINGE = {"A_fringe": 70, "B_fringe": 9}  # the same two with so many hosts without an in-link behind them, two links each into the graph


@functools.lru_cache(maxsize=None)
def _tuples(name):
    base = GRAPHS[name[0]]
    fringe = [(1001 + d, 1 + (7 * d + k) % base["n"]) for d in range(FRINGE.get(name, 0)) for k in (0, 31)]
    return graphs.lcg_graph(**base) + fringe


@functools.lru_cache(maxsize=None)
def _edges(name):
    return EdgeListGraph.from_tuples(_tuples(name)).host_edges()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(ids, row_ptr, src) of the reduced graph and the oracle's HyperBall run on it: (passes, values, kept)"""
    ids, row_ptr, src = graphs.dense_from_tuples(_tuples(name))
    o = hbo.Dense(np.ascontiguousarray(ids["lo"]), row_ptr, src)
    T = o.run()
    vals, keep, _ = o.finish()
    return (ids, row_ptr, src), (T, vals, keep)


@functools.lru_cache(maxsize=None)
def _bitvecs(name):
    return sref.bitvecs(*_oracle(name)[0])


def _sources(row_ptr, src):
    """picked from the edge list: three sids with an out-edge (sampled), two of them (forward), two sids with an in-edge (reversed)"""
    has_out = np.unique(np.asarray(src, dtype=np.int64))
    has_in = np.flatnonzero(np.diff(np.asarray(row_ptr, dtype=np.int64)) > 0)
    assert len(has_out) >= 3 and len(has_in) >= 2
    return has_out[[0, len(has_out) // 2, -1]].tolist(), has_out[[1, -2]].tolist(), has_in[[0, -1]].tolist()


def _check_run(ctx, name):
    (ids, row_ptr, src), (T, vals, keep) = _oracle(name)
    got = ctx.graph()
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], row_ptr) and np.array_equal(got[2], src)
    st = ctx.run()
    gids, gvals = ctx.results()
    assert st["passes"] == T and keep.any()
    assert np.array_equal(gids, ids[keep])
    assert np.array_equal(gvals.view(np.uint64), vals[keep].view(np.uint64))


def _check_operators(ctx, name):
    _check_run(ctx, name)
    (ids, row_ptr, src), _ = _oracle(name)
    sampled, forward, backward = _sources(row_ptr, src)
    st, h_ref = ts._check(ctx, sources_sids=sampled)
    assert st["sources"] == 3 and h_ref.any()  # (somebody is within reach of the sources: the comparison is not one of empty lists)
    for srcs, reversed in ((forward, False), (backward, True)):
        st = td._check(ctx, srcs, reversed, modes=(None,), ref=dref.bfs)
        assert st["reached"] > len(srcs)
    res, _ = tb._check(ctx, sampled, modes=(None,))  # against tests/betweenness_ref.py
    assert res.reached.sum() > len(sampled)
    ints = sref.id_ints(ids)
    want, _ = tsim._check(ctx, (ids, row_ptr, src), _bitvecs(name), [ints[s] for s in sampled], [ints[s] for s in backward], modes=(None,))
    assert want.any()  # against tests/inbound_similarity_ref.py


def _refused(fn):
    with pytest.raises(_lib.HyperballError) as e:
        fn()
    assert e.value.code == _lib.HB_ERR_INVALID


@pytest.mark.parametrize("variant", ["default", "no_sparse", "live_first"])
def test_reload_after_all_five_operators(gpu_ctx_factory, variant):
    # no_sparse: hb_distances owns its transpose, the sampled operator takes the dense / bitmap modes
    # live_first: the live-first device order forced on, both graphs with hosts without an in-link behind them: n_live
    # and n_live_pad of A (300 and 320 of 370 rows) are too large for B (69 and 128 of 79 rows)
    flags = _lib.HB_FLAG_ALL_RELS | {"no_sparse": _lib.HB_FLAG_NO_SPARSE, "live_first": _lib.HB_FLAG_LIVE_FIRST}.get(variant, 0)
    A, B = ("A_fringe", "B_fringe") if variant == "live_first" else ("A", "B")
    live = {A: (True, 300, 320), B: (True, 69, 128)} if variant == "live_first" else None  # (one host of lcg70 has no in-link by itself)
    with gpu_ctx_factory(flags=flags) as ctx:
        ctx.load_edges(_edges(A))
        assert live is None and not ctx.plan_live()[0] or ctx.plan_live() == live[A]
        _check_operators(ctx, A)
        cand_a = td._ints(ctx.sample_sources(5, 10))

        ctx.load_edges(_edges(B))
        assert live is None and not ctx.plan_live()[0] or ctx.plan_live() == live[B]
        # nothing of A answers for B: no distances, no histogram, no betweenness, no scores, and the sampler draws from B's candidates
        _refused(ctx.distance_count)
        _refused(ctx.sample_histogram)
        _refused(ctx.betweenness_count)
        _refused(ctx.similarity_all)
        (ids, row_ptr, src), _ = _oracle(B)
        cand_b = td._ints(ctx.sample_sources(5, 10))
        assert cand_b == td._ints(ids[ref.sample_sids(len(ids), row_ptr, src, 5, 10)]) and cand_b != cand_a
        _check_operators(ctx, B)

        ctx.load_edges(_edges(A))  # (the allocator hands back memory B and the first A used)
        _check_run(ctx, A)
