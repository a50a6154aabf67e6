"""hb_betweenness (Betweenness::calculate, crates/core/src/webgraph/centrality/betweenness.rs:29-146) against the host restatement in
tests/betweenness_ref.py.

Comparison rule: dist, sigma, the result id set, max_dist and all counts are compared EXACTLY; a value the restatement gives as 0.0 must
be +0.0; every other delta / value within rtol = 4 * 2^-53 * (L (D + 4) + S + 3), computed per case from the graph (L = deepest level,
D = largest out-degree, S = sources; betweenness_ref.rtol says why)."""
import json
import math
import os

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import EdgeListGraph
from tests import betweenness_ref as bref
from tests import distance_ref as dref
from tests import graphs

pytestmark = pytest.mark.gpu

MODES = (None, "dense", "sparse")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "betweenness_cases.json")


def _ints(ids):
    return [int(i["lo"]) | (int(i["hi"]) << 64) for i in ids]


def _u128(ints):
    out = np.zeros(len(ints), dtype=_lib.U128)
    for i, v in enumerate(ints):
        out[i]["lo"] = v & 0xFFFFFFFFFFFFFFFF
        out[i]["hi"] = v >> 64
    return out


def _ctx(factory, graph, flags=_lib.HB_FLAG_ALL_RELS, **kw):
    ctx = factory(flags=flags, **kw)
    ctx.load_edges(graph.host_edges())
    return ctx


def _assert_close(got, want, tol, what):
    """the comparison rule for f64 arrays: same NaN / inf pattern, +0.0 where the restatement has 0.0, rtol elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    zero = want == 0.0
    assert not got[zero].view(np.uint64).any(), what  # +0.0, bit for bit
    rest = ~(np.isnan(want) | inf | zero)
    err = np.abs(got[rest] - want[rest]) / np.abs(want[rest])
    worst = float(err.max()) if err.size else 0.0
    print("%s: worst relative error %.3g, rtol %.3g" % (what, worst, tol))
    assert worst <= tol, (what, worst, tol)


def _compare(ctx, ids, res, tol, got, mode, raw=False, debug=True):
    got_ids, got_vals, st = got
    keep = res.reached
    S = len(res.sources)
    assert np.array_equal(got_ids, ids[keep]), mode
    _assert_close(got_vals, res.values(raw)[keep], tol, "values (%s)" % mode)
    allv = ctx.betweenness_all()
    assert np.array_equal(allv[~keep], np.full(int((~keep).sum()), -1.0))
    assert allv[keep].tobytes() == got_vals.tobytes()
    assert ctx.betweenness_count() == len(got_ids) == st["results"] == int(keep.sum())
    assert st["sources"] == S and st["batches"] == (S + 7) // 8 and st["max_dist"] == res.max_dist
    assert sum(st["levels_mode"]) == st["levels_forward"] and st["levels_backward"] >= st["batches"]
    if mode == "dense":
        assert st["levels_mode"][1] == 0 and st["levels_mode"][2] == 0
    if mode == "sparse":
        assert st["levels_mode"][0] == 0
    if debug and S:
        dist, sigma, delta = ctx.debug_betweenness_batch()
        first = (S - 1) // 8 * 8
        for lane in range(8):
            k = first + lane
            if k >= S:
                assert (dist[:, lane] == 255).all() and not sigma[:, lane].any() and not delta[:, lane].view(np.uint64).any()
                continue
            assert np.array_equal(dist[:, lane], np.where(res.dist[k] < 0, 255, res.dist[k]).astype(np.uint8)), (mode, k)
            assert [int(x) for x in sigma[:, lane]] == [int(x) for x in res.sigma[k]], (mode, k)
            _assert_close(delta[:, lane], res.delta[k], tol, "delta of source %d (%s)" % (k, mode))
    return st


def _check(ctx, source_sids=None, modes=MODES, graph=None, ref=bref.literal, debug=True):
    """the default run and the two forced modes against the restatement; returns (restatement, default run's stats)"""
    ids, row_ptr, src = graph if graph is not None else ctx.graph()
    n = len(ids)
    sids = list(range(n)) if source_sids is None else list(source_sids)
    res = ref(n, row_ptr, src, sids)
    tol = bref.rtol(n, row_ptr, src, res)
    sources = None if source_sids is None else ids[np.asarray(sids, dtype=np.int64)]
    stats = [_compare(ctx, ids, res, tol, ctx.betweenness(sources, mode=mode), mode, debug=debug) for mode in modes]
    return res, stats[0]


def _path(length):
    return EdgeListGraph.from_tuples([(i, i + 1) for i in range(1, length)])


def _star(leaves=100_000):
    """hub 1 has `leaves` in-edges, hub 2 has `leaves` out-edges, 1 -> 2 (tests/test_distances.py)"""
    t = [(v, 1) for v in range(3, leaves + 3)] + [(2, v) for v in range(3, leaves + 3)] + [(1, 2)]
    return EdgeListGraph.from_tuples(t)


def _diamonds(k):
    """a chain of k diamonds a -> {b, c} -> d: 2^k shortest paths from its first node to its last"""
    t = []
    for i in range(k):
        a, d = 1 + 3 * i, 4 + 3 * i
        t += [(a, a + 1), (a, a + 2), (a + 1, d), (a + 2, d)]
    return EdgeListGraph.from_tuples(t)


# (1) the reference's own known answer (betweenness.rs tests::path): every sum has one term, so the values are equal with ==
def test_reference_known_answer():
    from stract_amd.betweenness import Betweenness
    with open(GOLDEN) as f:
        case = json.load(f)["cases"][0]
    nid = case["nodes"]
    b = Betweenness.calculate(EdgeListGraph.from_tuples([(nid[a], nid[b]) for a, b in case["edges"]]))
    assert b.centrality == {nid[k]: v for k, v in case["expect"].items()}
    assert list(b.centrality) == sorted(b.centrality) and b.max_dist == case["max_dist"]


# (2) fixture graphs, every node a source, default and forced modes, the last batch's state
@pytest.mark.parametrize("name", ["fixture", "host_fixture", "lcg", "lcg_sparse"])
def test_fixture_graphs_all_sources(gpu_ctx_factory, name):
    g = {"fixture": graphs.fixture_graph, "host_fixture": lambda: graphs.host_fixture()[0], "lcg": lambda: EdgeListGraph.from_tuples(graphs.lcg_graph()),
         "lcg_sparse": lambda: EdgeListGraph.from_tuples(graphs.lcg_graph(n=600, m=700, seed=5))}[name]()
    with _ctx(gpu_ctx_factory, g) as ctx:
        res, st = _check(ctx)
        assert st["sources"] == len(ctx.graph()[0]) and st["unknown_sources"] == 0
        assert st["device_bytes"] > 0 and st["edges_gathered"] > 0


# (3) lane packing: partial batches, a source that is another source's successor, S == 1, raw sums, duplicate / unknown ids
@pytest.mark.parametrize("S", [1, 2, 7, 8, 9, 17])
def test_lane_packing(gpu_ctx_factory, S):
    with _ctx(gpu_ctx_factory, EdgeListGraph.from_tuples(graphs.lcg_graph())) as ctx:
        ids, row_ptr, src = ctx.graph()
        n = len(ids)
        # an edge u -> v first (v is u's successor), then sids spread over the graph
        v = int(np.flatnonzero(np.diff(np.asarray(row_ptr, dtype=np.int64)) > 0)[0])
        u = int(src[int(row_ptr[v])])
        sids = [u, v][:S] + [s for s in range(3, n, 11) if s not in (u, v)][:max(S - 2, 0)]
        assert len(set(sids)) == S
        res, st = _check(ctx, sids)
        vals = res.values()
        if S == 1:
            assert np.isnan(vals[sids[0]]) and (np.isinf(vals[res.reached]) | np.isnan(vals[res.reached])).all()
        # HB_BC_RAW: the restatement's sums, and value x S (S - 1) within 1 ulp
        sources = ids[np.asarray(sids, dtype=np.int64)]
        tol = bref.rtol(n, row_ptr, src, res)
        raw = ctx.betweenness(sources, raw=True)
        _compare(ctx, ids, res, tol, raw, "raw", raw=True)
        if S > 1:
            _, norm_vals, _ = ctx.betweenness(sources)
            back = norm_vals * np.float64(S * (S - 1))
            assert (np.abs(back - raw[1]) <= np.spacing(raw[1])).all()
        # duplicates count once, unknown ids are counted
        dup = np.concatenate([sources, sources[:1], _u128([1 << 90, (1 << 90) + 1])])
        got = ctx.betweenness(dup, raw=True)
        assert got[2]["sources"] == S and got[2]["unknown_sources"] == 2
        assert got[0].tobytes() == raw[0].tobytes() and got[1].tobytes() == raw[1].tobytes()


# (4) hubs through chunk trees both ways, the heavy reader list in the backward pull
def test_star_hubs_through_chunk_trees(gpu_ctx_factory):
    leaves = 100_000
    with _ctx(gpu_ctx_factory, _star(leaves)) as ctx:
        ids = ctx.graph()[0]
        assert ctx.plan()["nv"] > 0 and _ints(ids[:3]) == [1, 2, 3]
        sids = [0, 1, 2, 3, 50, 5000, 70_000, leaves + 1]  # hub 1, hub 2 and six leaves
        res, st = _check(ctx, sids, ref=bref.numpy, debug=True)
        assert st["max_dist"] == 3 and st["results"] == leaves + 2
        # closed forms.  From a leaf x: x -> 1 -> 2 -> every other leaf, one path each: delta_x(2) = L - 1, delta_x(1) = L.  From hub 1:
        # delta(2) = L.  From hub 2 (2 -> leaf -> 1): every leaf carries 1 / L of the one pair (2, 1).
        L = float(leaves)
        _, raw, _ = ctx.betweenness(ids[np.asarray(sids, dtype=np.int64)], raw=True)
        assert raw[0] == 6 * L                        # node 1: six leaf sources, delta = L each (itself and hub 2: nothing)
        assert raw[1] == 6 * (L - 1) + L              # node 2: the leaf sources and hub 1
        leaf = raw[2 + 7]                             # a leaf that is no source: only hub 2's walk passes it
        assert leaf == 1.0 / L


# (5) path counts are integers: 2^60 and 2^63 exact, 2^64 saturates; a binomial lattice with unequal terms through a chunk tree
def test_path_counts(gpu_ctx_factory):
    for k in (60, 63):
        with _ctx(gpu_ctx_factory, _diamonds(k)) as ctx:
            res, st = _check(ctx, [0], modes=(None,))
            _, sigma, _ = ctx.debug_betweenness_batch()
            assert int(sigma[-1, 0]) == 2 ** k and st["max_dist"] == 2 * k
    with _ctx(gpu_ctx_factory, _diamonds(64)) as ctx:
        ids = ctx.graph()[0]
        ctx.betweenness(ids[[3]])  # a result ...
        assert ctx.betweenness_count() > 0
        for mode in MODES:
            with pytest.raises(_lib.HyperballError) as e:
                ctx.betweenness(ids[[0]], mode=mode)
            assert e.value.code == _lib.HB_ERR_LIMIT
            with pytest.raises(_lib.HyperballError) as e:  # ... that is gone
                ctx.betweenness_count()
            assert e.value.code == _lib.HB_ERR_INVALID
        _check(ctx, [3], modes=(None,))  # from the second diamond on there are 2^63 paths: fine again
    # 12 x 12 lattice (right / down edges) and a sink behind its last anti-diagonal: the sink's in-list has the binomials C(11, i)
    side = 12
    node = lambda i, j: 1 + i * side + j  # noqa: E731
    t = [(node(i, j), node(i + 1, j)) for i in range(side - 1) for j in range(side)] + [(node(i, j), node(i, j + 1)) for i in range(side) for j in range(side - 1)]
    sink = 1000
    t += [(node(i, side - 1 - i), sink) for i in range(side)]
    with _ctx(gpu_ctx_factory, EdgeListGraph.from_tuples(t), chunk=4) as ctx:
        assert ctx.plan()["nv"] > 0
        res, st = _check(ctx, [0, 1, 13])
        assert res.sigma[0][-1] == 2 ** (side - 1) and res.sigma[0][side * side - 1] == math.comb(2 * side - 2, side - 1)


# (6) depth: the distances are bytes
def test_depth_limit(gpu_ctx_factory):
    with _ctx(gpu_ctx_factory, _path(255)) as ctx:
        res, st = _check(ctx, [0])
        assert st["max_dist"] == 254 and st["results"] == 255
    with _ctx(gpu_ctx_factory, _path(256)) as ctx:
        ids = ctx.graph()[0]
        with pytest.raises(_lib.HyperballError) as e:
            ctx.betweenness(ids[[0]])
        assert e.value.code == _lib.HB_ERR_LIMIT
        res, st = _check(ctx, [1], modes=(None,))
        assert st["max_dist"] == 254


# (7) modes on a deep R-MAT graph with a long tail
def test_modes_on_a_long_tail_graph(gpu_ctx_factory):
    g = synth.RmatGraph(12, 30_000, tail=(900, 980, 2))
    graph = (g.ids, g.row_ptr, g.src)
    sids = sorted(np.random.default_rng(11).choice(g.n, 16, replace=False).tolist())
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        res, st = _check(ctx, sids, graph=graph, ref=bref.numpy)
        assert st["levels_mode"][0] > 0 and st["levels_mode"][1] + st["levels_mode"][2] > 0, st["levels_mode"]  # both kinds of level
        a = ctx.betweenness(g.ids[np.asarray(sids)])
        b = ctx.betweenness(g.ids[np.asarray(sids)])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()  # bit for bit


# (8) state: results, distances and a later hb_run are untouched; a second load
def test_state_of_the_other_operators_and_reload(gpu_ctx_factory):
    g = synth.RmatGraph(12, 30_000)
    graph = (g.ids, g.row_ptr, g.src)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        h0 = ctx.state_hash()
        r0 = ctx.results()
        want = dref.bfs(g.n, g.row_ptr, g.src, [11, 500])
        ctx.distances(g.ids[[11, 500]])
        _check(ctx, [3, 11, 500, 1000, 2000], modes=(None,), graph=graph, ref=bref.numpy)
        assert np.array_equal(ctx.distance_all(), want)
        r1 = ctx.results()
        assert r0[0].tobytes() == r1[0].tobytes() and r0[1].tobytes() == r1[1].tobytes()
        with pytest.raises(_lib.HyperballError):  # the HyperBall state was borrowed: hb_step needs a new hb_begin
            ctx.step()
        ctx.run()
        assert ctx.state_hash() == h0
        r2 = ctx.results()
        assert r0[0].tobytes() == r2[0].tobytes() and r0[1].tobytes() == r2[1].tobytes()
        # a smaller graph on the same context: nothing of the first one answers for it
        ctx.load_edges(EdgeListGraph.from_tuples(graphs.lcg_graph(n=70, m=300, seed=3)).host_edges())
        with pytest.raises(_lib.HyperballError) as e:
            ctx.betweenness_count()
        assert e.value.code == _lib.HB_ERR_INVALID
        _check(ctx)


# (9) record input: the same graph as a stream of records with duplicates (self links among them) gives the same values bit for bit as
# its clean edge list; and the self links themselves change no value beyond rounding (they are edges of the graph, so they move rows in
# the device layout and with them the order of the terms, but they lie on no shortest path)
def test_appended_records_with_duplicates_and_self_links(gpu_ctx_factory):
    tuples = graphs.lcg_graph(n=150, m=500, seed=9)
    nodes = sorted({t[0] for t in tuples} | {t[1] for t in tuples})
    loops = [(v, v) for v in nodes[::3]]
    clean = EdgeListGraph.from_tuples(sorted(set((t[0], t[1]) for t in tuples + loops))).host_edges()
    noisy = EdgeListGraph.from_tuples(tuples[:200] + loops + tuples[100:] + loops[:7] + tuples[:50]).host_edges()
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        ctx.load_edges(clean)
        assert ctx.stats()["m_unique"] == len(clean) < len(noisy)
        a = ctx.betweenness()
        res, _ = _check(ctx, modes=(None,))
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        ctx.append_edges(noisy[:300])
        ctx.append_edges(noisy[300:])
        ctx.finalize()
        assert ctx.stats()["m_unique"] == len(clean)
        b = ctx.betweenness()
    assert len(a[0]) > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    with _ctx(gpu_ctx_factory, EdgeListGraph.from_tuples(tuples)) as ctx:  # without the self links: the same restatement, the same rule
        ids, row_ptr, src = ctx.graph()
        plain = bref.literal(len(ids), row_ptr, src, range(len(ids)))
        assert np.array_equal(plain.reached, res.reached) and all(np.array_equal(x, y) for x, y in zip(plain.dist, res.dist)) and plain.sigma == res.sigma
        _compare(ctx, ids, res, bref.rtol(len(ids), row_ptr, src, plain), ctx.betweenness(), None, debug=False)


# (10) refusals
def test_refusals(gpu_ctx_factory):
    def refused(fn):
        with pytest.raises(_lib.HyperballError) as e:
            fn()
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_betweenness" in str(e.value)

    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        refused(lambda: ctx.betweenness())  # no graph loaded
        refused(lambda: ctx.betweenness_count())
        ctx.load_edges(np.zeros(0, dtype=_lib.EDGE))  # an empty graph: an empty result
        ids, vals, st = ctx.betweenness()
        assert len(ids) == 0 and len(vals) == 0 and st["sources"] == 0 and st["results"] == 0 and ctx.betweenness_count() == 0
    with _ctx(gpu_ctx_factory, graphs.fixture_graph()) as ctx:
        refused(lambda: ctx.betweenness_copy())  # no result yet
        refused(lambda: ctx.betweenness(flags=_lib.HB_BC_DENSE_ONLY | _lib.HB_BC_SPARSE_ONLY))
        ctx.begin()
        ctx.step()
        refused(lambda: ctx.betweenness())  # between hb_begin and hb_finish
        ctx.finish()
        ids, vals, st = ctx.betweenness(_u128([77, 78]))  # all sources unknown: succeeds, no result
        assert len(ids) == 0 and st["sources"] == 0 and st["unknown_sources"] == 2
        _check(ctx, modes=(None,))
    with _ctx(gpu_ctx_factory, _path(100_001)) as ctx:
        refused(lambda: ctx.betweenness())  # sources == NULL means every node: more than the reference's 100 000
        ids = ctx.graph()[0]
        got_ids, vals, st = ctx.betweenness(ids[[99_990]])
        assert len(got_ids) == 11 and st["max_dist"] == 10
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        refused(lambda: ctx.betweenness())


# C2 size, 8 sources against the numpy restatement (GPU only)
def test_c2_against_numpy(gpu_ctx_factory):
    g = synth.RmatGraph(20, 20_000_000)
    graph = (g.ids, g.row_ptr, g.src)
    outdeg = np.bincount(np.asarray(g.src, dtype=np.int64), minlength=g.n)
    sids = sorted(set([int(np.argmax(outdeg))] + np.random.default_rng(5).choice(np.flatnonzero(outdeg > 0), 7, replace=False).tolist()))
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        res, st = _check(ctx, sids, modes=(None,), graph=graph, ref=bref.numpy)
        assert st["levels_mode"][0] > 0
