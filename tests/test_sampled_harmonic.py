"""hb_sampled_harmonic (ApproxHarmonic::build, approx_harmonic.rs:40-89) against the host restatement in tests/sample_ref.py:
per-node distance histograms c_d bit-exact, values bit-exact to the definition of include/hyperball.h and within the reference's own
AMPC tolerance of its sequential f32 loop, the seeded sampler, the results API on the sampled result, refusals."""
import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import EdgeListGraph
from tests import graphs
from tests import sample_ref as ref

pytestmark = pytest.mark.gpu


def _ints(ids):
    return [int(i["lo"]) | (int(i["hi"]) << 64) for i in ids]


def _u128(ints):
    out = np.zeros(len(ints), dtype=_lib.U128)
    for i, v in enumerate(ints):
        out[i]["lo"] = v & ref.MASK64
        out[i]["hi"] = v >> 64
    return out


def _ctx(factory, graph, flags=_lib.HB_FLAG_ALL_RELS, **kw):
    ctx = factory(flags=flags, **kw)
    e = graph.host_edges()
    ctx.load_edges(e)
    return ctx


def _check(ctx, sources_sids=None, max_dist=7, seed=1, samples=0, num_nodes=0, tol_check=True):
    """one sampled run vs the restatement; returns (stats, reference histogram)"""
    ids, row_ptr, src = ctx.graph()
    n = len(ids)
    kw = dict(max_dist=max_dist, seed=seed, samples=samples, num_nodes=num_nodes)
    if sources_sids is not None:
        kw["sources"] = ids[np.asarray(sources_sids, dtype=np.int64)]
        srcs = list(sources_sids)
    st = ctx.sampled_harmonic(**kw)
    D = max_dist + 1
    assert st["levels"] == D
    if sources_sids is None:
        k = samples or ref.default_k(num_nodes or n)
        srcs = list(ref.sample_sids(n, row_ptr, src, seed, k))
        assert st["k_req"] == k
    assert st["sources"] == len(srcs)
    h_ref = ref.dijkstra_histogram(n, row_ptr, src, srcs, max_dist)
    h = ctx.sample_histogram()
    assert np.array_equal(h, h_ref)
    k_req = st["k_req"]
    N = num_nodes or n
    want = ref.values(h_ref, N, k_req)
    rid, rval = ctx.results()
    keep = ~np.isnan(want)
    assert st["results"] == int(keep.sum()) == len(rid)
    assert _ints(rid) == _ints(ids[keep])
    assert np.array_equal(rval.view(np.uint64), want[keep].view(np.uint64))
    if tol_check and keep.any() and np.isfinite(want[keep]).all():
        loop = ref.f32_loop(h_ref, N, k_req)[keep]
        assert np.all(np.abs(rval - loop) <= 1e-4 * np.abs(loop))  # entrypoint/ampc/harmonic_centrality/mod.rs:165-171
    return st, h_ref


def _path(length):
    return EdgeListGraph.from_tuples([(i, i + 1) for i in range(1, length)])


# (a) histograms and values bit-exact
def test_fixture_graphs(gpu_ctx_factory):
    with _ctx(gpu_ctx_factory, graphs.fixture_graph()) as ctx:
        _check(ctx, sources_sids=[0, 1, 2, 3])
        _check(ctx, samples=3, seed=5)
    g, _ = graphs.host_fixture()
    with _ctx(gpu_ctx_factory, g) as ctx:
        _check(ctx, sources_sids=[0, 2, 3])


def test_lcg_graph_max_dist_variants(gpu_ctx_factory):
    g = EdgeListGraph.from_tuples(graphs.lcg_graph())
    with _ctx(gpu_ctx_factory, g) as ctx:
        for md in (1, 7, 15):
            _check(ctx, max_dist=md, seed=md)


def test_directed_path_counts_distance_max_dist_plus_one(gpu_ctx_factory):
    with _ctx(gpu_ctx_factory, _path(12)) as ctx:
        st, h = _check(ctx, sources_sids=[0])
        # node 1 is the source; nodes 2..9 at distances 1..8 count, 10.. (distance 9+) do not
        assert h[:, :].sum() == 8 and h[8, 7] == 1 and h[9].sum() == 0
        ids, _ = ctx.results()
        assert _ints(ids) == list(range(2, 10))


# (c) batch boundaries
@pytest.mark.parametrize("k", [1, 511, 512, 513, 1100])
def test_batch_boundaries(gpu_ctx_factory, k):
    g = EdgeListGraph.from_tuples(graphs.lcg_graph(n=1500, m=6000, seed=k))
    with _ctx(gpu_ctx_factory, g) as ctx:
        st, _ = _check(ctx, samples=k, seed=k, tol_check=False)
        assert st["batches"] == (st["sources"] + 511) // 512


# (d) layout variants give identical histograms
@pytest.mark.parametrize("variant", ["chunk4", "no_reorder", "no_sparse", "no_frontier", "host_plan", "host_ingest"])
def test_layout_variants(gpu_ctx_factory, variant):
    extra = {"chunk4": 0, "no_reorder": _lib.HB_FLAG_NO_REORDER, "no_sparse": _lib.HB_FLAG_NO_SPARSE, "no_frontier": _lib.HB_FLAG_NO_FRONTIER,
             "host_plan": _lib.HB_FLAG_HOST_PLAN, "host_ingest": _lib.HB_FLAG_HOST_INGEST}[variant]
    tuples = graphs.lcg_graph(n=400, m=3000, seed=3) + [(1, v) for v in range(2, 300)] + [(v, 7) for v in range(8, 350)]  # hubs both ways
    g = EdgeListGraph.from_tuples(tuples)
    hists, modes = [], []
    for flags, chunk in ((_lib.HB_FLAG_ALL_RELS, 0), (_lib.HB_FLAG_ALL_RELS | extra, 4 if variant == "chunk4" else 0)):
        with _ctx(gpu_ctx_factory, g, flags=flags, chunk=chunk) as ctx:
            st, _ = _check(ctx, samples=40, seed=9, tol_check=False)
            hists.append(ctx.sample_histogram())
            modes.append(int(np.bitwise_or.reduce(np.asarray(st["level_modes"], dtype=np.int64))))
    assert np.array_equal(hists[0], hists[1])
    # the default-flags context has sweep support: on this graph the A_t rule takes the 40 walks through a sweep level (1), dense levels
    # (2-5) and a bitmap level (6), so all six instances of the level kernel have produced the restatement's histogram
    assert modes[0] == 0b111


# (e) the sampler
def test_sampler(gpu_ctx_factory):
    g = EdgeListGraph.from_tuples(graphs.lcg_graph(n=300, m=500, seed=4) + [(1000, 1000)])  # 1000: only a self link
    with _ctx(gpu_ctx_factory, g) as ctx:
        ids, row_ptr, src = ctx.graph()
        n = len(ids)
        for seed, k in ((0, 10), (7, 100), (123, 10 ** 4)):
            got = ctx.sample_sources(seed, k)
            assert _ints(got) == _ints(ids[ref.sample_sids(n, row_ptr, src, seed, k)])
        every = _ints(ctx.sample_sources(1, 10 ** 4))
        assert 1000 in every  # a self link makes a candidate
        cand = len(every)
        # default k = the formula; norm uses k_req even when fewer candidates exist
        st, _ = _check(ctx, seed=3, num_nodes=5000)
        assert st["k_req"] == ref.default_k(5000) and st["sources"] == ref.default_k(5000)
        st, _ = _check(ctx, seed=3, samples=cand + 50)
        assert st["k_req"] == cand + 50 and st["sources"] == cand


# (f) HB_FLAG_ALL_RELS
def test_all_rels_follows_skipped_edges(gpu_ctx_factory):
    g = EdgeListGraph.from_tuples([(1, 2, graphs.NOFOLLOW), (2, 3, graphs.TAG), (3, 4, 0)])
    with _ctx(gpu_ctx_factory, g) as ctx:
        assert ctx.stats()["m_eff"] == 3
        _check(ctx, sources_sids=[0])
        assert _ints(ctx.results()[0]) == [2, 3, 4]
    with _ctx(gpu_ctx_factory, g, flags=0) as ctx:
        assert ctx.stats()["m_eff"] == 1
        ctx.sampled_harmonic(sources=_u128([1]))
        assert len(ctx.results()[0]) == 0


# (g) results API on the sampled result, and hb_run around it
def test_results_api_and_hyperball_unchanged(gpu_ctx_factory, tmp_path):
    from tests import speedy_kv_reader as kv
    g = synth.RmatGraph(12, 30_000)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        h0 = list(ctx.state_hash())
        r0 = ctx.results()
        st = ctx.sampled_harmonic(seed=11)
        ids, vals = ctx.results()
        assert len(ids) == st["results"] > 0
        ranks = ctx.ranks()
        order = sorted(range(len(vals)), key=lambda j: (-vals[j], _ints(ids[j:j + 1])[0]))
        pos = np.empty(len(order), dtype=np.int64)
        pos[order] = np.arange(len(order))
        assert np.array_equal(ranks.astype(np.int64), pos)
        tid, tval = ctx.top(25)
        assert _ints(tid) == [_ints(ids[j:j + 1])[0] for j in order[:25]]
        assert np.array_equal(tval, vals[order[:25]])
        ctx.store_harmonic(str(tmp_path))
        cen = kv.Db(str(tmp_path / "harmonic"), "f64", str(tmp_path))
        rnk = kv.Db(str(tmp_path / "harmonic_rank"), "u64", str(tmp_path))
        ints = kv.ids_to_ints(ids)
        got = dict(cen.items())
        assert len(got) == len(ids)
        assert all(np.float64(got[i]).view(np.uint64) == np.float64(v).view(np.uint64) for i, v in zip(ints, vals.tolist()))
        assert dict(rnk.items()) == dict(zip(ints, ranks.tolist()))
        ctx.run()
        assert list(ctx.state_hash()) == h0
        r1 = ctx.results()
        assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1].view(np.uint64), r1[1].view(np.uint64))


# (h) refusals and edge cases
def test_refusals_and_edge_cases(gpu_ctx_factory):
    with _ctx(gpu_ctx_factory, EdgeListGraph.from_tuples([])) as ctx:
        st = ctx.sampled_harmonic(seed=1)
        assert st["sources"] == 0 and len(ctx.results()[0]) == 0
    with _ctx(gpu_ctx_factory, graphs.fixture_graph()) as ctx:
        st = ctx.sampled_harmonic(num_nodes=1)  # k = 0 for N <= 1: empty, not an error
        assert st["k_req"] == 0 and len(ctx.results()[0]) == 0
        st = ctx.sampled_harmonic(num_nodes=1, samples=2, seed=3)  # N = 1: norm = inf
        _, vals = ctx.results()
        assert len(vals) and np.all(np.isinf(vals))
        for bad in ([graphs.A, graphs.A], [graphs.A, 99], []):  # duplicate, unknown, an explicit empty list (not "sample")
            with pytest.raises(_lib.HyperballError) as e:
                ctx.sampled_harmonic(sources=_u128(bad))
            assert e.value.code == _lib.HB_ERR_INVALID
        with pytest.raises(_lib.HyperballError) as e:
            ctx.sampled_harmonic(max_dist=16)
        assert e.value.code == _lib.HB_ERR_LIMIT
        with pytest.raises(_lib.HyperballError) as e:
            ctx.sampled_harmonic(samples=65536)
        assert e.value.code == _lib.HB_ERR_LIMIT
    # not in the middle of a HyperBall run (its state and result snapshots belong to that run)
    with _ctx(gpu_ctx_factory, graphs.fixture_graph()) as ctx:
        ctx.begin()
        ctx.step()
        with pytest.raises(_lib.HyperballError) as e:
            ctx.sampled_harmonic()
        assert e.value.code == _lib.HB_ERR_INVALID
        ctx.finish()
        ctx.sampled_harmonic(sources=_u128([graphs.A]))
        assert _ints(ctx.results()[0]) == [graphs.B, graphs.C]
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        with pytest.raises(_lib.HyperballError) as e:
            ctx.sampled_harmonic()
        assert e.value.code == _lib.HB_ERR_INVALID


# (j) C2 size, default k, against the bit-parallel BFS
def test_c2_default_k_bit_exact(gpu_ctx_factory):
    g = synth.RmatGraph(20, 20_000_000)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        st = ctx.sampled_harmonic(seed=2024)
        n = len(g.ids)
        k = ref.default_k(n)
        assert st["k_req"] == k
        srcs = ref.sample_sids(n, g.row_ptr, g.src, 2024, k)
        h_ref = ref.bfs_histogram(n, g.row_ptr, g.src, srcs, 7)
        assert np.array_equal(ctx.sample_histogram(), h_ref)
        want = ref.values(h_ref, n, k)
        keep = ~np.isnan(want)
        ids, vals = ctx.results()
        assert len(ids) == int(keep.sum())
        assert np.array_equal(vals.view(np.uint64), want[keep].view(np.uint64))


# the operator mirror (stract_amd/approx_harmonic.py): build -> get / iter / len, and the two stores it writes
def test_approx_harmonic_mirror(gpu_ctx_factory, tmp_path):
    from stract_amd.approx_harmonic import ApproxHarmonic
    from tests import speedy_kv_reader as kv
    g = EdgeListGraph.from_tuples([(a, b, graphs.NOFOLLOW) for a, b in graphs.lcg_graph(n=120, m=600, seed=8)])
    ah = ApproxHarmonic.build(g, str(tmp_path / "out"), seed=4)
    with _ctx(gpu_ctx_factory, g) as ctx:
        st = ctx.sampled_harmonic(seed=4)
        ids, vals = ctx.results()
    assert ah.len() == len(ids) == st["results"] > 0
    assert list(ah.iter()) == list(zip(_ints(ids), vals.tolist()))
    assert ah.get(_ints(ids[:1])[0]) == vals[0] and ah.get(10 ** 9) is None
    cen = kv.Db(str(tmp_path / "out" / "harmonic"), "f64", str(tmp_path))
    assert dict(cen.items()) == dict(zip(_ints(ids), vals.tolist()))


# (i) the page graph straight from an edge store (hb_load_webgraph with HBW_PAGE_GRAPH)
def test_page_graph_load_of_an_edge_store(gpu_ctx_factory, tmp_path):
    from stract_amd import webgraph
    from tests import tantivy_fixture as tf
    rng = np.random.default_rng(17)
    pages = [(int(a), int(b), int(f)) for a, b, f in zip(rng.integers(1, 300, 1200), rng.integers(1, 300, 1200),
                                                         rng.choice([0, graphs.NOFOLLOW, graphs.TAG], 1200))]
    page = EdgeListGraph.from_tuples(pages).host_edges()
    host = page.copy()  # the host-id columns hold other ids: a load that read them would build another graph
    host["from"]["lo"] = (page["from"]["lo"] % 7) + 5000
    host["to"]["lo"] = (page["to"]["lo"] % 5) + 6000
    tf.write_edge_store(str(tmp_path / "edges"), [host[:500], host[500:]], page_segments=[page[:500], page[500:]])
    with _ctx(gpu_ctx_factory, EdgeListGraph(page)) as want:
        want.sampled_harmonic(seed=5)
        wids, wvals = want.results()
        wh = want.sample_histogram()
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        webgraph.load_webgraph(ctx, str(tmp_path / "edges"), verify_crc=True, page_graph=True)
        assert ctx.stats()["m_input"] == len(page) and ctx.stats()["m_eff"] == ctx.stats()["m_unique"]
        _check(ctx, seed=5)
        ids, vals = ctx.results()
        assert np.array_equal(ids, wids) and np.array_equal(vals.view(np.uint64), wvals.view(np.uint64))
        assert np.array_equal(ctx.sample_histogram(), wh)
        with pytest.raises(_lib.HyperballError) as e:
            webgraph.load_webgraph(ctx, str(tmp_path / "edges"), page_ids=True, page_graph=True)
        assert e.value.code == _lib.HB_ERR_INVALID
    with gpu_ctx_factory(flags=_lib.HB_FLAG_REFERENCE_TAIL) as ctx:
        with pytest.raises(_lib.HyperballError) as e:
            webgraph.load_webgraph(ctx, str(tmp_path / "edges"), page_graph=True)
        assert e.value.code == _lib.HB_ERR_INVALID
