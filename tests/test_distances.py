"""hb_distances (ShortestPaths, crates/core/src/webgraph/shortest_path.rs:26-227) against the host restatement in tests/distance_ref.py.
Every comparison is exact: the id list and the distance bytes both equal the restatement's map."""
import json
import os

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import EdgeListGraph
from tests import distance_ref as dref
from tests import graphs

pytestmark = pytest.mark.gpu

MODES = (None, "top_down", "bottom_up")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shortest_path_cases.json")


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


def _run(ctx, ids, want, sources, reversed, max_dist, mode):
    """one call, compared with the restatement's distance array `want` (per sid) in all three result forms; returns the stats"""
    keep = want != dref.UNREACHED
    got_ids, got_dist, st = ctx.distances(sources, reversed=reversed, max_dist=max_dist, mode=mode)
    assert np.array_equal(got_ids, ids[keep]), (reversed, max_dist, mode)
    assert np.array_equal(got_dist, want[keep]), (reversed, max_dist, mode)
    # (9) the three result calls agree with each other and with the statistics
    assert np.array_equal(ctx.distance_all(), want)
    assert ctx.distance_count() == len(got_ids) == st["reached"] == sum(st["frontier"])
    assert st["max_distance"] == (int(want[keep].max()) if keep.any() else 0)
    assert len(st["step"]) == st["levels"] + 1
    if mode == "top_down":
        assert not any(st["step"])
    if mode == "bottom_up":
        assert all(st["step"][1:])
    return st


def _check(ctx, source_sids, reversed=False, max_dist=None, modes=MODES, graph=None, ref=dref.dijkstra):
    """(5) the default run and the two forced steps against the restatement; returns the default run's stats"""
    ids, row_ptr, src = graph if graph is not None else ctx.graph()
    want = ref(len(ids), row_ptr, src, source_sids, reversed=reversed, max_dist=max_dist)
    sources = ids[np.asarray(source_sids, dtype=np.int64)]
    stats = [_run(ctx, ids, want, sources, reversed, max_dist, mode) for mode in modes]
    return stats[0]


def _both_kinds(st):
    return 0 in st["step"][1:] and 1 in st["step"][1:]


def _path(length):
    return EdgeListGraph.from_tuples([(i, i + 1) for i in range(1, length)])


def _star(leaves=100_000):
    """hub 1 has `leaves` in-edges, hub 2 has `leaves` out-edges, 1 -> 2: the chunk trees of both are on every path"""
    t = [(v, 1) for v in range(3, leaves + 3)] + [(2, v) for v in range(3, leaves + 3)] + [(1, 2)]
    return EdgeListGraph.from_tuples(t)


def _long_tail():
    g = synth.RmatGraph(12, 30_000, tail=(900, 980, 2))  # 53 levels from its largest hub
    return g


# (1) the reference's own known answers (webgraph/tests.rs:58-180)
def test_reference_known_answers(gpu_ctx_factory):
    from stract_amd.shortest_path import ShortestPaths
    with open(GOLDEN) as f:
        gold = json.load(f)
    for case in gold["cases"]:
        g = gold["graphs"][case["graph"]]
        nid = g["nodes"]
        graph = EdgeListGraph.from_tuples([(nid[a], nid[b]) for a, b in g["edges"]])
        with ShortestPaths.from_graph(graph) as sp:
            src = nid[case["source"]]
            node_map = sp.reversed_distances(src) if case["reversed"] else sp.distances(src)
            raw = sp.raw_reversed_distances(src) if case["reversed"] else sp.raw_distances(src)
            raw7 = sp.raw_reversed_distances_with_max(src, 7) if case["reversed"] else sp.raw_distances_with_max(src, 7)
        for name, d in case["expect"].items():
            assert node_map.get(nid[name]) == d, case["name"]
            assert raw.get(nid[name]) == d and raw7.get(nid[name]) == d, case["name"]
        if "expect_len" in case:
            assert len(node_map) == case["expect_len"], case["name"]
            assert raw == {src: 0} == raw7, case["name"]  # dijkstra_multi inserts the source before it looks at an edge
        assert raw[src] == 0 and list(raw) == sorted(raw)
    # the D source of the A/B/C/D graph reversed: nothing but D
    g = gold["graphs"]["abcd"]
    nid = g["nodes"]
    with _ctx(gpu_ctx_factory, EdgeListGraph.from_tuples([(nid[a], nid[b]) for a, b in g["edges"]])) as ctx:
        ids, dist, st = ctx.distances(_u128([nid["D"]]), reversed=True)
        assert _ints(ids) == [nid["D"]] and dist.tolist() == [0] and st["reached"] == 1
        ids, dist, st = ctx.distances(_u128([nid["E"]]))
        assert len(ids) == 0 and st["unknown_sources"] == 1 and st["reached"] == 0


# (2) fixture graphs: single / multi source, both directions, max_dist variants; the two restatements agree on them
@pytest.mark.parametrize("reversed", [False, True])
def test_fixture_graphs(gpu_ctx_factory, reversed):
    with _ctx(gpu_ctx_factory, graphs.fixture_graph()) as ctx:
        for srcs in ([0], [3], [0, 3], [1, 2, 3]):
            for md in (None, 0, 1, 7):
                _check(ctx, srcs, reversed, md)
    g, _ = graphs.host_fixture()
    with _ctx(gpu_ctx_factory, g) as ctx:
        for srcs in ([0], [2], [1, 3]):
            _check(ctx, srcs, reversed)


@pytest.mark.parametrize("reversed", [False, True])
def test_lcg_graph_max_dist_variants(gpu_ctx_factory, reversed):
    g = EdgeListGraph.from_tuples(graphs.lcg_graph())
    with _ctx(gpu_ctx_factory, g) as ctx:
        ids, row_ptr, src = ctx.graph()
        n = len(ids)
        for md in (None, 0, 1, 7, 15, 200):
            for srcs in ([5], [0, 17, 120, 199]):
                _check(ctx, srcs, reversed, md)
                a = dref.dijkstra(n, row_ptr, src, srcs, reversed=reversed, max_dist=md)
                assert np.array_equal(a, dref.bfs(n, row_ptr, src, srcs, reversed=reversed, max_dist=md))
    # a sparse one: deep, with unreachable parts
    g = EdgeListGraph.from_tuples(graphs.lcg_graph(n=600, m=700, seed=5))
    with _ctx(gpu_ctx_factory, g) as ctx:
        ids, row_ptr, src = ctx.graph()
        for md in (None, 1, 15):
            _check(ctx, [3], reversed, md)
            _check(ctx, [10, 11, 400], reversed, md)
            a = dref.dijkstra(len(ids), row_ptr, src, [10, 11, 400], reversed=reversed, max_dist=md)
            assert np.array_equal(a, dref.bfs(len(ids), row_ptr, src, [10, 11, 400], reversed=reversed, max_dist=md))


def test_wide_node_ids_and_duplicate_sources(gpu_ctx_factory):
    salt = 0x9E3779B97F4A7C15

    def nid(k):
        return ((k * salt) & 0xFFFFFFFFFFFFFFFF) | ((k % 7 + 1) << 64) | (k << 100)
    g = EdgeListGraph.from_tuples([(nid(a), nid(b)) for a, b in graphs.lcg_graph(n=150, m=500, seed=9)])
    with _ctx(gpu_ctx_factory, g) as ctx:
        ids = ctx.graph()[0]
        assert any(int(i["hi"]) for i in ids)
        for reversed in (False, True):
            _check(ctx, [7], reversed)
            _check(ctx, [0, 149], reversed, 3)
        # a duplicate and an unknown id next to a known one: counted, not an error
        a = ctx.distances(ids[[7]])
        b = ctx.distances(np.concatenate([ids[[7, 7]], _u128([12345])]))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2]["unknown_sources"] == 0 and b[2]["unknown_sources"] == 1 and b[2]["frontier"][0] == 1


# (3) the u8 rule on a directed path of 300 nodes
def test_u8_rule_on_a_long_path(gpu_ctx_factory):
    with _ctx(gpu_ctx_factory, _path(300)) as ctx:
        st = _check(ctx, [0])
        ids, dist, _ = ctx.distances(_u128([1]))
        assert _ints(ids) == list(range(1, 256)) and dist.tolist() == list(range(255))  # distances 0..254, the rest absent
        assert st["max_distance"] == 254 and st["reached"] == 255 and st["levels"] == 254
        for md in (254, 255):
            i2, d2, _ = ctx.distances(_u128([1]), max_dist=md)
            assert np.array_equal(i2, ids) and np.array_equal(d2, dist)
            _check(ctx, [0], max_dist=md)
        st = _check(ctx, [0], max_dist=9)
        ids, dist, _ = ctx.distances(_u128([1]), max_dist=9)
        assert len(ids) == 11 and dist.tolist() == list(range(11)) and st["levels"] == 10
        # reversed from the far end: the same rule the other way
        st = _check(ctx, [299], reversed=True)
        assert st["reached"] == 255
        st = _check(ctx, [299], reversed=True, max_dist=9)
        assert st["reached"] == 11


# (4) deep and wide graphs, (5) forced steps agree (inside _check), the default run uses both kinds of step on the star
def test_long_tail_graph_is_deep(gpu_ctx_factory):
    g = _long_tail()
    graph = (g.ids, g.row_ptr, g.src)
    outdeg = np.bincount(np.asarray(g.src, dtype=np.int64), minlength=g.n)
    hub = int(np.argmax(outdeg))
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        st = _check(ctx, [hub], graph=graph)
        assert st["levels"] >= 40, st["levels"]
        far = int(np.argmax(np.where(dref.dijkstra(g.n, g.row_ptr, g.src, [hub]) == dref.UNREACHED, 0, dref.dijkstra(g.n, g.row_ptr, g.src, [hub]))))
        st = _check(ctx, [far], reversed=True, graph=graph)
        assert st["max_distance"] >= 40
        _check(ctx, [hub, far], max_dist=15, graph=graph)


@pytest.mark.parametrize("reversed", [False, True])
def test_star_hubs_through_chunk_trees(gpu_ctx_factory, reversed):
    with _ctx(gpu_ctx_factory, _star()) as ctx:
        ids = ctx.graph()[0]
        assert ctx.plan()["nv"] > 0  # hub rows are split into chunk trees
        leaf = 5000
        st = _check(ctx, [leaf], reversed)
        assert st["reached"] == len(ids) and st["max_distance"] == 3
        assert _both_kinds(st), st["step"]  # the hub's 100 000 edges against what is left unexplored: Beamer's rule switches
        _check(ctx, [0], reversed, modes=(None,))      # from the hub with the in-edges
        _check(ctx, [1], reversed, 1, modes=(None,))   # from the hub with the out-edges
        _check(ctx, [0, 1, leaf], reversed, modes=(None,))


# the switch rule's constants can be overridden from the environment (read at every call): another sequence of steps, the same distances
def test_switch_rule_overrides_from_the_environment(gpu_ctx_factory, monkeypatch):
    with _ctx(gpu_ctx_factory, EdgeListGraph.from_tuples(graphs.lcg_graph())) as ctx:
        ids, row_ptr, src = ctx.graph()
        want = dref.bfs(len(ids), row_ptr, src, [5])
        st = _run(ctx, ids, want, ids[[5]], False, None, None)
        assert st["step"][1] == 0  # one frontier node against 1200 edges: top-down
        monkeypatch.setenv("HB_DIST_ALPHA", "1000000000")
        monkeypatch.setenv("HB_DIST_BETA", "1000000000")  # n_f * beta < n never holds
        eager = _run(ctx, ids, want, ids[[5]], False, None, None)
        assert all(eager["step"][1:]) and eager["levels"] == st["levels"]  # bottom-up from the first level on, and it never switches back
        monkeypatch.setenv("HB_DIST_ALPHA", "0")  # not a number the rule can use: the built-in constant
        monkeypatch.setenv("HB_DIST_BETA", "")
        assert _run(ctx, ids, want, ids[[5]], False, None, None)["step"] == st["step"]


# (6) layout variants give identical output
@pytest.mark.parametrize("variant", ["chunk4", "no_reorder", "no_xcd_map", "host_plan", "host_ingest", "no_sparse"])
def test_layout_variants(gpu_ctx_factory, variant):
    extra = {"chunk4": 0, "no_reorder": _lib.HB_FLAG_NO_REORDER, "no_xcd_map": _lib.HB_FLAG_NO_XCD_MAP, "host_plan": _lib.HB_FLAG_HOST_PLAN,
             "host_ingest": _lib.HB_FLAG_HOST_INGEST, "no_sparse": _lib.HB_FLAG_NO_SPARSE}[variant]
    tuples = graphs.lcg_graph(n=400, m=3000, seed=3) + [(1, v) for v in range(2, 300)] + [(v, 7) for v in range(8, 350)]  # hubs both ways
    g = EdgeListGraph.from_tuples(tuples)
    out = []
    for flags, chunk in ((_lib.HB_FLAG_ALL_RELS, 0), (_lib.HB_FLAG_ALL_RELS | extra, 4 if variant == "chunk4" else 0)):
        with _ctx(gpu_ctx_factory, g, flags=flags, chunk=chunk) as ctx:
            for reversed in (False, True):
                for srcs, md in (([0], None), ([6], None), ([20, 399], 2)):
                    _check(ctx, srcs, reversed, md)
                    out.append(ctx.distance_all())
    half = len(out) // 2
    assert all(np.array_equal(a, b) for a, b in zip(out[:half], out[half:]))


# default contexts filter on SKIPPED_REL (the AMPC job, mapper.rs:116-119); HB_FLAG_ALL_RELS follows every edge (the trait)
def test_rel_filter_of_default_contexts(gpu_ctx_factory):
    g = EdgeListGraph.from_tuples([(1, 2, graphs.NOFOLLOW), (2, 3, graphs.TAG), (3, 4, 0)])
    with _ctx(gpu_ctx_factory, g) as ctx:
        ids, dist, _ = ctx.distances(_u128([1]))
        assert _ints(ids) == [1, 2, 3, 4] and dist.tolist() == [0, 1, 2, 3]
    with _ctx(gpu_ctx_factory, g, flags=0) as ctx:
        ids, dist, _ = ctx.distances(_u128([3]))
        assert _ints(ids) == [3, 4] and dist.tolist() == [0, 1]
        ids, dist, _ = ctx.distances(_u128([4]), reversed=True)
        assert _ints(ids) == [3, 4] and dist.tolist() == [1, 0]


# (7) page-level distances from an edge store (hb_load_webgraph with HBW_PAGE_GRAPH)
def test_page_graph_load_of_an_edge_store(gpu_ctx_factory, tmp_path):
    from stract_amd import webgraph
    from tests import tantivy_fixture as tf
    rng = np.random.default_rng(23)
    pages = [(int(a), int(b), int(f)) for a, b, f in zip(rng.integers(1, 300, 900), rng.integers(1, 300, 900),
                                                         rng.choice([0, graphs.NOFOLLOW, graphs.TAG], 900))]
    page = EdgeListGraph.from_tuples(pages).host_edges()
    host = page.copy()  # the host-id columns hold other ids: a load that read them would build another graph
    host["from"]["lo"] = (page["from"]["lo"] % 7) + 5000
    host["to"]["lo"] = (page["to"]["lo"] % 5) + 6000
    tf.write_edge_store(str(tmp_path / "edges"), [host[:400], host[400:]], page_segments=[page[:400], page[400:]])
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        webgraph.load_webgraph(ctx, str(tmp_path / "edges"), verify_crc=True, page_graph=True)
        assert ctx.stats()["m_input"] == len(page)
        ids = ctx.graph()[0]
        assert set(_ints(ids)) == {p[0] for p in pages} | {p[1] for p in pages}
        for reversed in (False, True):
            _check(ctx, [4], reversed)
            _check(ctx, [9, 100], reversed, 2)


# (8) state: the centrality results and a later hb_run are untouched
def test_results_and_hyperball_unchanged(gpu_ctx_factory):
    g = synth.RmatGraph(12, 30_000)
    graph = (g.ids, g.row_ptr, g.src)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        h0 = ctx.state_hash()
        r0 = ctx.results()
        for reversed in (False, True):
            st = _check(ctx, [11, 500], reversed, graph=graph)
            assert st["reached"] > 1
            r1 = ctx.results()
            assert r0[0].tobytes() == r1[0].tobytes() and r0[1].tobytes() == r1[1].tobytes()
            assert ctx.state_hash() == h0
        ctx.run()
        assert ctx.state_hash() == h0
        r2 = ctx.results()
        assert r0[0].tobytes() == r2[0].tobytes() and r0[1].tobytes() == r2[1].tobytes()
        want = dref.dijkstra(g.n, g.row_ptr, g.src, [11, 500])
        ctx.distances(g.ids[[11, 500]])
        ctx.sampled_harmonic(seed=3)  # a sampled run in between does not disturb the distances either
        assert np.array_equal(ctx.distance_all(), want)


# (10) refusals
def test_refusals(gpu_ctx_factory):
    def refused(fn):
        with pytest.raises(_lib.HyperballError) as e:
            fn()
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_distance" in str(e.value)

    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        refused(lambda: ctx.distances(_u128([graphs.A])))  # no graph loaded
        refused(lambda: ctx.distance_count())
        ctx.load_edges(np.zeros(0, dtype=_lib.EDGE))  # an empty graph: every source is unknown, nothing is reached
        ids, dist, st = ctx.distances(_u128([graphs.A, graphs.B]))
        assert len(ids) == 0 and len(dist) == 0 and st["reached"] == 0 and st["unknown_sources"] == 2 and st["levels"] == 0
        assert ctx.distance_count() == 0
    with _ctx(gpu_ctx_factory, graphs.fixture_graph()) as ctx:
        refused(lambda: ctx.distance_copy())  # no distances yet
        refused(lambda: ctx.distances(_u128([])))  # source_count == 0
        refused(lambda: ctx.distances(_u128([graphs.A]), flags=_lib.HB_DIST_TOP_DOWN_ONLY | _lib.HB_DIST_BOTTOM_UP_ONLY))
        ctx.begin()
        ctx.step()
        refused(lambda: ctx.distances(_u128([graphs.A])))  # between hb_begin and hb_finish
        ctx.finish()
        ids, dist, st = ctx.distances(_u128([graphs.A]))
        assert _ints(ids) == [graphs.A, graphs.B, graphs.C] and dist.tolist() == [0, 1, 1]
        ids, dist, st = ctx.distances(_u128([77, 78]))  # all sources unknown: succeeds, reaches nothing
        assert len(ids) == 0 and st["reached"] == 0 and st["unknown_sources"] == 2 and ctx.distance_count() == 0
        assert np.all(ctx.distance_all() == _lib.HB_DIST_UNREACHED)
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        refused(lambda: ctx.distances(_u128([graphs.A])))


# (11) C2 size, both directions, against the numpy BFS (GPU only)
@pytest.mark.parametrize("reversed", [False, True])
def test_c2_against_numpy_bfs(gpu_ctx_factory, reversed):
    g = synth.RmatGraph(20, 20_000_000)
    outdeg = np.bincount(np.asarray(g.src, dtype=np.int64), minlength=g.n)
    indeg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
    rng = np.random.default_rng(5)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        both = False
        for srcs, md in (([int(np.argmax(outdeg))], None), ([int(np.argmax(indeg))], None), (rng.integers(0, g.n, 3).tolist(), None),
                         (rng.integers(0, g.n, 1).tolist(), 2)):
            want = dref.bfs(g.n, g.row_ptr, g.src, srcs, reversed=reversed, max_dist=md)
            for mode in MODES:
                st = _run(ctx, g.ids, want, g.ids[np.asarray(srcs, dtype=np.int64)], reversed, md, mode)
                both = both or (mode is None and _both_kinds(st))
        assert both  # at this size the default run switches direction
