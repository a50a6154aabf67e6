"""hb_inbound_similarity with a limit (hb_similarity_options.limit: every BitVec from backlinks(v, limit) as hb_backlinks defines it)
against the host restatement in tests/limited_similarity_ref.py.

Comparison rule: EVERYTHING is exact.  Every check compares the scores of all nodes bit for bit and the counts / bloom / len of the
debug export as integers; the stats' listed rows and list entries are compared with what the graph says.  The restatement's numpy form
is used throughout (tests/test_limited_similarity_ref.py shows it equal to the literal one); the hand-written known answer runs through
the literal form."""
import ctypes
import json
import os

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import ids_from_ints
from tests import distance_ref as dref
from tests import fans
from tests import graphs
from tests import inbound_similarity_ref as sref
from tests import limited_similarity_ref as lref
from tests import similar_hosts_ref as shref
from tests.test_similar_hosts import A1, A2, A3, LONELY, SRC0, TALL, long_graph, small_graph, small_keys

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "limited_similarity_cases.json")


def _load(factory, graph, chunk=0, tune=()):
    ctx = factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk, tune=tune)
    ctx.load_dense(*graph)
    return ctx


def _set(ctx, keys):
    if keys:
        ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
    else:
        ctx.links_set_keys()


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _assert_exact(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


def _listed(graph, limit):
    """(listed rows, entries of their lists): a self link, or more in-neighbours than the limit"""
    if not limit:
        return 0, 0
    rp = np.asarray(graph[1], dtype=np.int64)
    src = np.asarray(graph[2], dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    self_link = np.bincount(rows[src == rows], minlength=len(rp) - 1)
    degree = np.diff(rp) - self_link
    listed = (self_link > 0) | (degree > limit)
    return int(listed.sum()), int(np.minimum(degree[listed], limit).sum())


def _check(ctx, graph, keys, limit, liked, disliked=(), normalized=False, self_score=None, modes=(None,), what=""):
    """one call per mode against the restatement: the scores of all nodes, the last batch's counts, bloom and len, the stats.
    `keys` must be what the context's key set holds.  Returns (scores, [stats], cut graph)."""
    ids = graph[0]
    cut = lref.cut_graph(*graph, lref.key_by_sid(ids, keys) if keys else None, limit)
    want = lref.numpy_scores(cut, liked, disliked, normalized, 1.0 if self_score is None else self_score)
    entries = list(liked) + list(disliked)
    last = entries[(len(entries) - 1) // 16 * 16:]
    w_counts, w_bloom, w_len = lref.numpy_export(cut, last)
    known = set(sref.id_ints(ids))
    stats = []
    for mode in modes:
        st = ctx.inbound_similarity(ids_from_ints(liked), ids_from_ints(disliked), normalized=normalized, self_score=self_score, mode=mode, limit=limit)
        tag = "%s limit %d (%s)" % (what, limit, mode)
        _assert_exact(ctx.similarity_all(), want, "scores " + tag)
        counts, bloom, length = ctx.debug_similarity_batch()
        bad = np.argwhere(counts[:, :len(last)] != w_counts)
        assert not len(bad), ("counts " + tag, bad[:5])
        assert not counts[:, len(last):].any(), tag
        assert np.array_equal(bloom, w_bloom), "bloom " + tag
        assert np.array_equal(length, w_len), ("len " + tag, np.flatnonzero(length != w_len)[:5])
        assert (st["listed_rows"], st["list_entries"]) == _listed(graph, limit), tag
        assert st["batches"] == (len(entries) + 15) // 16 and st["unknown"] == sum(1 for e in entries if e not in known)
        stats.append(st)
    return want, stats, cut


# ---- (0) the hand-written known answer, through the literal form --------------------------------------------------------------------
def test_known_answer(gpu_ctx_factory):
    with open(GOLDEN) as f:
        g = json.load(f)
    graph = graphs.dense_from_tuples([tuple(e) for e in g["edges"]])
    ints = sref.id_ints(graph[0])
    with _load(gpu_ctx_factory, graph) as ctx:
        for case in g["cases"]:
            keys = [tuple(k) for k in case["keys"]]
            _set(ctx, keys)
            st = ctx.inbound_similarity(ids_from_ints(case["liked"]), ids_from_ints(case["disliked"]), normalized=case["normalized"], limit=case["limit"])
            want = np.array([case["expect"].get(str(v), case["rest"]) for v in ints], dtype=np.float64)
            _assert_exact(ctx.similarity_all(), want, case["name"])
            _, _, length = ctx.debug_similarity_batch()
            assert {str(v): int(x) for v, x in zip(ints, length) if x} == case["len"], case["name"]
            # limit 2: 10 (four in-neighbours and a self link) and 11 (three); limit 8: 10 alone, for its self link
            assert st["listed_rows"] == {0: 0, 2: 2, 8: 1}[case["limit"]], case["name"]


# ---- (1) the cut at its edge -----------------------------------------------------------------------------------------------------------
FAN_KS = (3, 9, 63, 64, 65, 66, 200)


def _fan_graph(self_links=()):
    """the flipped fan - hub h_K has the in-list of length K - plus, per hub, a twin with the same in-list and a half twin with every
    second entry of it: nodes whose cut lists overlap the hub's, so the scores depend on which entries a cut keeps"""
    fan = fans.Fan(FAN_KS)
    t = fan.tuples(flipped=True)
    nxt = fan.n + 1
    twin, half = {}, {}
    for K in FAN_KS:
        leaves = (fan.leaves(K) + 1).tolist()
        twin[K], half[K] = nxt, nxt + 1
        nxt += 2
        t += [(v, twin[K]) for v in leaves] + [(v, half[K]) for v in leaves[1::2]]
    t += [(v, v) for v in self_links]
    return fan, graphs.dense_from_tuples(t), twin, half


@pytest.mark.parametrize("chunk", [0, 4])
def test_cut_at_its_edge(gpu_ctx_factory, chunk):
    fan, graph, twin, half = _fan_graph()
    K = 65  # under the default chunk (64) the uncut list of h_65 sits in a tree; under chunk = 4 every hub's does
    hub = fan.hub_of(K) + 1
    liked = [hub, fan.hub_of(200) + 1, twin[9], int(fan.leaves(K)[0]) + 1, fan.r + 1, half[K]]
    disliked = [fan.hub_of(64) + 1, twin[200]]
    with _load(gpu_ctx_factory, graph, chunk) as ctx:
        assert ctx.plan()["nv"] > 0
        for limit in (K - 1, K, K + 1, 1):
            want, (st,), cut = _check(ctx, graph, [], limit, liked, disliked, normalized=True, what="fan chunk %d" % chunk)
            i = sref.id_ints(graph[0]).index(hub)
            assert int(cut[1][i + 1] - cut[1][i]) == min(K, limit)
            # listed = longer than the limit (the graph has no self link).  At 64: h_65, h_66, h_200, their twins and the half twin of
            # h_200; h_65 and its twin are not at 65 and 66
            assert st["listed_rows"] == {64: 7, 65: 5, 66: 3}.get(limit, st["listed_rows"])
            t = sref.id_ints(graph[0]).index(twin[K])
            assert want[t] > 2.0 / 6.0 + 0.1  # the twin shares the whole cut list with the liked hub (2 / 6: a node that shares nothing)


# ---- (2) keys -----------------------------------------------------------------------------------------------------------------------------
def _lcg(self_links=(3, 50, 120, 199), wide=False):
    t = graphs.lcg_graph() + [(v, v) for v in self_links]
    if wide:  # ids that differ only in the high word: one bloom bit for all, the order is the high word's
        t = [(((a + 1) << 64) | 5, ((b + 1) << 64) | 5) for a, b in t]
    return graphs.dense_from_tuples(t)


def test_key_situations(gpu_ctx_factory):
    graph = _lcg()
    ints = sref.id_ints(graph[0])
    liked, disliked = ints[:9] + [3, 50], [ints[30], 120]
    with _load(gpu_ctx_factory, graph) as ctx:
        a, _, _ = _check(ctx, graph, [], 3, liked, disliked, what="no key set")
        keys = [(v, v % 3) for v in ints] + [(1 << 90, 0)]  # equal keys on both sides of every cut
        _set(ctx, keys)
        b, _, _ = _check(ctx, graph, keys, 3, liked, disliked, what="equal keys")
        assert a.tobytes() != b.tobytes()  # a state kept across hb_links_set_keys would answer with `a`
        keys2 = [(v, 1000 - v) for v in ints[::2]]
        _set(ctx, keys2)  # between two limited calls with the same limit
        c, _, _ = _check(ctx, graph, keys2, 3, liked, disliked, what="new keys")
        assert c.tobytes() != b.tobytes()
        _set(ctx, [])
        _check(ctx, graph, [], 3, liked, disliked, what="keys cleared")
    wide = _lcg(wide=True)
    wints = sref.id_ints(wide[0])
    with _load(gpu_ctx_factory, wide, 4) as ctx:
        keys = [(v, 7) for v in wints]
        _set(ctx, keys)
        _check(ctx, wide, keys, 2, wints[:5] + [wints[3] & ((1 << 64) - 1)], wints[40:42], what="high words")


def test_keys_from_ranks(gpu_ctx_factory):
    graph = _lcg()
    ints = sref.id_ints(graph[0])
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        ctx.run()
        ids, _ = ctx.results()
        ranks = ctx.ranks()
        ctx.links_set_keys(from_ranks=True)
        _check(ctx, graph, list(zip(sref.id_ints(ids), ranks.tolist())), 3, ints[5:25], ints[:2], normalized=True, what="ranks")


# ---- (3) limit changes on one context ------------------------------------------------------------------------------------------------------
def test_limit_changes_on_one_context(gpu_ctx_factory):
    graph = _lcg()
    ints = sref.id_ints(graph[0])
    liked, disliked = ints[10:30], ints[3:5]
    with _load(gpu_ctx_factory, graph) as ctx:
        seen = []
        for limit in (4, 2, 0, 4):
            want, (st,), _ = _check(ctx, graph, [], limit, liked, disliked, what="limit change")
            seen.append((want.tobytes(), st))
        assert seen[0][0] == seen[3][0] and len({s[0] for s in seen}) == 3
        assert seen[0][1]["ms_lists"] > 0.0 and seen[1][1]["ms_lists"] > 0.0 and seen[2][1]["ms_lists"] == 0.0
        with _load(gpu_ctx_factory, graph) as fresh:  # a fresh context's answer, for the last one
            fresh.inbound_similarity(ids_from_ints(liked), ids_from_ints(disliked), limit=4)
            _assert_exact(ctx.similarity_all(), fresh.similarity_all(), "fresh context")
        st = ctx.inbound_similarity(ids_from_ints(liked), ids_from_ints(disliked), limit=4)
        assert st["ms_lists"] == 0.0 and st["listed_rows"] == seen[3][1]["listed_rows"] > 0  # the same limit again: the lists are reused


# ---- (4) self links ----------------------------------------------------------------------------------------------------------------------------
def test_self_links(gpu_ctx_factory):
    # S has a self link and three other in-neighbours; 2 sets bloom bit 42, and so would S = 66 itself: with the self link counted the
    # bloom keeps the bit, without it the bit is 2's alone.  T has a self link and 4 other in-neighbours: degree + 1 == limit + 1 at limit 4
    S, T = 66, 130
    assert (21 * S) % 64 == (21 * 2) % 64 == 42 and (21 * T) % 64 == 42
    t = [(1, S), (2, S), (3, S), (S, S), (1, T), (3, T), (4, T), (5, T), (T, T), (1, 9), (3, 9), (4, 9), (S, 9), (T, 9)]
    graph = graphs.dense_from_tuples(t)
    ints = sref.id_ints(graph[0])
    with _load(gpu_ctx_factory, graph) as ctx:
        _, _, cut = _check(ctx, graph, [], 4, [S, T, 9], [1], what="self links")
        _, bloom, length = ctx.debug_similarity_batch()
        assert int(length[ints.index(S)]) == 3 and int(length[ints.index(T)]) == 4 and int(length[ints.index(9)]) == 4
        assert int(bloom[ints.index(T)]) & (1 << 42) == 0 and int(bloom[ints.index(S)]) & (1 << 42)  # T's own bit is gone, 2 keeps S's
        ctx.inbound_similarity(ids_from_ints([S]), limit=0)
        _, bloom0, length0 = ctx.debug_similarity_batch()
        assert int(length0[ints.index(S)]) == 4 and int(length0[ints.index(T)]) == 5 and int(bloom0[ints.index(T)]) & (1 << 42)
        _check(ctx, graph, [], 3, [S, T, 9], [1], what="self links")  # T: degree 4 > 3, cut as well
    # a self link inside the hub's own chunk tree
    fan, graph, twin, half = _fan_graph(self_links=[fans.Fan(FAN_KS).hub_of(65) + 1, fans.Fan(FAN_KS).hub_of(9) + 1])
    hub = fan.hub_of(65) + 1
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        for limit in (66, 65, 64, 8):
            _, (st,), cut = _check(ctx, graph, [], limit, [hub, twin[65], fan.hub_of(9) + 1], [half[65]], what="self link in a tree")
            i = sref.id_ints(graph[0]).index(hub)
            assert int(cut[1][i + 1] - cut[1][i]) == min(65, limit)


# ---- (5) the bloom over the cut entries only ---------------------------------------------------------------------------------------------------
def test_bloom_over_the_cut_entries_only(gpu_ctx_factory):
    """tests/test_similar_hosts.py test_bloom_over_the_512_entries_only: LIKED has 513 in-links, the 512 with the smallest ids all carry
    bloom bit 41, the 513th, FAR, bit 0.  CAND has five in-links with five different bits, among them 41 and 0.  Over the 512 best the
    gate says 4 x 1 < 5: sim 0; with FAR's key the best of all the mask has both bits: 4 x 2 >= 5."""
    LIKED, CAND, FAR = 7, 50000, 40000
    near = [64 * j + 5 for j in range(1, 513)]
    graph = shref.layered({LIKED: near + [FAR]}, {near[0]: [CAND], FAR: [CAND]}, [(40001, CAND), (40002, CAND), (40003, CAND)])
    ints = sref.id_ints(graph[0])
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        want, _, _ = _check(ctx, graph, [], 512, [LIKED], what="gated")
        assert want[ints.index(CAND)] == 0.0
        keys = [(FAR, 0)]
        _set(ctx, keys)
        want, _, _ = _check(ctx, graph, keys, 512, [LIKED], what="not gated")
        assert want[ints.index(CAND)] > 0.0
        whole = lref.numpy_scores(lref.cut_graph(*graph, None, 0), [LIKED], [])
        assert whole[ints.index(CAND)] > 0.0  # the whole in-list holds both bits under any order


# ---- (6) the cross-operator oracle -----------------------------------------------------------------------------------------------------------------
def _small_graph_with_listed_rows():
    """small_graph(33) of tests/test_similar_hosts.py with listed rows among the liked hosts and the candidates: self links on A1, A2 and
    on TALL (the target every source links to), and 520 more sources into TALL, whose in-list is then cut at 512"""
    ids, row_ptr, src = small_graph(33)
    ints = sref.id_ints(ids)
    rp = np.asarray(row_ptr, dtype=np.int64)
    t = [(ints[int(u)], ints[v]) for v in range(len(ints)) for u in src[rp[v]:rp[v + 1]]]
    t += [(A1, A1), (A2, A2), (TALL, TALL)] + [(900000 + j, TALL) for j in range(520)]
    return graphs.dense_from_tuples(t)


@pytest.mark.parametrize("which,count", [("long", 1), ("small", 8), ("small", 33)])
def test_similar_hosts_scores_are_these_scores(gpu_ctx_factory, which, count):
    graph = long_graph() if which == "long" else _small_graph_with_listed_rows()
    ints = sref.id_ints(graph[0])
    keys = small_keys(graph, 3)
    liked = ([A3] if which == "long" else [A1, A2, LONELY, A1, 1 << 99] + list(range(SRC0, SRC0 + 40)))[:count]
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        _set(ctx, keys)
        ctx.similar_hosts(ids_from_ints(liked), 1024)
        ids, scores = ctx.similar_copy()
        assert len(ids) > 3
        _, (st,), _ = _check(ctx, graph, keys, 512, liked, normalized=True, what="oracle")
        assert st["listed_rows"] >= 2  # a liked host and a candidate among them: the limited path, not only the plumbing
        _assert_exact(ctx.similarity_lookup(ids), scores, "hb_similar_hosts against hb_inbound_similarity(limit = 512)")
        _, _, length = ctx.debug_similarity_batch()
        ctx.backlinks(graph[0], 512)
        _, _, _, degrees = ctx.links_copy(ids=False, keys=False)
        assert np.array_equal(length, np.minimum(degrees, 512).astype(np.uint32))
        ids2, scores2 = ctx.similar_copy()  # the operator's result is still there
        assert ids.tobytes() == ids2.tobytes() and scores.tobytes() == scores2.tobytes()


# ---- (7) equivalence with the whole mode ---------------------------------------------------------------------------------------------------------------
def test_large_limit_equals_the_whole_mode(gpu_ctx_factory):
    graph = _lcg(self_links=())
    ints = sref.id_ints(graph[0])
    liked, disliked = ints[:20], ints[50:53]
    top = int(np.diff(np.asarray(graph[1], dtype=np.int64)).max())
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        ctx.inbound_similarity(ids_from_ints(liked), ids_from_ints(disliked), normalized=True)
        whole = ctx.similarity_all(), ctx.debug_similarity_batch()
        for limit in (top, 1024):
            _, (st,), _ = _check(ctx, graph, [], limit, liked, disliked, normalized=True, what="whole")
            assert st["listed_rows"] == 0 and st["list_entries"] == 0
            _assert_exact(ctx.similarity_all(), whole[0], "limit %d against the whole mode" % limit)
            for a, b in zip(ctx.debug_similarity_batch(), whole[1]):
                assert np.array_equal(a, b)
        _, (st,), _ = _check(ctx, graph, [], top - 1, liked, disliked, normalized=True, what="one below")
        assert st["listed_rows"] >= 1


# ---- (8) modes and batches ---------------------------------------------------------------------------------------------------------------------------------
def _entries(ints, L, D, lonely):
    pool = ints[::max(1, len(ints) // 41)] + ints[1::7]
    pool = pool * ((L + D) // len(pool) + 1)
    liked = pool[:L]
    liked[1] = lonely       # an anchor without in-links
    liked[3] = 1 << 100     # no node of the graph
    liked[5] = liked[0]     # a duplicate: a slot of its own
    liked[6] = 3            # a listed anchor: node 3 has a self link
    disliked = pool[L:L + D]
    disliked[0] = liked[0]  # the same id liked and disliked
    if D > 2:
        disliked[2] = (1 << 100) + 1
    return liked, disliked


@pytest.mark.parametrize("L,D", [(15, 2), (30, 3)])
def test_modes_and_batches(gpu_ctx_factory, L, D):
    graph = graphs.dense_from_tuples(graphs.lcg_graph() + [(v, v) for v in (3, 50, 120, 199)] + [(500, 1)])
    ints = sref.id_ints(graph[0])
    liked, disliked = _entries(ints, L, D, lonely=500)
    assert (len(liked) + len(disliked) + 15) // 16 == (2 if L == 15 else 3)
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        keys = [(v, (v * 31) % 11) for v in ints]
        _set(ctx, keys)
        want, (auto, dense, sparse), _ = _check(ctx, graph, keys, 3, liked, disliked, normalized=True, self_score=0.25, modes=(None, "dense", "sparse"), what="modes")
        assert dense["levels_mode"][0] == sum(auto["levels_mode"]) >= 2 and sparse["levels_mode"][0] == 0 and auto["listed_rows"] > 50
        assert dense["rows_nonzero"] == sparse["rows_nonzero"] == auto["rows_nonzero"] > 0
        n = len(ints)
        for k in (1, 10, n + 7):
            for skip in (False, True):
                got_ids, got_vals = ctx.similarity_top(k, skip_anchors=skip)
                order = sref.top_order(graph[0], want, k, skip=liked + disliked if skip else ())
                assert sref.id_ints(got_ids) == [v for _, v in order], (k, skip)
                _assert_exact(got_vals, [s for s, _ in order], "top %d" % k)


# ---- (9) C1-size R-MAT against the numpy form, several pieces of the list builder --------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 4])
def test_c1_rmat(gpu_ctx_factory, chunk):
    g = synth.make_config("C1")[0]
    graph = (np.asarray(g.ids), np.asarray(g.row_ptr), np.asarray(g.src))
    ints = sref.id_ints(graph[0])
    indeg = np.diff(np.asarray(graph[1], dtype=np.int64))
    hubs = np.argsort(-indeg, kind="stable")
    liked = [ints[i] for i in hubs[:6]] + [ints[i] for i in hubs[2000:2012]]
    disliked = [ints[i] for i in hubs[6:8]]
    rng = np.random.default_rng(9)
    keys = list(zip(ints, rng.integers(0, 50, len(ints)).tolist()))
    with _load(gpu_ctx_factory, graph, chunk, tune=(0, _lib.HB_X_SIM_SMALL_PIECES)) as ctx:  # pieces of 64 hosts
        _set(ctx, keys)
        _, (st,), _ = _check(ctx, graph, keys, 8, liked, disliked, normalized=True, what="C1 chunk %d" % chunk)
        assert st["listed_rows"] > 300 and st["batches"] == 2


# ---- (10) refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_the_previous_result(gpu_ctx_factory):
    graph = _lcg()
    ints = sref.id_ints(graph[0])
    liked = ints[:5]
    with _load(gpu_ctx_factory, graph) as ctx:
        want, _, _ = _check(ctx, graph, [], 3, liked, what="before")

        def refused(fn):
            with pytest.raises(_lib.HyperballError) as e:
                fn()
            assert e.value.code == _lib.HB_ERR_INVALID and "hb_inbound_similarity" in str(e.value)
            _assert_exact(ctx.similarity_all(), want, "the previous result after a refusal")
            _check(ctx, graph, [], 3, liked, what="the previous call again")

        refused(lambda: ctx.inbound_similarity(ids_from_ints(liked), limit=1025))
        ctx.begin()
        ctx.step()
        with pytest.raises(_lib.HyperballError) as e:  # between hb_begin and hb_finish
            ctx.inbound_similarity(ids_from_ints(liked), limit=3)
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_inbound_similarity" in str(e.value)
        _assert_exact(ctx.similarity_all(), want, "the previous result after a refusal")
        ctx.finish()
        _check(ctx, graph, [], 3, liked, what="the previous call again")
        # the shorter struct of a caller that does not know the limit: whole in-lists
        o = _lib.HbSimilarityOptions()
        o.struct_size = _lib.HbSimilarityOptions.limit.offset
        o.limit = 3
        arr = ids_from_ints(liked)
        o.liked, o.liked_count = arr.ctypes.data, len(arr)
        st = _lib.HbSimilarityStats()
        st.struct_size = ctypes.sizeof(_lib.HbSimilarityStats)
        ctx._check(ctx.lib.hb_inbound_similarity(ctx.h, ctypes.byref(o), ctypes.byref(st)))
        _assert_exact(ctx.similarity_all(), lref.numpy_scores(lref.cut_graph(*graph, None, 0), liked, []), "old struct_size")
        assert st.listed_rows == 0


# ---- (11) state -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_of_the_other_operators_and_reload(gpu_ctx_factory):
    g = synth.RmatGraph(11, 14_000)
    graph = (np.asarray(g.ids), np.asarray(g.row_ptr), np.asarray(g.src))
    ints = sref.id_ints(graph[0])
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(*graph)
        loaded = ctx.stats()["device_bytes"]
        ctx.run()
        h0 = ctx.state_hash()
        r0 = ctx.results()
        dist_want = dref.bfs(g.n, g.row_ptr, g.src, [11, 500])
        ctx.distances(g.ids[[11, 500]])
        b0 = ctx.betweenness(g.ids[[3, 11, 500]])
        ctx.links_set_keys(from_ranks=True)
        ctx.nearest_seed(from_image=True)
        n0 = ctx.nearest_seed_all()
        ctx.backlinks(g.ids[:50], 5)
        l0 = ctx.links_copy()
        ctx.similar_hosts(g.ids[[7, 11]], 50)
        s0 = ctx.similar_copy()
        before = ctx.stats()["device_bytes"]
        ids, _ = r0
        keys = list(zip(sref.id_ints(ids), ctx.ranks().tolist()))
        liked, disliked = [ints[i] for i in (7, 11, 500, 1000)], [ints[-5]]
        _, (st,), _ = _check(ctx, graph, keys, 4, liked, disliked, normalized=True, what="state")
        assert st["listed_rows"] > 0 and ctx.stats()["device_bytes"] > before
        assert np.array_equal(ctx.distance_all(), dist_want)
        b1 = ctx.betweenness_copy()
        assert b0[0].tobytes() == b1[0].tobytes() and b0[1].tobytes() == b1[1].tobytes()
        r1 = ctx.results()
        assert r0[0].tobytes() == r1[0].tobytes() and r0[1].tobytes() == r1[1].tobytes()
        assert n0.tobytes() == ctx.nearest_seed_all().tobytes()
        l1 = ctx.links_copy()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(l0, l1))
        s1 = ctx.similar_copy()
        assert s0[0].tobytes() == s1[0].tobytes() and s0[1].tobytes() == s1[1].tobytes()
        ctx.forwardlinks(g.ids[:50], 5)
        f0 = ctx.links_copy()
        _check(ctx, graph, keys, 2, liked, disliked, what="state, another limit")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(f0, ctx.links_copy()))
        ctx.run()
        assert ctx.state_hash() == h0
        r2 = ctx.results()
        assert r0[0].tobytes() == r2[0].tobytes() and r0[1].tobytes() == r2[1].tobytes()
        # a reload: the lists are gone with the graph, the first limited call builds them again
        ctx.load_dense(*graph)
        fresh = ctx.stats()["device_bytes"]
        assert fresh == loaded < before  # back at the level of the first load: nothing of the list state is still booked
        with pytest.raises(_lib.HyperballError):
            ctx.similarity_all()
        _, (st2,), _ = _check(ctx, graph, [], 4, liked, disliked, what="after the reload")
        assert st2["ms_lists"] > 0.0 and st2["listed_rows"] > 0
        small = graphs.dense_from_tuples(graphs.lcg_graph(n=70, m=300, seed=3) + [(5, 5)])
        ctx.load_dense(*small)
        assert ctx.stats()["device_bytes"] < fresh
        _, (st3,), _ = _check(ctx, small, [], 4, [1, 2, 5], [4], what="a smaller graph")
        assert st3["ms_lists"] > 0.0 and 0 < st3["listed_rows"] < st2["listed_rows"]


def test_device_bytes_follow_the_list_state(gpu_ctx_factory):
    """the list state is booked when it is built and unbooked when hb_links_set_keys or another limit drops it; a call with limit 0
    keeps it.  The list builder's own holders (the links state: they only grow) are read from hb_links_set_keys' stats."""
    graph = _lcg()
    ints = sref.id_ints(graph[0])
    liked = ids_from_ints(ints[:5])
    keys = [(v, v % 5) for v in ints]
    total = lambda: ctx.stats()["device_bytes"]  # noqa: E731
    with _load(gpu_ctx_factory, graph) as ctx:
        loaded = total()
        st0 = ctx.inbound_similarity(liked, limit=0)
        assert st0["device_bytes"] > 0 and total() == loaded + st0["device_bytes"]
        st4 = ctx.inbound_similarity(liked, limit=4)
        s4 = total()
        lim4 = st4["device_bytes"] - st0["device_bytes"]
        assert lim4 >= _listed(graph, 4)[0] * 4 * 4 + len(ints) * 4 and s4 > loaded + st4["device_bytes"] - 1  # (+ the links state)
        assert ctx.inbound_similarity(liked, limit=0)["device_bytes"] == st4["device_bytes"] and total() == s4  # limit 0 keeps the lists
        _set(ctx, keys)
        k1 = ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))["device_bytes"]
        assert total() == s4 - lim4  # hb_links_set_keys dropped them
        assert ctx.inbound_similarity(liked, limit=0)["device_bytes"] == st0["device_bytes"]
        again = ctx.inbound_similarity(liked, limit=4)
        assert again["ms_lists"] > 0.0 and again["device_bytes"] == st4["device_bytes"] and total() == s4  # the same sizes under any order
        st3 = ctx.inbound_similarity(liked, limit=3)  # another limit: the lists of limit 4 go, those of limit 3 come
        s3 = total()
        lim3 = st3["device_bytes"] - st0["device_bytes"]
        assert st3["ms_lists"] > 0.0 and lim3 > 0 and lim3 != lim4
        k2 = ctx.links_set_keys()["device_bytes"]
        assert total() == s3 - lim3 and (s3 - lim3) - (s4 - lim4) == k2 - k1  # what is left differs by the links state's growth alone
        ctx.load_dense(*graph)
        assert total() == loaded


# ---- (12) the Python mirror ---------------------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(gpu_ctx_factory):
    from stract_amd.inbound_similarity import Scorer
    graph = _lcg()
    ints = sref.id_ints(graph[0])
    with _load(gpu_ctx_factory, graph) as ctx:
        cut = lref.cut_graph(*graph, None, 3)
        want = lref.numpy_scores(cut, [3, 50, 7], [9], True, 0.5)
        s = Scorer.new(ctx, [3, 50, 7], [9], normalized=True, limit=3)
        s.set_self_score(0.5)
        all_ids, all_scores = s.score_all()
        assert all_ids == ints
        _assert_exact(all_scores, want, "score_all")
        _assert_exact(s.score([50, 777777, 3]), [want[ints.index(50)], 1.0 / 3.0, want[ints.index(3)]], "score")
        order = sref.top_order(graph[0], want, 5, skip=[3, 50, 7, 9])
        top_ids, top_vals = s.top(5, skip_anchors=True)
        assert top_ids == [v for _, v in order]
        _assert_exact(top_vals, [x for x, _ in order], "top")
        assert s.stats["listed_rows"] == _listed(graph, 3)[0] > 0
        whole = Scorer.new(ctx, [3, 50, 7], [9], normalized=True)  # the default: limit = 0
        _assert_exact(whole.score_all()[1], lref.numpy_scores(lref.cut_graph(*graph, None, 0), [3, 50, 7], [9], True), "whole")
