"""hb_forwardlinks (HostForwardlinksQuery .. Limit(L), crates/core/src/webgraph/query/forwardlink.rs:183-330) against the host restatement
in tests/forwardlinks_ref.py, and against hb_backlinks on the reversed graph.

Comparison rule: EVERYTHING is exact - offsets, degrees and keys as integers, list entries as node ids, in list order.

The shapes are the smallest that cross every switch of the device code: out-lists of 0 .. 4097 entries on the plain fan of
tests/fans.py (an out-list is cut into segments of 2048 entries: one, two and three of them), targets behind chunk trees of up to six
levels on the flipped fan (every out-edge of a leaf enters its hub's tree at the lowest level), and both at once on a complete
bipartite graph.  In the fans the sid of a node is its index, so the numpy form of the restatement applies directly."""
import ctypes

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import EdgeListGraph, ids_from_ints
from tests import fans
from tests import forwardlinks_ref as fref
from tests import graphs
from tests import links_ref as lref
from tests.test_links import KS, LIMITS, SELF_KS, DIGIT_FLAGS, _chunks, _hash64, _lists, _load, _row_of, _set_keys

pytestmark = pytest.mark.gpu

U64_MAX = fref.U64_MAX
SPREAD, NO_SHORTCUT, KEEP_SELF = _lib.HB_LINKS_SPREAD_ORDS, _lib.HB_LINKS_NO_SHORTCUT, _lib.HB_LINKS_KEEP_SELF
SEGMENT = 2048  # hb_links.hip.h kFwSegment
_FAN = []


def _fan():
    if not _FAN:
        _FAN.append(fans.Fan(Ks=KS))
    return _FAN[0]


def _forward(graph):
    """(ids, out_ptr, dst) of a graph as Context.graph() returns it"""
    return (graph[0],) + fref.out_csr(graph[1], graph[2])


def _want(fgraph, key, qsids, limit, keep_self=False):
    qsids = np.asarray(qsids, dtype=np.int64)
    known = qsids >= 0
    off, to, k, deg = fref.numpy_form(fgraph[1], fgraph[2], key, qsids[known], limit, keep_self)
    lens = np.zeros(len(qsids), dtype=np.int64)
    degrees = np.zeros(len(qsids), dtype=np.int64)
    lens[known] = np.diff(off)
    degrees[known] = deg
    return np.concatenate(([0], np.cumsum(lens))).astype(np.uint64), to, k, degrees.astype(np.uint64)


def _run(ctx, fgraph, key, qsids, limit, flags=0, slots=0, query_ids=None, what=""):
    """one call against the numpy form: offsets, ids, keys and degrees, and the counters of the stats"""
    qsids = np.asarray(qsids, dtype=np.int64)
    if query_ids is None:
        query_ids = fgraph[0][qsids]
    off, to, k, deg = _want(fgraph, key, qsids, limit, bool(flags & KEEP_SELF))
    st = ctx.forwardlinks(query_ids, limit, flags=flags, slots_per_batch=slots)
    got_off, got_ids, got_keys, got_deg = ctx.links_copy()
    assert np.array_equal(got_off, off), (what, limit, flags)
    assert np.array_equal(got_deg, deg), (what, limit, flags)
    bad = np.flatnonzero((got_ids["lo"] != fgraph[0]["lo"][to]) | (got_ids["hi"] != fgraph[0]["hi"][to]))
    assert not len(bad), (what, limit, flags, bad[:5], got_ids["lo"][bad[:5]], fgraph[0]["lo"][to][bad[:5]])
    assert np.array_equal(got_keys, k), (what, limit, flags)
    distinct = np.unique(qsids[qsids >= 0])
    ddeg = dict(zip(qsids.tolist(), deg.tolist()))
    assert st["queries"] == len(qsids) and st["unknown"] == int((qsids < 0).sum()) and st["distinct"] == len(distinct), what
    assert st["entries"] == int(off[-1]) == ctx.links_count()[1] and ctx.links_count()[0] == len(qsids), what
    assert st["edges_gathered"] == sum(ddeg[s] for s in distinct.tolist()), what
    selecting = [s for s in distinct.tolist() if ddeg[s] > limit or ((flags & NO_SHORTCUT) and ddeg[s] > 0)]
    assert st["selected"] == len(selecting), (what, limit, flags, st["selected"], len(selecting))
    raw = np.diff(fgraph[1])[distinct]  # the segments scanned: the whole reader lists, self links included
    assert st["rows_walked"] == int((-(-raw // SEGMENT)).sum()) and (st["device_bytes"] > 0 or not len(distinct)), what
    return st, (got_off, got_ids, got_keys, got_deg)


@pytest.fixture(scope="module")
def loaded(gpu_ctx_factory):
    """loaded(flipped, chunk, self_links) -> (fan, context, forward graph, plan): every variant loaded once for the whole module"""
    cache = {}

    def get(flipped=False, chunk=0, self_links=False):
        key = (flipped, chunk, self_links)
        if key not in cache:
            fan = _fan()
            tuples = fan.tuples(flipped=flipped)
            if self_links:
                tuples += [(fan.hub_of(K) + 1, fan.hub_of(K) + 1) for K in SELF_KS]
            ctx = _load(gpu_ctx_factory, tuples, chunk)
            graph = ctx.graph()
            assert np.array_equal(graph[0]["lo"], np.arange(1, fan.n + 1, dtype=np.uint64)) and not graph[0]["hi"].any()  # sid == node index
            cache[key] = (fan, ctx, _forward(graph), ctx.plan())
        return cache[key]

    yield get
    for _, ctx, _, _ in cache.values():
        ctx.close()


# (1) long out-lists: degree < L, == L, == L + 1 and >> L; one, two and three segments
def _long_out_lists(loaded, flags):
    fan, ctx, fgraph, plan = loaded()
    assert np.array_equal(np.diff(fgraph[1])[fan.hub], np.array(fan.Ks)) and plan["nv"] == 0  # h_K has out-degree K; no chunk row anywhere
    queries = np.concatenate((fan.hub, [fan.r, fan.x, int(fan.leaves(9)[3]), fan.n - 1]))  # (r has the hubs as its out-neighbours; a tip has none)
    for salt in (0, 1):
        key = _hash64(salt, fan.n)
        _set_keys(ctx, fgraph, key)
        for limit in LIMITS:
            st, res = _run(ctx, fgraph, key, queries, limit, flags, what="salt %d" % salt)
            lists = _lists(res)
            for K, lst in zip(KS, lists):  # (what the comparison above already says, spelled out for the hubs)
                leaves = fan.leaves(K)
                best = leaves[np.lexsort((leaves, key[leaves]))][:limit]
                assert lst == (best + 1).tolist(), (K, limit)
            assert st["batches"] == 1 and lists[-1] == []


def test_long_out_lists_and_limits(loaded):
    _long_out_lists(loaded, 0)


# (2) the ascent through the chunk trees: every leaf of the flipped fan links to its hub, and finds it from the bottom of the hub's tree
@pytest.mark.parametrize("chunk", [0, 4])
def test_ascent_through_chunk_trees(loaded, chunk):
    fan, ctx, fgraph, plan = loaded(flipped=True, chunk=chunk)
    row_of = _row_of(fan, plan)
    depth = {K: _chunks(plan, row_of[fan.hub_of(K)])[1] for K in KS}
    if chunk == 0:
        assert all(depth[K] >= 1 for K in KS if K >= 65) and all(depth[K] == 0 for K in KS if K <= 64), depth
    else:
        assert depth[4097] == 6 and all(depth[K] >= 1 for K in KS if K >= 5) and depth[4] == 0, depth
    key = _hash64(8, fan.n)
    _set_keys(ctx, fgraph, key)
    groups = (4097, 4096, 257, 65, 64, 9, 5, 4, 1)
    tips = np.arange(fan.tip_first, fan.n, 97)
    queries = np.concatenate([fan.leaves(K) for K in groups] + [fan.hub, [fan.r, fan.x, fan.r2], tips])
    for limit in (1, 3):
        st, res = _run(ctx, fgraph, key, queries, limit, what="ascent")
        lists, at = _lists(res), 0
        for K in groups:
            assert lists[at:at + K] == [[fan.hub_of(K) + 1]] * K, K  # from six levels down for K = 4097 under chunk = 4
            at += K
        assert lists[at:at + len(KS)] == [[fan.r + 1]] * len(KS) and st["selected"] == 0
        assert all(len(lst) == 1 for lst in lists[-len(tips):])  # a tip links to its leaf


# (3) both at once: 17 sources x 1025 targets, every target a three-level tree under chunk = 4, every out-list one longer than the largest limit
def _bipartite(gpu_ctx_factory, cache=[]):
    if not cache:
        S, T = 17, 1025
        tuples = [(s, S + t) for s in range(1, S + 1) for t in range(1, T + 1)]
        ctx = _load(gpu_ctx_factory, tuples, 4)
        graph = ctx.graph()
        assert np.array_equal(graph[0]["lo"], np.arange(1, S + T + 1, dtype=np.uint64))
        plan = ctx.plan()
        order = plan["order"]
        row_of = np.full(S + T, -1, dtype=np.int64)
        row_of[order[order != 0xFFFFFFFF].astype(np.int64)] = np.flatnonzero(order != 0xFFFFFFFF)
        # three levels: the target's node row and two levels of chunk rows under it (17 > 4 x 4)
        assert all(_chunks(plan, row_of[t])[1] == 2 for t in range(S, S + T)) and len(plan["level_begin"]) == 3
        cache.append((ctx, _forward(graph), row_of, S, T))
    return cache[0]


def _both_at_once(gpu_ctx_factory, flags):
    ctx, fgraph, row_of, S, T = _bipartite(gpu_ctx_factory)
    assert np.array_equal(np.diff(fgraph[1])[:S], np.full(S, T))
    pos = np.argsort(np.argsort(row_of[S:], kind="stable"), kind="stable")  # the targets' place in device-row order
    placements = {"first": pos, "last": T - 1 - pos, "strided": (pos * 513) % T}  # (513 is coprime to 1025: a permutation)
    for name, rank in placements.items():
        assert sorted(rank.tolist()) == list(range(T)), name
        key = np.concatenate((np.full(S, 7, dtype=np.uint64), rank.astype(np.uint64)))
        _set_keys(ctx, fgraph, key)
        for limit in (1, 512, 1024):
            st, res = _run(ctx, fgraph, key, np.arange(S), limit, flags, what=name)
            want = (S + np.argsort(rank, kind="stable")[:limit] + 1).tolist()
            assert _lists(res) == [want] * S and res[2].tolist() == list(range(limit)) * S and st["selected"] == S
    _, res = _run(ctx, fgraph, key, [S, S + T - 1], 3, flags)  # the targets link nowhere
    assert _lists(res) == [[], []]


def test_long_lists_behind_chunk_trees(gpu_ctx_factory):
    _both_at_once(gpu_ctx_factory, 0)


# (4) special entries
def _self_links(loaded, flags):
    # plain fan: the hub's self link is one of K + 1 node rows in its reader list
    fan, ctx, fgraph, plan = loaded(self_links=True)
    key = (_hash64(5, fan.n) | np.uint64(1)) + np.uint64(1)  # at least 2
    for K in SELF_KS:
        key[fan.hub_of(K)] = 0  # the smallest key of all
    _set_keys(ctx, fgraph, key)
    for K in (5, 65, 4097):
        hub, leaves = fan.hub_of(K), fan.leaves(K)
        best = (leaves[np.lexsort((leaves, key[leaves]))] + 1).tolist()
        for limit in (1, 2, min(K, 1024)):
            st, res = _run(ctx, fgraph, key, [hub], limit, flags, what="self dropped")
            assert _lists(res)[0] == best[:limit] and int(res[3][0]) == K
            assert st["selected"] == (1 if K > limit or flags & NO_SHORTCUT else 0)
            st, res = _run(ctx, fgraph, key, [hub], limit, flags | KEEP_SELF, what="self kept")
            assert _lists(res)[0] == ([hub + 1] + best)[:limit] and int(res[3][0]) == K + 1 and int(res[2][0]) == 0
    _, res = _run(ctx, fgraph, key, [fan.hub_of(0), fan.hub_of(1)], 3, flags)
    assert _lists(res) == [[], [int(fan.leaves(1)[0]) + 1]] and res[3].tolist() == [0, 1]
    _, res = _run(ctx, fgraph, key, [fan.hub_of(0), fan.hub_of(1)], 3, flags | KEEP_SELF)
    assert _lists(res) == [[fan.hub_of(0) + 1], [fan.hub_of(1) + 1, int(fan.leaves(1)[0]) + 1]] and res[3].tolist() == [1, 2]
    # flipped fan under chunk = 4: the hub's self link enters the hub's OWN chunk tree - the entry is a chunk row, the target the hub
    fan, ctx, fgraph, plan = loaded(flipped=True, chunk=4, self_links=True)
    _set_keys(ctx, fgraph, key)
    for K in (5, 65, 4097):
        hub = fan.hub_of(K)
        assert _chunks(plan, _row_of(fan, plan)[hub])[1] >= 1
        _, res = _run(ctx, fgraph, key, [hub], 2, flags, what="self behind a tree")
        assert _lists(res)[0] == [fan.r + 1] and int(res[3][0]) == 1
        _, res = _run(ctx, fgraph, key, [hub], 2, flags | KEEP_SELF, what="self behind a tree, kept")
        assert _lists(res)[0] == [hub + 1, fan.r + 1] and int(res[3][0]) == 2


def test_self_links(loaded):
    _self_links(loaded, 0)


def test_equal_keys_around_the_cut(loaded):
    fan, ctx, fgraph, plan = loaded()
    leaves = fan.leaves(4097)
    base = _hash64(3, fan.n) | np.uint64(1 << 40)
    tied = [int(leaves[4000]), int(leaves[2047]), int(leaves[2048])]  # in the last, the first and the second segment
    key = base.copy()
    key[tied] = 5
    key[leaves[3]] = 1
    key[leaves[4096]] = 2
    _set_keys(ctx, fgraph, key)
    for limit in (3, 4, 5, 6):  # the cut before, inside and behind the three tied entries
        _, res = _run(ctx, fgraph, key, [fan.hub_of(4097)], limit, what="tie")
        want = [int(leaves[3]), int(leaves[4096])] + sorted(tied)
        assert _lists(res)[0][:5] == [v + 1 for v in want[:limit]]
    key = _hash64(9, fan.n) % np.uint64(50)  # ties all over
    _set_keys(ctx, fgraph, key)
    for limit in (1, 49, 50, 51, 1024):
        _run(ctx, fgraph, key, fan.hub, limit, what="ties all over")


def _literal_check(ctx, graph, keys, queries, limit, flags=0, slots=0):
    """a small graph against the literal restatement; keys: [(node, key)], queries: [node]"""
    lists, degrees, unknown_keys, unknown = fref.literal(*graph, keys, queries, limit, bool(flags & KEEP_SELF))
    st = ctx.forwardlinks(ids_from_ints(queries), limit, flags=flags, slots_per_batch=slots)
    off, ids, got_keys, deg = ctx.links_copy()
    assert _lists((off, ids, got_keys, deg)) == [[u for u, _ in lst] for lst in lists]
    assert got_keys.tolist() == [k for lst in lists for _, k in lst] and deg.tolist() == degrees and st["unknown"] == unknown
    return lists, st


def test_ties_on_wide_ids_and_no_key_set(gpu_ctx_factory):
    """128-bit ids that differ only in the high word: a tie goes to the smaller NodeID; before any hb_links_set_keys every key is u64::MAX"""
    rng = np.random.default_rng(23)
    nodes = [(hi << 64) | 5 for hi in range(1, 41)]
    edges = sorted({(nodes[int(a)], nodes[int(b)]) for a, b in rng.integers(0, 40, (300, 2))})
    with _load(gpu_ctx_factory, edges) as ctx:
        graph = ctx.graph()
        assert lref.id_ints(graph[0]) == nodes
        for limit in (1, 3, 1024):
            lists, _ = _literal_check(ctx, graph, [], nodes, limit)  # without any hb_links_set_keys call
            assert all([u for u, _ in lst] == sorted(u for u, _ in lst) for lst in lists) and all(k == U64_MAX for lst in lists for _, k in lst)
        keys = [(v, i % 3) for i, v in enumerate(nodes)]
        st = ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
        assert st["listed"] == 40
        for limit in (1, 3, 1024):
            _literal_check(ctx, graph, keys, nodes, limit)
            _literal_check(ctx, graph, keys, nodes, limit, KEEP_SELF)


def test_u64_max_is_a_key(gpu_ctx_factory):
    edges = [(9, 3), (9, 4), (9, 5), (2, 1), (7, 6), (7, 8)]
    with _load(gpu_ctx_factory, edges) as ctx:
        graph = ctx.graph()
        keys = [(3, U64_MAX), (4, U64_MAX - 1), (6, U64_MAX), (77, 1), (4, 0), (4, U64_MAX - 1)]  # listed u64::MAX, an unknown id, duplicates
        st = ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
        assert st["listed"] == 3 and st["unknown_keys"] == 1
        lists, _ = _literal_check(ctx, graph, keys, [9, 7, 2], 3)
        assert lists == [[(4, U64_MAX - 1), (3, U64_MAX), (5, U64_MAX)], [(6, U64_MAX), (8, U64_MAX)], [(1, U64_MAX)]]
        lists, _ = _literal_check(ctx, graph, keys, [9, 7], 1)
        assert lists == [[(4, U64_MAX - 1)], [(6, U64_MAX)]]


# (5) the debug flags change nothing
@pytest.mark.parametrize("flags", DIGIT_FLAGS)
def test_digit_flags_change_nothing_on_long_out_lists(loaded, flags):
    _long_out_lists(loaded, flags)


@pytest.mark.parametrize("flags", DIGIT_FLAGS)
def test_digit_flags_change_nothing_behind_chunk_trees(gpu_ctx_factory, flags):
    _both_at_once(gpu_ctx_factory, flags)


@pytest.mark.parametrize("flags", DIGIT_FLAGS)
def test_digit_flags_change_nothing_on_self_links(loaded, flags):
    _self_links(loaded, flags)


# (6) batches and queries
def test_batches(loaded):
    fan, ctx, fgraph, plan = loaded(flipped=True, chunk=4, self_links=True)
    key = _hash64(9, fan.n) % np.uint64(50)  # ties all over
    _set_keys(ctx, fgraph, key)
    rng = np.random.default_rng(5)
    qsids = np.concatenate((fan.hub, rng.integers(0, fan.n, 260), fan.hub[::3], [-1] * 17))
    rng.shuffle(qsids)
    qsids = np.concatenate((qsids[:299], [fan.n - 1]))  # the last query is the highest sid: the last slot of the last batch
    assert len(qsids) == 300 and (qsids < 0).any() and len(np.unique(qsids)) < 290
    query_ids = np.zeros(300, dtype=_lib.U128)
    query_ids["lo"] = np.where(qsids >= 0, qsids + 1, fan.n + 1000 + np.arange(300)).astype(np.uint64)
    distinct = len(np.unique(qsids[qsids >= 0]))
    results = []
    for slots in (0, 1, 7, 64):
        st, res = _run(ctx, fgraph, key, qsids, 5, slots=slots, query_ids=query_ids, what="slots %d" % slots)
        assert st["batches"] == (1 if slots == 0 else -(-distinct // slots))
        results.append(tuple(a.tobytes() for a in res))
        assert len(_lists(res)[-1]) == 1  # a tip links to its leaf
    assert all(r == results[0] for r in results)
    # the same on long lists: the plain fan, whose hubs span several segments, a hub per batch and seven
    fan, ctx, fgraph, plan = loaded()
    key = _hash64(4, fan.n)
    _set_keys(ctx, fgraph, key)
    qs = np.concatenate((fan.hub, [fan.r, -1, fan.hub_of(4097)]))
    ids = np.zeros(len(qs), dtype=_lib.U128)
    ids["lo"] = np.where(qs >= 0, qs + 1, fan.n + 5).astype(np.uint64)
    results = [tuple(a.tobytes() for a in _run(ctx, fgraph, key, qs, 64, slots=slots, query_ids=ids)[1]) for slots in (0, 1, 7, 64)]
    assert all(r == results[0] for r in results)
    st = ctx.forwardlinks(np.zeros(0, dtype=_lib.U128), 5)
    off, ids, keys, deg = ctx.links_copy()
    assert st["queries"] == 0 and st["batches"] == 0 and off.tolist() == [0] and len(ids) == len(keys) == len(deg) == 0 and ctx.links_count() == (0, 0)


# (7) an independent oracle: the backlinks of the reversed graph, loaded in a second context with the same keys
def _against_reversed(gpu_ctx_factory, graph, key, queries, limits, chunk=0):
    out_ptr, dst = fref.out_csr(graph[1], graph[2])
    listed = np.flatnonzero(key != np.uint64(U64_MAX))
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk) as fwd, gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk) as rev:
        fwd.load_dense(*graph)
        rev.load_dense(graph[0], out_ptr.astype(np.uint64), dst.astype(np.uint32))
        for ctx in (fwd, rev):
            ctx.links_set_keys(graph[0][listed], key[listed])
        for limit in limits:
            for flags in (0, KEEP_SELF):
                a = fwd.forwardlinks(queries, limit, flags=flags)
                got = tuple(x.tobytes() for x in fwd.links_copy())
                b = rev.backlinks(queries, limit, flags=flags)
                assert got == tuple(x.tobytes() for x in rev.links_copy()), (limit, flags)
                assert all(a[f] == b[f] for f in ("queries", "unknown", "distinct", "entries", "edges_gathered", "selected")) and a["entries"] > 0
        return fwd.stats()["virtual_rows"], rev.stats()["virtual_rows"]


def test_against_backlinks_of_the_reversed_graph_lcg(gpu_ctx_factory):
    graph = graphs.dense_from_tuples(graphs.lcg_graph() + [(7, 7), (1000, 1), (1000, 1000)])
    n = len(graph[0])
    key = _hash64(4, n) % np.uint64(7)
    key[:5] = U64_MAX
    queries = np.concatenate((graph[0], ids_from_ints([5555]), graph[0][:3]))
    vf, vr = _against_reversed(gpu_ctx_factory, graph, key, queries, (1, 3, 1024), chunk=4)
    assert vf > 0 and vr > 0  # chunk trees on both sides


def test_against_backlinks_of_the_reversed_graph_rmat(gpu_ctx_factory):
    g = synth.make_config("C1")[0]
    graph = (np.asarray(g.ids), np.asarray(g.row_ptr), np.asarray(g.src))
    key = _hash64(6, g.n) % np.uint64(1000)
    key[::9] = U64_MAX
    outdeg = np.diff(fref.out_csr(graph[1], graph[2])[0])
    top = np.argsort(-outdeg, kind="stable")[:64]
    assert int(outdeg[top].min()) > 16 and int(outdeg[top].max()) > 512  # some lists are cut at every limit
    queries = np.concatenate((graph[0][top], graph[0][::5]))
    _against_reversed(gpu_ctx_factory, graph, key, queries, (1, 16, 512))


# (8) refusals: each leaves the previous result as it was
def _raw(ctx, **fields):
    o = _lib.HbLinksOptions()
    o.struct_size = ctypes.sizeof(_lib.HbLinksOptions)
    o.limit = 3
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        setattr(o, k, v)
    st = _lib.HbLinksStats()
    st.struct_size = ctypes.sizeof(_lib.HbLinksStats)
    ctx._check(ctx.lib.hb_forwardlinks(ctx.h, ctypes.byref(o), ctypes.byref(st)))


_ONE_ID = ids_from_ints([1])
REFUSALS = {
    "limit 0": lambda ctx: ctx.forwardlinks(_ONE_ID, 0),
    "limit 1025": lambda ctx: ctx.forwardlinks(_ONE_ID, 1025),
    "slots above 65536": lambda ctx: ctx.forwardlinks(_ONE_ID, 3, slots_per_batch=65537),
    "nodes NULL": lambda ctx: _raw(ctx, node_count=1),
    "opt NULL": lambda ctx: ctx._check(ctx.lib.hb_forwardlinks(ctx.h, None, None)),
    "open run": lambda ctx: ctx.forwardlinks(_ONE_ID, 3),
}


@pytest.mark.parametrize("previous", ["forward", "backward"])
@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusal_keeps_the_previous_result(gpu_ctx_factory, which, previous):
    with _load(gpu_ctx_factory, graphs.lcg_graph(n=40, m=160, seed=9)) as ctx:
        graph = ctx.graph()
        nodes = lref.id_ints(graph[0])
        keys = [(v, v % 3) for v in nodes]
        ctx.links_set_keys(ids_from_ints(nodes), np.array([k for _, k in keys], dtype=np.uint64))

        def query():
            if previous == "forward":
                _literal_check(ctx, graph, keys, nodes[::2] + [999], 3)
            else:
                ctx.backlinks(ids_from_ints(nodes[::2] + [999]), 3)

        query()
        before = tuple(a.tobytes() for a in ctx.links_copy()) + ctx.links_count()
        if "open run" in which:
            ctx.begin()
        with pytest.raises(_lib.HyperballError) as e:
            REFUSALS[which](ctx)
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_forwardlinks" in str(e.value), which
        if "open run" in which:
            ctx.finish()
        assert tuple(a.tobytes() for a in ctx.links_copy()) + ctx.links_count() == before, which
        query()  # the keys are the ones set before the refusal, too
        assert tuple(a.tobytes() for a in ctx.links_copy()) + ctx.links_count() == before, which


def test_refusals_of_the_entry(gpu_ctx_factory):
    def refused(fn, who):
        with pytest.raises(_lib.HyperballError) as e:
            fn()
        assert e.value.code == _lib.HB_ERR_INVALID and who in str(e.value)

    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        refused(lambda: ctx.forwardlinks(_ONE_ID, 3), "hb_forwardlinks")  # no graph loaded
        ctx.load_edges(np.zeros(0, dtype=_lib.EDGE))  # an empty graph: every query is unknown
        st = ctx.forwardlinks(ids_from_ints([1, 2]), 3)
        assert st["unknown"] == 2 and st["entries"] == 0 and ctx.links_copy()[0].tolist() == [0, 0, 0]
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        refused(lambda: ctx.forwardlinks(_ONE_ID, 3), "hb_forwardlinks")


# (9) the neighbours: nothing of theirs moves, the backlinks answer as before, a reload starts afresh
def test_neighbours_and_reload(gpu_ctx_factory):
    g = synth.RmatGraph(11, 14_000)
    graph = (g.ids, g.row_ptr, g.src)
    fgraph = _forward(graph)
    key = _hash64(6, g.n) % np.uint64(1000)
    liked = g.ids[[7, 11, 500]]
    outdeg = np.diff(fgraph[1])
    qsids = np.concatenate((np.argsort(-outdeg, kind="stable")[:40], np.arange(0, g.n, 37)))
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(*graph)
        ctx.run()
        h0, r0 = ctx.state_hash(), ctx.results()
        d0 = ctx.distances(g.ids[[11, 500]])[:2]
        b0 = ctx.betweenness(g.ids[[3, 11, 500]])[:2]
        ctx.inbound_similarity(liked)
        s0 = ctx.similarity_all()
        ctx.nearest_seed(g.ids[::5], np.arange(len(g.ids[::5])) / 16.0, g.ids, key, discount_factor=0.5, rounds=3)
        n0 = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes())
        ctx.run()
        assert ctx.state_hash() == h0
        _set_keys(ctx, fgraph, key)
        ctx.backlinks(g.ids[qsids], 16)
        back = tuple(a.tobytes() for a in ctx.links_copy())
        before = ctx.stats()["device_bytes"]
        st, res = _run(ctx, fgraph, key, qsids, 16, what="first call")
        assert st["selected"] > 0 and ctx.stats()["device_bytes"] >= before + 4 * ctx.stats()["virtual_rows"]  # the table of tops is booked
        mine = tuple(a.tobytes() for a in res)
        assert mine != back

        def still_mine():
            assert tuple(a.tobytes() for a in ctx.links_copy()) == mine

        # what the others left is untouched by the call ...
        assert ctx.state_hash() == h0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.distance_copy(), d0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.betweenness_copy(), b0))
        assert ctx.similarity_all().tobytes() == s0.tobytes()
        assert (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes()) == n0
        # ... and each of them computes what it computed before, and leaves the forward result readable
        ctx.run()
        assert ctx.state_hash() == h0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        still_mine()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.distances(g.ids[[11, 500]])[:2], d0))
        still_mine()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.betweenness(g.ids[[3, 11, 500]])[:2], b0))
        still_mine()
        ctx.inbound_similarity(liked)
        assert ctx.similarity_all().tobytes() == s0.tobytes()
        still_mine()
        ctx.nearest_seed(g.ids[::5], np.arange(len(g.ids[::5])) / 16.0, g.ids, key, discount_factor=0.5, rounds=3)
        assert (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes()) == n0
        still_mine()
        # the backlinks answer what they answered before, and the forward links after them
        ctx.backlinks(g.ids[qsids], 16)
        assert tuple(a.tobytes() for a in ctx.links_copy()) == back
        ctx.begin()
        ctx.step()
        ctx.finish()
        st2, res2 = _run(ctx, fgraph, key, qsids, 16, what="second call")
        assert tuple(a.tobytes() for a in res2) == mine and st2["device_bytes"] == st["device_bytes"]
        ctx.run()
        assert ctx.state_hash() == h0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        # a second load: neither the keys, the table of tops nor the result of the first graph answer for the new one
        tuples = graphs.lcg_graph(n=70, m=300, seed=3)
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        with pytest.raises(_lib.HyperballError) as e:
            ctx.links_count()
        assert e.value.code == _lib.HB_ERR_INVALID
        sgraph = ctx.graph()
        snodes = lref.id_ints(sgraph[0])
        lists, st3 = _literal_check(ctx, sgraph, [], snodes, 4)  # NodeID order: no key survived the load
        assert all([u for u, _ in lst] == sorted(u for u, _ in lst) for lst in lists) and all(k == U64_MAX for lst in lists for _, k in lst)
        assert 0 < st3["device_bytes"] < st["device_bytes"]


def test_context_without_sweep_support(gpu_ctx_factory):
    """HB_FLAG_NO_SPARSE: the transpose does not exist after the load; the first call builds it"""
    tuples = _fan().tuples(flipped=True)
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS | _lib.HB_FLAG_NO_SPARSE, chunk=4) as ctx:
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        fan = _fan()
        fgraph = _forward(ctx.graph())
        key = _hash64(1, fan.n)
        kst = _set_keys(ctx, fgraph, key)
        before = ctx.stats()["device_bytes"]
        queries = np.concatenate((fan.leaves(4097)[::64], fan.hub, [fan.r]))
        st, res = _run(ctx, fgraph, key, queries, 3, what="no sweep support")
        own = st["device_bytes"] - kst["device_bytes"]  # what the operator's holders grew by; the rest is the transpose
        assert ctx.stats()["device_bytes"] - before >= own + 4 * len(fgraph[2]) and _lists(res)[0] == [fan.hub_of(4097) + 1]
        st2, res2 = _run(ctx, fgraph, key, queries, 3, what="second call")
        assert tuple(a.tobytes() for a in res2) == tuple(a.tobytes() for a in res)
        ctx.run()
        _run(ctx, fgraph, key, queries, 3, what="after a run")


# (10) the Python mirror
def test_python_mirror(gpu_ctx_factory):
    from stract_amd import forwardlinks
    tuples = graphs.lcg_graph() + [(7, 7)]
    with _load(gpu_ctx_factory, tuples) as ctx:
        graph = ctx.graph()
        nodes = lref.id_ints(graph[0])
        keys = [(v, (v * 7) % 5) for v in nodes[3:]]
        st = forwardlinks.set_link_keys(ctx, [v for v, _ in keys], [k for _, k in keys])
        assert st["listed"] == len(keys)
        queries = nodes[::3] + [7, 12345, 7]
        for keep_self in (False, True):
            lists, degrees, _, _ = fref.literal(*graph, keys, queries, 4, keep_self)
            off, ids, got_keys, deg = forwardlinks.host_forwardlinks(ctx, queries, 4, keep_self=keep_self)
            assert _lists((off, ids, got_keys, deg)) == [[u for u, _ in lst] for lst in lists]
            assert got_keys.tolist() == [k for lst in lists for _, k in lst] and deg.tolist() == degrees
        ctx.run()
        assert forwardlinks.set_link_keys_from_ranks(ctx)["listed"] == len(ctx.results()[0])
        off, ids, got_keys, deg = forwardlinks.host_forwardlinks(ctx, graph[0][:10], 2)
        ranks = dict(zip(lref.id_ints(ctx.results()[0]), ctx.ranks().tolist()))
        assert got_keys.tolist() == [ranks.get(u, U64_MAX) for u in lref.id_ints(ids)]
