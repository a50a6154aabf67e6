"""hb_links_set_keys / hb_backlinks (HostBacklinksQuery .. Limit(L), crates/core/src/webgraph/query/backlink.rs:230-360) against the host
restatement in tests/links_ref.py.

Comparison rule: EVERYTHING is exact - offsets, degrees and keys as integers, list entries as node ids, in list order.

The list-length, position, self-link, tie and digit tests run on the flipped fan of tests/fans.py, whose in-lists carry the lengths:
the hub h_K has its K leaves as in-neighbours, under the default chunk and under chunk = 4 (a six-level tree at 4097).  Positions
inside a hub's list are taken from the plan, not from the leaf numbers: the planner permutes rows.  In the fan the sid of a node is its
index, so the numpy form of the restatement (equal to the literal one: tests/test_links_ref.py) applies directly."""
import ctypes

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import EdgeListGraph, ids_from_ints
from tests import fans
from tests import graphs
from tests import links_ref as lref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
U64_MAX = lref.U64_MAX
KS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
SELF_KS = (0, 1, 5, 65, 4097)  # hubs that get a self link (0: then its only in-neighbour is itself)
LIMITS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024)
SPREAD, NO_SHORTCUT, KEEP_SELF = _lib.HB_LINKS_SPREAD_ORDS, _lib.HB_LINKS_NO_SHORTCUT, _lib.HB_LINKS_KEEP_SELF
DIGIT_FLAGS = (SPREAD, NO_SHORTCUT, SPREAD | NO_SHORTCUT)
_FAN = []


def _fan():
    if not _FAN:
        _FAN.append(fans.Fan(Ks=KS))
    return _FAN[0]


def _hash64(salt, count):
    """splitmix64 of (salt, node index + 1) as a uint64 array: the smallest keys of a list land at arbitrary positions"""
    with np.errstate(over="ignore"):
        z = np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(salt) + 1) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _load(factory, tuples, chunk=0):
    ctx = factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk)
    ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
    return ctx


def _set_keys(ctx, graph, key):
    """the key of every sid, u64::MAX = not listed"""
    key = np.asarray(key, dtype=np.uint64)
    listed = np.flatnonzero(key != np.uint64(U64_MAX))
    st = ctx.links_set_keys(graph[0][listed], key[listed])
    assert st["listed"] == len(listed) and st["unknown_keys"] == 0 and (st["device_bytes"] > 0 or not len(graph[0]))
    return st


def _sids(graph, ids):
    """sid of every id of `ids`, an ascending subset of the graph's ids"""
    n, k = len(graph[0]), len(ids)
    hi = np.concatenate((graph[0]["hi"], ids["hi"]))
    lo = np.concatenate((graph[0]["lo"], ids["lo"]))
    tag = np.concatenate((np.zeros(n, dtype=np.int8), np.ones(k, dtype=np.int8)))
    order = np.lexsort((tag, lo, hi))  # every id of the subset directly behind its equal
    sub = tag[order] == 1
    sids = (np.cumsum(~sub) - 1)[sub]
    assert graph[0][sids].tobytes() == np.ascontiguousarray(ids).tobytes()
    return sids.astype(np.int64)


def _want(graph, key, qsids, limit, keep_self=False):
    qsids = np.asarray(qsids, dtype=np.int64)
    known = qsids >= 0
    off, frm, k, deg = lref.numpy_form(graph[1], graph[2], key, qsids[known], limit, keep_self)
    lens = np.zeros(len(qsids), dtype=np.int64)
    degrees = np.zeros(len(qsids), dtype=np.int64)
    lens[known] = np.diff(off)
    degrees[known] = deg
    return np.concatenate(([0], np.cumsum(lens))).astype(np.uint64), frm, k, degrees.astype(np.uint64)


def _run(ctx, graph, key, qsids, limit, flags=0, slots=0, query_ids=None, what=""):
    """one call against the numpy form: offsets, ids, keys and degrees, and the counters of the stats"""
    qsids = np.asarray(qsids, dtype=np.int64)
    if query_ids is None:
        query_ids = graph[0][qsids]
    keep_self = bool(flags & KEEP_SELF)
    off, frm, k, deg = _want(graph, key, qsids, limit, keep_self)
    st = ctx.backlinks(query_ids, limit, flags=flags, slots_per_batch=slots)
    got_off, got_ids, got_keys, got_deg = ctx.links_copy()
    assert np.array_equal(got_off, off), (what, limit, flags)
    assert np.array_equal(got_deg, deg), (what, limit, flags)
    bad = np.flatnonzero((got_ids["lo"] != graph[0]["lo"][frm]) | (got_ids["hi"] != graph[0]["hi"][frm]))
    assert not len(bad), (what, limit, flags, bad[:5], got_ids["lo"][bad[:5]], graph[0]["lo"][frm][bad[:5]])
    assert np.array_equal(got_keys, k), (what, limit, flags)
    distinct = np.unique(qsids[qsids >= 0])
    ddeg = dict(zip(qsids.tolist(), deg.tolist()))
    assert st["queries"] == len(qsids) and st["unknown"] == int((qsids < 0).sum()) and st["distinct"] == len(distinct), what
    assert st["entries"] == int(off[-1]) == ctx.links_count()[1] and ctx.links_count()[0] == len(qsids), what
    assert st["edges_gathered"] == sum(ddeg[s] for s in distinct.tolist()), what
    selecting = [s for s in distinct.tolist() if ddeg[s] > limit or ((flags & NO_SHORTCUT) and ddeg[s] > 0)]
    assert st["selected"] == len(selecting), (what, limit, flags, st["selected"], len(selecting))
    assert st["rows_walked"] >= len(distinct) and (st["device_bytes"] > 0 or not len(distinct))
    return st, (got_off, got_ids, got_keys, got_deg)


def _lists(res):
    off, ids, keys, _ = res
    ints = lref.id_ints(ids)
    return [ints[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


@pytest.fixture(scope="module")
def loaded(gpu_ctx_factory):
    """loaded(chunk, self_links) -> (fan, context, graph, plan): the flipped fan, every variant loaded once for the whole module"""
    cache = {}

    def get(chunk=0, self_links=False):
        key = (chunk, self_links)
        if key not in cache:
            fan = _fan()
            tuples = fan.tuples(flipped=True)
            if self_links:
                tuples += [(fan.hub_of(K) + 1, fan.hub_of(K) + 1) for K in SELF_KS]
            ctx = _load(gpu_ctx_factory, tuples, chunk)
            graph = ctx.graph()
            assert np.array_equal(graph[0]["lo"], np.arange(1, fan.n + 1, dtype=np.uint64)) and not graph[0]["hi"].any()  # sid == node index
            cache[key] = (fan, ctx, graph, ctx.plan())
        return cache[key]

    yield get
    for _, ctx, _, _ in cache.values():
        ctx.close()


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _row_of(fan, plan):
    order = plan["order"]
    row_of = np.full(fan.n, -1, dtype=np.int64)
    row_of[order[order != NONE].astype(np.int64)] = np.flatnonzero(order != NONE)
    assert (row_of >= 0).all()
    return row_of


def _entries(plan, row):
    rp = plan["row_ptr"].astype(np.int64)
    e = plan["src"][rp[row]:rp[row + 1]]
    return e[e != NONE].astype(np.int64)


def _chunks(plan, row):
    """the list of `row` in list order as its lowest-level chunks: [[node rows of the first chunk], ...] (a list that is no tree: one
    chunk); and the depth of the tree (0 = none)"""
    e = _entries(plan, row)
    if not len(e) or (e < plan["n_pad"]).all():
        return [e.tolist()], 0
    assert (e >= plan["n_pad"]).all()
    out, depth = [], 0
    for v in e.tolist():
        sub, d = _chunks(plan, v)
        out += sub
        depth = max(depth, d + 1)
    return out, depth


def _hub_list(fan, plan, K, self_link=False):
    """the chunks of h_K's list as NODE indices"""
    chunks, depth = _chunks(plan, _row_of(fan, plan)[fan.hub_of(K)])
    chunks = [[int(plan["order"][r]) for r in ch] for ch in chunks]
    flat = sorted(v for ch in chunks for v in ch)
    assert flat == sorted(fan.leaves(K).tolist() + ([fan.hub_of(K)] if self_link else [])), K
    return chunks, depth


# (1) list lengths x limits: degree < L, == L, == L + 1 and >> L on flat rows and on trees
def _list_lengths(loaded, chunk, flags):
    fan, ctx, graph, plan = loaded(chunk)
    assert np.array_equal(np.diff(graph[1].astype(np.int64))[fan.hub], np.array(fan.Ks))
    depth = {K: _hub_list(fan, plan, K)[1] for K in KS}
    if chunk == 0:
        assert all(depth[K] >= 1 for K in KS if K >= 65) and all(depth[K] == 0 for K in KS if K <= 64), depth
    else:
        assert depth[4097] == 6 and all(depth[K] >= 1 for K in KS if K >= 5) and depth[4] == 0, depth
    queries = np.concatenate((fan.hub, [fan.r, fan.x, int(fan.leaves(9)[3])]))  # (r has the hubs as its in-neighbours)
    for salt in (0, 1):
        key = _hash64(salt, fan.n)
        _set_keys(ctx, graph, key)
        for limit in LIMITS:
            st, res = _run(ctx, graph, key, queries, limit, flags, what="salt %d" % salt)
            lists = _lists(res)
            for K, lst in zip(KS, lists):  # (what the comparison above already says, spelled out for the hubs)
                leaves = fan.leaves(K)
                best = leaves[np.lexsort((leaves, key[leaves]))][:limit]
                assert lst == (best + 1).tolist(), (K, limit)
            assert st["batches"] == 1


@pytest.mark.parametrize("chunk", [0, 4])
def test_list_lengths_and_limits(loaded, chunk):
    _list_lengths(loaded, chunk, 0)


# (2) where the kept entries sit in the hub's list
def _placements(chunks):
    first, last = chunks[0], chunks[-1]
    out = {"first chunk": first[:4], "ragged last chunk": last[:4], "one per chunk": [ch[i % len(ch)] for i, ch in enumerate(chunks[:24])]}
    if len(chunks) > 1:
        out["straddling"] = first[-2:] + chunks[1][:2]
    return out


@pytest.mark.parametrize("chunk", [0, 4])
def test_where_the_kept_entries_sit(loaded, chunk):
    fan, ctx, graph, plan = loaded(chunk)
    base = (_hash64(11, fan.n) | np.uint64(1 << 40))  # far above the placed keys
    for K in (65, 4097):
        chunks, _ = _hub_list(fan, plan, K)
        assert len(chunks) >= 2 and len(chunks[-1]) < len(chunks[0])  # a ragged last chunk
        seen = 0
        for name, placed in _placements(chunks).items():
            key = base.copy()
            L = len(placed)
            rank = (np.arange(L) * 7 + 3) % L if L > 1 else np.zeros(1, dtype=np.int64)  # (7 is coprime to every L here: a permutation)
            assert sorted(rank.tolist()) == list(range(L)), (name, L)
            key[placed] = rank.astype(np.uint64)
            _set_keys(ctx, graph, key)
            _, res = _run(ctx, graph, key, [fan.hub_of(K)], L, what=name)
            want = [placed[int(np.flatnonzero(rank == j)[0])] + 1 for j in range(L)]
            assert _lists(res)[0] == want and res[2].tolist() == list(range(L)), (K, name)
            seen += 1
        assert seen == 4


# (3) self links: the hub carries the smallest key of all
def _self_links(loaded, chunk, flags):
    fan, ctx, graph, plan = loaded(chunk, self_links=True)
    key = (_hash64(5, fan.n) | np.uint64(1)) + np.uint64(1)  # at least 2
    runner = {}
    for K in SELF_KS:
        key[fan.hub_of(K)] = 0  # the smallest key of all
    for K in (5, 65, 4097):
        chunks, _ = _hub_list(fan, plan, K, self_link=True)
        mine = next(i for i, ch in enumerate(chunks) if fan.hub_of(K) in ch)
        others = [v for i, ch in enumerate(chunks) if i != mine for v in ch] or [v for v in chunks[mine] if v != fan.hub_of(K)]
        runner[K] = others[len(others) // 2]
        key[runner[K]] = 1
    _set_keys(ctx, graph, key)
    for K in (5, 65, 4097):
        hub = fan.hub_of(K)
        if K <= 1024:
            # degree == L once the self link is dropped (with it: L + 1 entries): the list is the whole in-list, no select
            st, res = _run(ctx, graph, key, [hub], K, flags, what="self, L == degree")
            lst = _lists(res)[0]
            assert hub + 1 not in lst and len(lst) == K and int(res[3][0]) == K and lst[0] == runner[K] + 1
            assert st["selected"] == (1 if flags & NO_SHORTCUT else 0)
        for limit in (1, 2, 1024):
            st, res = _run(ctx, graph, key, [hub], limit, flags, what="self, L < degree")
            lst = _lists(res)[0]
            assert lst[0] == runner[K] + 1 and hub + 1 not in lst and int(res[3][0]) == K and res[2][0] == 1 and (limit == 1 or res[2][1] >= 2)
            assert st["selected"] == (1 if K > limit or flags & NO_SHORTCUT else 0)
        # the same with the self link kept: the hub is present and first, and the list of L is cut
        L = min(K, 1024)
        st, res = _run(ctx, graph, key, [hub], L, flags | KEEP_SELF, what="self kept")
        lst = _lists(res)[0]
        assert lst[:2] == [hub + 1, runner[K] + 1] and len(lst) == L and int(res[3][0]) == K + 1 and st["selected"] == 1
    # a hub whose only in-neighbour is itself, and one with one leaf besides itself
    _, res = _run(ctx, graph, key, [fan.hub_of(0), fan.hub_of(1)], 3, flags)
    assert _lists(res) == [[], [int(fan.leaves(1)[0]) + 1]] and res[3].tolist() == [0, 1]
    _, res = _run(ctx, graph, key, [fan.hub_of(0), fan.hub_of(1)], 3, flags | KEEP_SELF)
    assert _lists(res) == [[fan.hub_of(0) + 1], [fan.hub_of(1) + 1, int(fan.leaves(1)[0]) + 1]] and res[3].tolist() == [1, 2]


@pytest.mark.parametrize("chunk", [0, 4])
def test_self_links(loaded, chunk):
    _self_links(loaded, chunk, 0)


# (4) ties
@pytest.mark.parametrize("chunk", [0, 4])
def test_ties_on_the_fan(loaded, chunk):
    fan, ctx, graph, plan = loaded(chunk)
    # no keys at all: NodeID order
    nokey = np.full(fan.n, U64_MAX, dtype=np.uint64)
    st = ctx.links_set_keys()
    assert st["listed"] == 0
    for limit in (1, 3, 64, 1024):
        _, res = _run(ctx, graph, nokey, fan.hub, limit, what="no keys")
        for K, lst in zip(KS, _lists(res)):
            assert lst == (fan.leaves(K)[:limit] + 1).tolist()
        assert (res[2] == np.uint64(U64_MAX)).all()
    # equal keys on both sides of the cut, in different chunks of the 4097 hub
    chunks, _ = _hub_list(fan, plan, 4097)
    assert len(chunks) >= 4
    base = _hash64(3, fan.n) | np.uint64(1 << 40)
    for a, b, c in ((0, len(chunks) - 1, 2), (1, len(chunks) // 2, len(chunks) - 2)):
        tied = [chunks[a][-1], chunks[b][0], chunks[c][1 % len(chunks[c])]]
        assert len(set(tied)) == 3
        key = base.copy()
        key[tied] = 5
        first, second = chunks[3][0], chunks[3][1]  # (chunk 3 is none of a, b, c)
        assert 3 not in (a, b, c)
        key[first] = 1
        key[second] = 2
        _set_keys(ctx, graph, key)
        for limit in (3, 4, 5, 6):  # the cut before, inside and behind the three tied entries
            _, res = _run(ctx, graph, key, [fan.hub_of(4097)], limit, what="tie")
            want = [first, second] + sorted(tied)
            assert _lists(res)[0][:5] == [v + 1 for v in want[:limit]]


def _literal_check(ctx, graph, keys, queries, limit, flags=0, slots=0):
    """a small graph against the literal restatement; keys: [(node, key)], queries: [node]"""
    lists, degrees, unknown_keys, unknown = lref.literal(*graph, keys, queries, limit, bool(flags & KEEP_SELF))
    st = ctx.backlinks(ids_from_ints(queries), limit, flags=flags, slots_per_batch=slots)
    off, ids, got_keys, deg = ctx.links_copy()
    assert _lists((off, ids, got_keys, deg)) == [[u for u, _ in lst] for lst in lists]
    assert got_keys.tolist() == [k for lst in lists for _, k in lst] and deg.tolist() == degrees and st["unknown"] == unknown
    return lists, st


def test_ties_on_wide_ids(gpu_ctx_factory):
    """128-bit ids that differ only in the high word: a tie goes to the smaller NodeID"""
    rng = np.random.default_rng(23)
    nodes = [(hi << 64) | 5 for hi in range(1, 41)]
    edges = sorted({(nodes[int(a)], nodes[int(b)]) for a, b in rng.integers(0, 40, (300, 2))})
    with _load(gpu_ctx_factory, edges) as ctx:
        graph = ctx.graph()
        assert lref.id_ints(graph[0]) == nodes
        for limit in (1, 3, 1024):
            lists, _ = _literal_check(ctx, graph, [], nodes, limit)  # without any hb_links_set_keys call
            assert all([u for u, _ in lst] == sorted(u for u, _ in lst) for lst in lists) and max(len(lst) for lst in lists) == min(limit, 11)  # (the longest in-list has 11 entries)
        keys = [(v, i % 3) for i, v in enumerate(nodes)]
        st = ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
        assert st["listed"] == 40
        for limit in (1, 3, 1024):
            _literal_check(ctx, graph, keys, nodes, limit)


def test_u64_max_is_a_key(gpu_ctx_factory):
    edges = [(3, 9), (4, 9), (5, 9), (1, 2), (6, 7), (8, 7)]
    with _load(gpu_ctx_factory, edges) as ctx:
        graph = ctx.graph()
        keys = [(3, U64_MAX), (4, U64_MAX - 1), (6, U64_MAX), (77, 1), (4, 0), (4, U64_MAX - 1)]  # listed u64::MAX, an unknown id, duplicates
        st = ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
        assert st["listed"] == 3 and st["unknown_keys"] == 1
        lists, _ = _literal_check(ctx, graph, keys, [9, 7, 2], 3)
        assert lists == [[(4, U64_MAX - 1), (3, U64_MAX), (5, U64_MAX)], [(6, U64_MAX), (8, U64_MAX)], [(1, U64_MAX)]]
        lists, _ = _literal_check(ctx, graph, keys, [9, 7], 1)
        assert lists == [[(4, U64_MAX - 1)], [(6, U64_MAX)]]


# (5) radix digits
@pytest.mark.parametrize("flags", DIGIT_FLAGS)
@pytest.mark.parametrize("chunk", [0, 4])
def test_digit_flags_change_nothing_on_list_lengths(loaded, chunk, flags):
    _list_lengths(loaded, chunk, flags)


@pytest.mark.parametrize("flags", DIGIT_FLAGS)
@pytest.mark.parametrize("chunk", [0, 4])
def test_digit_flags_change_nothing_on_self_links(loaded, chunk, flags):
    _self_links(loaded, chunk, flags)


@pytest.mark.parametrize("which", ["last of its bin", "first of its bin"])
def test_threshold_at_the_edge_of_a_top_digit_bin(loaded, which):
    """the keys are a permutation of 0 .. n - 1, so ord == key; with HB_LINKS_SPREAD_ORDS the select runs on ord * floor(2^32 / n) and
    its first round bins by the top byte of that"""
    fan, ctx, graph, plan = loaded(4)
    n, L, K = fan.n, 64, 4097
    mult = (1 << 32) // n
    assert (n - 1) * mult >= 1 << 24  # all four digits are used
    top = lambda o: (o * mult) >> 24  # noqa: E731
    bin_no = 3
    first_of_next = -(-((bin_no + 1) << 24) // mult)
    T = first_of_next - 1 if which == "last of its bin" else -(-(bin_no << 24) // mult)
    assert top(T) == bin_no and (top(T + 1) == bin_no + 1 if which == "last of its bin" else top(T - 1) == bin_no - 1)
    assert top(T - 2) == bin_no or which != "last of its bin"
    assert top(T + 2) == bin_no or which != "first of its bin"
    rng = np.random.default_rng(7)
    leaves = fan.leaves(K).copy()
    rng.shuffle(leaves)
    near_below, near_above = [T - 1, T - 2], [T + 1, T + 2]  # neighbours of the threshold on both sides
    below = np.concatenate((near_below, rng.choice(T - 2, L - 3, replace=False)))
    above = np.concatenate((near_above, T + 3 + rng.choice(n - T - 3, K - L - 2, replace=False)))
    leaf_ord = np.concatenate((below, [T], above)).astype(np.int64)
    assert len(leaf_ord) == K and len(set(leaf_ord.tolist())) == K and int((leaf_ord < T).sum()) == L - 1
    rest_nodes = np.setdiff1d(np.arange(n), leaves)
    rest_ord = np.setdiff1d(np.arange(n), leaf_ord)
    key = np.zeros(n, dtype=np.uint64)
    key[leaves] = leaf_ord.astype(np.uint64)
    key[rest_nodes] = rng.permutation(rest_ord).astype(np.uint64)
    assert np.array_equal(np.sort(key), np.arange(n, dtype=np.uint64))  # a permutation: ord == key
    _set_keys(ctx, graph, key)
    for flags in (SPREAD, SPREAD | NO_SHORTCUT, 0):
        for limit in (L - 1, L, L + 1):
            _, res = _run(ctx, graph, key, [fan.hub_of(K), fan.r], limit, flags, what=which)
            assert int(res[2][min(limit, L) - 1]) == (T if limit >= L else int(np.sort(leaf_ord)[limit - 1]))
        _, res = _run(ctx, graph, key, [fan.hub_of(K)], L, flags, what=which)
        assert int(res[2][-1]) == T and len(res[2]) == L  # the threshold entry is the last one kept


# (6) batches
def test_batches(loaded):
    fan, ctx, graph, plan = loaded(4)
    key = _hash64(9, fan.n) % np.uint64(50)  # ties all over
    _set_keys(ctx, graph, key)
    rng = np.random.default_rng(5)
    last = int(fan.leaf_first[0] + np.flatnonzero(fan.tips_of_leaf > 0)[-1])  # the last leaf that has an in-neighbour (its tips)
    qsids = np.concatenate((fan.hub, rng.integers(0, last, 260), fan.hub[::3], [-1] * 17))
    rng.shuffle(qsids)
    qsids = np.concatenate((qsids[:299], [last]))  # the last query is the highest sid: the last slot of the last batch
    assert len(qsids) == 300 and (qsids < 0).any() and len(np.unique(qsids)) < 290
    query_ids = np.zeros(300, dtype=_lib.U128)
    query_ids["lo"] = np.where(qsids >= 0, qsids + 1, fan.n + 1000 + np.arange(300)).astype(np.uint64)
    distinct = len(np.unique(qsids[qsids >= 0]))
    results = []
    for slots in (0, 1, 7, 64):
        st, res = _run(ctx, graph, key, qsids, 5, slots=slots, query_ids=query_ids, what="slots %d" % slots)
        assert st["batches"] == (1 if slots == 0 else -(-distinct // slots))
        results.append(tuple(a.tobytes() for a in res))
        last = int(qsids[-1])
        frm = graph[2][int(graph[1][last]):int(graph[1][last + 1])].astype(np.int64)
        frm = frm[np.lexsort((frm, key[frm]))][:5]
        assert _lists(res)[-1] == (frm + 1).tolist() and len(frm) > 0
    assert all(r == results[0] for r in results)
    st = ctx.backlinks(np.zeros(0, dtype=_lib.U128), 5)
    off, ids, keys, deg = ctx.links_copy()
    assert st["queries"] == 0 and st["batches"] == 0 and off.tolist() == [0] and len(ids) == len(keys) == len(deg) == 0 and ctx.links_count() == (0, 0)


# (7) keys from ranks
def test_keys_from_ranks(gpu_ctx_factory):
    with _load(gpu_ctx_factory, graphs.lcg_graph()) as ctx:
        graph = ctx.graph()
        nodes = lref.id_ints(graph[0])
        with pytest.raises(_lib.HyperballError) as e:
            ctx.links_set_keys(from_ranks=True)  # no live image
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_links_set_keys" in str(e.value)
        for make in (ctx.run, lambda: ctx.sampled_harmonic(max_dist=2, sources=graph[0][[5, 17, 100]])):
            make()
            ids, _ = ctx.results()
            ranks = ctx.ranks()
            assert 0 < len(ids) <= len(nodes)
            st = ctx.links_set_keys(from_ranks=True)
            assert st["listed"] == len(ids)
            for limit in (1, 3, 1024):
                ctx.backlinks(graph[0], limit)
                got = tuple(a.tobytes() for a in ctx.links_copy())
                _literal_check(ctx, graph, list(zip(lref.id_ints(ids), ranks.tolist())), nodes, limit)
            st = ctx.links_set_keys(ids, ranks)
            assert st["listed"] == len(ids)
            ctx.backlinks(graph[0], 1024)
            assert tuple(a.tobytes() for a in ctx.links_copy()) == got
            r2 = ctx.results()  # the image is only read
            assert r2[0].tobytes() == ids.tobytes()


# (8) against its L = 1 sibling
def _against_nearest_seed(ctx, graph, key):
    listed = np.flatnonzero(key != np.uint64(U64_MAX))
    ctx.nearest_seed(None, None, graph[0][listed], key[listed], discount_factor=0.5)
    seed, has = ctx.nearest_seed_seeds()
    ctx.links_set_keys(graph[0][listed], key[listed])
    ctx.backlinks(graph[0], 1)
    off, ids, _, deg = ctx.links_copy()
    assert np.array_equal(np.diff(off.astype(np.int64)) == 1, has) and np.array_equal(deg > 0, has)
    assert ids.tobytes() == np.ascontiguousarray(seed[has]).tobytes() and has.any() and not has.all()


def test_against_nearest_seed(loaded, gpu_ctx_factory):
    fan, ctx, graph, plan = loaded(4, self_links=True)  # (the tips have no in-neighbour, h_0 only itself)
    key = _hash64(2, fan.n) % np.uint64(9)
    key[::5] = U64_MAX
    _against_nearest_seed(ctx, graph, key)
    with _load(gpu_ctx_factory, graphs.lcg_graph() + [(1000, 1), (7, 7)]) as small:  # (1000 has no in-neighbour, 7 a self link)
        sgraph = small.graph()
        key = _hash64(4, len(sgraph[0])) % np.uint64(7)
        key[:5] = U64_MAX
        _against_nearest_seed(small, sgraph, key)


# (9) refusals: each leaves the previous result as it was
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
    ctx._check(ctx.lib.hb_backlinks(ctx.h, ctypes.byref(o), ctypes.byref(st)))


def _raw_keys(ctx, **fields):
    o = _lib.HbLinksKeyOptions()
    o.struct_size = ctypes.sizeof(_lib.HbLinksKeyOptions)
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        setattr(o, k, v)
    ctx._check(ctx.lib.hb_links_set_keys(ctx.h, ctypes.byref(o), None))


_ONE_ID, _ONE_KEY = ids_from_ints([1]), np.array([3], dtype=np.uint64)
REFUSALS = {
    "limit 0": lambda ctx: ctx.backlinks(_ONE_ID, 0),
    "limit 1025": lambda ctx: ctx.backlinks(_ONE_ID, 1025),
    "slots above 65536": lambda ctx: ctx.backlinks(_ONE_ID, 3, slots_per_batch=65537),
    "nodes NULL": lambda ctx: _raw(ctx, node_count=1),
    "opt NULL": lambda ctx: ctx._check(ctx.lib.hb_backlinks(ctx.h, None, None)),
    "open run": lambda ctx: ctx.backlinks(_ONE_ID, 3),
    "keys: open run": lambda ctx: ctx.links_set_keys(_ONE_ID, _ONE_KEY),
    "keys: from ranks without a live image": lambda ctx: ctx.links_set_keys(from_ranks=True),
    "keys: from ranks and a list": lambda ctx: _raw_keys(ctx, flags=_lib.HB_LINKS_KEYS_FROM_RANKS, key_ids=_ONE_ID, keys=_ONE_KEY, key_count=1),
    "keys: key ids NULL": lambda ctx: _raw_keys(ctx, keys=_ONE_KEY, key_count=1),
    "keys: keys NULL": lambda ctx: _raw_keys(ctx, key_ids=_ONE_ID, key_count=1),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusal_keeps_the_previous_result(gpu_ctx_factory, which):
    with _load(gpu_ctx_factory, graphs.lcg_graph(n=40, m=160, seed=9)) as ctx:
        graph = ctx.graph()
        nodes = lref.id_ints(graph[0])
        keys = [(v, v % 3) for v in nodes]
        ctx.links_set_keys(ids_from_ints(nodes), np.array([k for _, k in keys], dtype=np.uint64))
        _literal_check(ctx, graph, keys, nodes[::2] + [999], 3)
        before = tuple(a.tobytes() for a in ctx.links_copy()) + ctx.links_count()
        if which == "keys: from ranks and a list":
            ctx.run()  # (with a live image: the refusal is about the list)
        if "open run" in which:
            ctx.begin()
        with pytest.raises(_lib.HyperballError) as e:
            REFUSALS[which](ctx)
        assert e.value.code == _lib.HB_ERR_INVALID and ("hb_links_set_keys" if which.startswith("keys") else "hb_backlinks") in str(e.value), which
        if "open run" in which:
            ctx.finish()
        assert tuple(a.tobytes() for a in ctx.links_copy()) + ctx.links_count() == before, which
        _literal_check(ctx, graph, keys, nodes[::2] + [999], 3)  # the keys are the ones set before the refusal, too
        assert tuple(a.tobytes() for a in ctx.links_copy()) + ctx.links_count() == before, which


def test_refusals_of_the_entry(gpu_ctx_factory):
    def refused(fn, who):
        with pytest.raises(_lib.HyperballError) as e:
            fn()
        assert e.value.code == _lib.HB_ERR_INVALID and who in str(e.value)

    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        refused(lambda: ctx.backlinks(_ONE_ID, 3), "hb_backlinks")  # no graph loaded
        refused(lambda: ctx.links_set_keys(_ONE_ID, _ONE_KEY), "hb_links_set_keys")
        refused(ctx.links_count, "hb_links_count")
        ctx.load_edges(np.zeros(0, dtype=_lib.EDGE))  # an empty graph: every query is unknown
        assert ctx.links_set_keys(_ONE_ID, _ONE_KEY)["unknown_keys"] == 1
        st = ctx.backlinks(ids_from_ints([1, 2]), 3)
        assert st["unknown"] == 2 and st["entries"] == 0 and ctx.links_copy()[0].tolist() == [0, 0, 0]
    with _load(gpu_ctx_factory, graphs.lcg_graph(n=40, m=160, seed=9)) as ctx:
        refused(ctx.links_count, "hb_links_count")  # no result yet
        refused(ctx.links_copy, "hb_links_count")
        ctx.backlinks(ids_from_ints([1, 2]), 3)
        e = ctx.links_count()[1]
        off, deg = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        ctx._check(ctx.lib.hb_links_copy(ctx.h, _lib._ptr(off), _lib._ptr(deg), None, None, 0))  # offsets and degrees alone need no room
        assert int(off[-1]) == e > 0 and (deg >= np.diff(off)).all()
        small = np.zeros(e, dtype=_lib.U128)
        refused(lambda: ctx._check(ctx.lib.hb_links_copy(ctx.h, None, None, _lib._ptr(small), None, e - 1)), "hb_links_copy")
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        refused(lambda: ctx.backlinks(_ONE_ID, 3), "hb_backlinks")
        refused(lambda: ctx.links_set_keys(_ONE_ID, _ONE_KEY), "hb_links_set_keys")


# (10) the neighbours: nothing of theirs moves, and the result outlives each of them
def test_neighbours_and_reload(gpu_ctx_factory):
    g = synth.RmatGraph(11, 14_000)
    graph = (g.ids, g.row_ptr, g.src)
    nodes = lref.id_ints(g.ids)
    key = _hash64(6, g.n) % np.uint64(1000)
    liked = g.ids[[7, 11, 500]]
    indeg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
    qsids = np.concatenate((np.argsort(-indeg, kind="stable")[:40], np.arange(0, g.n, 37)))
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
        before = ctx.stats()["device_bytes"]
        kst = _set_keys(ctx, graph, key)
        st, res = _run(ctx, graph, key, qsids, 16, what="first call")
        assert st["selected"] > 0 and kst["device_bytes"] > 0
        assert ctx.stats()["device_bytes"] == before + st["device_bytes"]
        mine = tuple(a.tobytes() for a in res)

        def still_mine():
            assert tuple(a.tobytes() for a in ctx.links_copy()) == mine

        # what the others left is untouched by the call ...
        assert ctx.state_hash() == h0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.distance_copy(), d0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.betweenness_copy(), b0))
        assert ctx.similarity_all().tobytes() == s0.tobytes()
        assert (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes()) == n0
        # ... and each of them computes what it computed before, and leaves the backlinks result readable
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
        # hb_step between two calls
        ctx.begin()
        ctx.step()
        ctx.finish()
        st2, res2 = _run(ctx, graph, key, qsids, 16, what="second call")
        assert tuple(a.tobytes() for a in res2) == mine and st2["device_bytes"] == st["device_bytes"]
        ctx.begin()
        ctx.step()
        ctx.finish()
        ctx.run()
        assert ctx.state_hash() == h0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        # a second load: neither the keys nor the result of the first graph answer for the new one
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


# (11) the Python mirror
def test_python_mirror(gpu_ctx_factory):
    from stract_amd import backlinks
    tuples = graphs.lcg_graph() + [(7, 7)]
    with _load(gpu_ctx_factory, tuples) as ctx:
        graph = ctx.graph()
        nodes = lref.id_ints(graph[0])
        keys = [(v, (v * 7) % 5) for v in nodes[3:]]
        st = backlinks.set_link_keys(ctx, [v for v, _ in keys], [k for _, k in keys])
        assert st["listed"] == len(keys)
        queries = nodes[::3] + [7, 12345, 7]
        for keep_self in (False, True):
            lists, degrees, _, _ = lref.literal(*graph, keys, queries, 4, keep_self)
            off, ids, got_keys, deg = backlinks.host_backlinks(ctx, queries, 4, keep_self=keep_self)
            assert _lists((off, ids, got_keys, deg)) == [[u for u, _ in lst] for lst in lists]
            assert got_keys.tolist() == [k for lst in lists for _, k in lst] and deg.tolist() == degrees
        ctx.run()
        assert backlinks.set_link_keys_from_ranks(ctx)["listed"] == len(ctx.results()[0])
        off, ids, got_keys, deg = backlinks.host_backlinks(ctx, graph[0][:10], 2)
        ranks = dict(zip(lref.id_ints(ctx.results()[0]), ctx.ranks().tolist()))
        assert got_keys.tolist() == [ranks.get(u, U64_MAX) for u in lref.id_ints(ids)]


# (12) C2 size against the numpy form of the restatement (GPU only)
def test_c2_against_numpy(gpu_ctx_factory):
    g = synth.make_config("C2")[0]
    graph = (g.ids, g.row_ptr, g.src)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        assert ctx.stats()["virtual_rows"] > 0
        ctx.run()
        rids, _ = ctx.results()
        key = np.full(g.n, U64_MAX, dtype=np.uint64)
        key[_sids(graph, rids)] = ctx.ranks()
        st = ctx.links_set_keys(from_ranks=True)
        assert st["listed"] == len(rids) and 0 < len(rids) < g.n
        indeg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
        rng = np.random.default_rng(12)
        qsids = np.concatenate((np.argsort(-indeg, kind="stable")[:256], rng.choice(g.n, 256, replace=False)))
        st, res = _run(ctx, graph, key, qsids, 512, what="C2")
        assert st["selected"] >= 200 and int(indeg[qsids[:256]].min()) > 512  # (conditions on the INPUT: the hubs have more than they may keep)
        assert st["rows_walked"] > len(np.unique(qsids))  # chunk rows were walked
