"""hb_nearest_seed (HarmonicNearestSeed, crates/core/src/entrypoint/centrality.rs:126-201) against the host restatement in
tests/nearest_seed_ref.py.

Comparison rule: EVERYTHING is exact.  Seeds are compared as node ids; values as f64 bit patterns - a value is an original or an original
times discount_factor r times, computed the same way by the restatement; every counter of the stats as an integer.

The list-length, position, self-link and tie tests run on the flipped fan of tests/fans.py, whose in-lists carry the lengths: the hub
h_K has its K leaves as in-neighbours, under the default chunk and under chunk = 4 (a six-level tree at 4097).  Positions inside a
hub's list are taken from the plan, not from the leaf numbers: the planner permutes rows."""
import ctypes

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import EdgeListGraph, ids_from_ints
from tests import distance_ref as dref
from tests import fans
from tests import graphs
from tests import inbound_similarity_ref as sref
from tests import nearest_seed_ref as nref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
KS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
SELF_KS = (0, 1, 5, 65, 4097)  # hubs that get a self link (0: then its only in-neighbour is itself)
SALTS = tuple(range(8))
_FAN = []


def _fan():
    if not _FAN:
        _FAN.append(fans.Fan(Ks=KS))
    return _FAN[0]


def _hash64(salt, nodes):
    """splitmix64 of (salt, node): the minimum of a list lands at an arbitrary position"""
    m = (1 << 64) - 1
    out = []
    for v in nodes:
        z = (int(v) * 0x9E3779B97F4A7C15 + (int(salt) + 1) * 0xD1B54A32D192ED03) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        out.append(z ^ (z >> 31))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _call(ctx, orig=(), keys=(), discount=0.5, rounds=0, **kw):
    """orig: [(node int, value)], keys: [(node int, key)]"""
    orig, keys = list(orig), list(keys)
    return ctx.nearest_seed(ids_from_ints([v for v, _ in orig]), np.array([x for _, x in orig], dtype=np.float64),
                            ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64),
                            discount_factor=discount, rounds=rounds, **kw)


def _seeds(ctx, nodes):
    seed, has = ctx.nearest_seed_seeds()
    ints = sref.id_ints(seed)
    assert all(s == 0 for s, h in zip(ints, has.tolist()) if not h)
    return {v: s for v, s, h in zip(nodes, ints, has.tolist()) if h}


def _check(ctx, graph, orig=(), keys=(), discount=0.5, rounds=0, what=""):
    """one call against the literal restatement: the seed of every node, count / copy / all, every counter of the stats"""
    nodes = sref.id_ints(graph[0])
    want_seeds, want_vals, want_stats = nref.literal(*graph, list(orig), list(keys), discount, rounds)
    st = _call(ctx, orig, keys, discount, rounds)
    got_seeds = _seeds(ctx, nodes)
    bad = [v for v in nodes if got_seeds.get(v) != want_seeds.get(v)]
    assert not bad, (what, [(v, got_seeds.get(v), want_seeds.get(v)) for v in bad[:5]])
    want_all = np.array([want_vals.get(v, -1.0) for v in nodes], dtype=np.float64)
    got_all = ctx.nearest_seed_all()
    diff = np.flatnonzero(_bits(got_all) != _bits(want_all))
    assert not len(diff), (what, diff[:5], got_all[diff[:5]], want_all[diff[:5]])
    ids, vals = ctx.nearest_seed_copy()
    keep = [v for v in nodes if v in want_vals]
    assert ctx.nearest_seed_count() == len(keep) and sref.id_ints(ids) == keep, what
    assert np.array_equal(_bits(vals), _bits([want_vals[v] for v in keep])), what
    for k in nref.STAT_KEYS:
        assert st[k] == want_stats[k], (what, k, st[k], want_stats[k])
    assert st["device_bytes"] > 0 and st["results"] == st["with_original"] + sum(st["filled"])
    assert st["results"] + st["no_seed"] + st["seed_without_value"] == len(nodes)
    return want_seeds, want_vals, st


def _load(factory, tuples, chunk=0):
    ctx = factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk)
    ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
    return ctx


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


# (1) list lengths: every switch of the quad loop and of the chunk trees, the minimum at arbitrary positions
@pytest.mark.parametrize("chunk", [0, 4])
def test_list_lengths_on_the_flipped_fan(loaded, chunk):
    fan, ctx, graph, plan = loaded(chunk)
    assert np.array_equal(np.diff(graph[1].astype(np.int64))[fan.hub], np.array(fan.Ks))
    depth = {K: _hub_list(fan, plan, K)[1] for K in KS}
    if chunk == 0:
        assert all(depth[K] >= 1 for K in KS if K >= 65) and all(depth[K] == 0 for K in KS if K <= 64), depth
    else:
        assert depth[4097] == 6 and all(depth[K] >= 1 for K in KS if K >= 5) and depth[4] == 0, depth
    nodes = sref.id_ints(graph[0])
    for salt in SALTS:
        keys = list(zip(nodes, _hash64(salt, nodes)))
        want, _, _ = _check(ctx, graph, keys=keys, what="salt %d" % salt)
        for K in KS:  # (what the comparison above already says, spelled out for the hubs)
            if K:
                leaves = (fan.leaves(K) + 1).tolist()
                assert want[fan.hub_of(K) + 1] == min(leaves, key=lambda v: (keys[v - 1][1], v))


# (2) the position of the minimum in the hub's list
def _positions(chunks):
    flat_len = sum(len(ch) for ch in chunks)
    first = len(chunks[0])
    pos = [0, 3, 4, first - 1, first, flat_len - len(chunks[-1]), flat_len - 1]  # (a ragged last chunk of one entry: the last two agree)
    return [min(max(p, 0), flat_len - 1) for p in pos]


@pytest.mark.parametrize("chunk", [0, 4])
def test_position_of_the_minimum(loaded, chunk):
    fan, ctx, graph, plan = loaded(chunk)
    nodes = sref.id_ints(graph[0])
    base = [k | 1 for k in _hash64(11, nodes)]  # never 0
    lists = {K: [v for ch in _hub_list(fan, plan, K)[0] for v in ch] for K in (5, 65, 4097)}
    positions = {K: _positions(_hub_list(fan, plan, K)[0]) for K in lists}
    assert len(set(positions[4097])) >= (6 if chunk == 0 else 4)  # (chunk = 4: entries 3 and 4 ARE the end of the first chunk and the start of the second)
    for i in range(7):
        keys = list(base)
        picked = {}
        for K in lists:
            leaf = lists[K][positions[K][i]]
            keys[leaf] = 0
            picked[K] = leaf
        want, _, _ = _check(ctx, graph, keys=list(zip(nodes, keys)), what="position %d" % i)
        for K, leaf in picked.items():
            assert want[fan.hub_of(K) + 1] == leaf + 1


# (3) self links: the hub's own candidate is the minimum of its chunk and must not hide the runner-up
@pytest.mark.parametrize("chunk", [0, 4])
def test_self_link_with_the_smallest_key(loaded, chunk):
    fan, ctx, graph, plan = loaded(chunk, self_links=True)
    nodes = sref.id_ints(graph[0])
    base = [(k | 1) + 1 for k in _hash64(5, nodes)]  # at least 2
    for K in SELF_KS:
        base[fan.hub_of(K)] = 0  # the smallest key of all
    seen_other_chunk = False
    for other_chunk in (False, True):
        keys = list(base)
        runner = {}
        for K in (5, 65, 4097):
            chunks, _ = _hub_list(fan, plan, K, self_link=True)
            mine = next(i for i, ch in enumerate(chunks) if fan.hub_of(K) in ch)
            same = [v for v in chunks[mine] if v != fan.hub_of(K)]
            others = [v for i, ch in enumerate(chunks) if i != mine for v in ch]
            pick = others[len(others) // 2] if (other_chunk and others) or not same else same[-1]
            seen_other_chunk |= other_chunk and bool(others)
            keys[pick] = 1
            runner[K] = pick
        want, _, _ = _check(ctx, graph, keys=list(zip(nodes, keys)), what="other chunk: %s" % other_chunk)
        assert fan.hub_of(0) + 1 not in want  # its only in-neighbour is itself: no seed
        assert want[fan.hub_of(1) + 1] == int(fan.leaves(1)[0]) + 1  # in the flipped fan h_1 has its one leaf besides itself
        for K, leaf in runner.items():
            assert want[fan.hub_of(K) + 1] == leaf + 1, K
    assert seen_other_chunk


# (4) ties and missing keys
@pytest.mark.parametrize("chunk", [0, 4])
def test_ties_and_missing_keys(loaded, chunk):
    fan, ctx, graph, plan = loaded(chunk)
    nodes = sref.id_ints(graph[0])
    want, _, st = _check(ctx, graph, what="no keys")  # every seed is the smallest in-neighbour id
    rp, src = graph[1].astype(np.int64), graph[2]
    for K in KS:
        if K:
            assert want[fan.hub_of(K) + 1] == int(fan.leaves(K).min()) + 1
    assert all(want[v + 1] == int(src[rp[v]:rp[v + 1]].min()) + 1 for v in range(fan.n) if rp[v + 1] > rp[v]) and st["unknown_keys"] == 0
    # two equal minimal keys in different chunks of the 4097 hub
    chunks, _ = _hub_list(fan, plan, 4097)
    assert len(chunks) >= 4
    base = [k | 1 for k in _hash64(3, nodes)]
    for a, b in ((0, len(chunks) - 1), (1, len(chunks) // 2), (len(chunks) - 2, 2)):
        keys = list(base)
        keys[chunks[a][-1]] = keys[chunks[b][0]] = 0
        want, _, _ = _check(ctx, graph, keys=list(zip(nodes, keys)), what="tie between chunks %d and %d" % (a, b))
        assert want[fan.hub_of(4097) + 1] == min(chunks[a][-1], chunks[b][0]) + 1


def test_ties_on_wide_ids(gpu_ctx_factory):
    """128-bit ids whose low words are ordered unlike the full ids: a tie goes to the smaller NodeID, not to the smaller low word"""
    rng = np.random.default_rng(23)
    nodes = [(hi << 64) | (1000 - 7 * hi) for hi in range(1, 41)]
    edges = sorted({(nodes[int(a)], nodes[int(b)]) for a, b in rng.integers(0, 40, (300, 2))})
    with _load(gpu_ctx_factory, edges) as ctx:
        graph = ctx.graph()
        assert sref.id_ints(graph[0]) == nodes
        want, _, _ = _check(ctx, graph, orig=[(v, 0.5) for v in nodes[::3]], what="wide, no keys")
        rp, src = graph[1].astype(np.int64), graph[2]
        low_first = sum(1 for v in range(40) if nodes[v] in want and want[nodes[v]] & ((1 << 64) - 1) != min(nodes[int(u)] & ((1 << 64) - 1) for u in src[rp[v]:rp[v + 1]] if u != v))
        assert low_first > 10  # the low words would have chosen otherwise
        _check(ctx, graph, orig=[(v, 0.5) for v in nodes[::3]], keys=[(v, i % 3) for i, v in enumerate(nodes)], rounds=2, what="wide, three keys")


# (5) u64::MAX is an ordinary key
def test_u64_max_is_a_key(gpu_ctx_factory):
    edges = [(3, 9), (4, 9), (5, 9), (1, 2), (6, 7), (8, 7)]
    with _load(gpu_ctx_factory, edges) as ctx:
        graph = ctx.graph()
        orig = [(3, 0.5), (4, 0.25), (8, 0.125)]
        want, vals, _ = _check(ctx, graph, orig=orig, keys=[(1, 5), (2, 1)], what="unlisted in-neighbours")
        assert want[9] == 3 and vals[9] == 0.25 and want[7] == 6 and 7 not in vals
        want, vals, _ = _check(ctx, graph, orig=orig, keys=[(3, nref.U64_MAX), (4, nref.U64_MAX - 1), (6, nref.U64_MAX)], what="listed u64::MAX")
        assert want[9] == 4 and vals[9] == 0.125 and want[7] == 6


# (6) the value rules
def _lcg_lists(nodes):
    orig = [(v, (i % 5) / 8.0) for i, v in enumerate(nodes[::3])]  # ties in the value, and 0.0
    orig += [(nodes[0], 0.875), (nodes[3], 0.0), (1 << 70, 0.5), (777777, 0.25), (nodes[0], 0.625)]  # duplicates (the last wins), unknown ids
    keys = [(v, k % 7) for v, k in zip(nodes, _hash64(2, nodes))] + [((1 << 70) + 1, 0)]
    return orig, keys[5:]  # the first five nodes are not listed


@pytest.mark.parametrize("rounds", [1, 2, 255])
def test_value_rules_on_the_lcg_graph(gpu_ctx_factory, rounds):
    with _load(gpu_ctx_factory, graphs.lcg_graph()) as ctx:
        graph = ctx.graph()
        nodes = sref.id_ints(graph[0])
        n = len(nodes)
        assert n == 200
        orig, keys = _lcg_lists(nodes)
        for discount in (0.5, 0.3, 0.0):
            _, vals, st = _check(ctx, graph, orig, keys, discount, rounds, what="rounds %d, discount %s" % (rounds, discount))
            assert st["unknown_orig"] == 2 and st["unknown_keys"] == 1 and st["with_original"] == len(nodes[::3]) and st["filled"][0] > 0
            assert st["rounds_run"] == (1 if rounds == 1 else 2 if rounds == 2 else st["rounds_run"]) and st["rounds_run"] <= rounds
            assert len(set(vals.values())) < len(vals)  # ties in the value
            for k in (0, 1, 7, n + 5):
                ids, got = ctx.nearest_seed_top(k)
                order = nref.top_order(vals, k)
                assert sref.id_ints(ids) == [v for v, _ in order], (k, discount)
                assert np.array_equal(_bits(got), _bits([x for _, x in order])), (k, discount)
            assert len(ctx.nearest_seed_top(n + 5)[0]) == st["results"]
        if rounds == 255:
            assert 2 < st["rounds_run"] < 255 and st["filled"][st["rounds_run"] - 1] == 0  # stopped by the round that filled nothing


def test_python_mirror(gpu_ctx_factory, tmp_path):
    from stract_amd.nearest_seed import NearestSeed, harmonic_nearest_seed
    from tests import speedy_kv_reader as kv
    tuples = graphs.lcg_graph()
    g = EdgeListGraph.from_tuples(tuples)
    graph = graphs.dense_from_tuples(tuples)
    nodes = sref.id_ints(graph[0])
    original = {v: (i % 5) / 8.0 for i, v in enumerate(nodes[::3])}
    ranks = {v: k % 7 for v, k in zip(nodes, _hash64(2, nodes))}
    want_seeds, want_vals, _ = nref.literal(*graph, list(original.items()), list(ranks.items()), 0.5, 1)
    ids, vals, st = harmonic_nearest_seed(g, original, ranks, output=tmp_path / "out")
    assert dict(zip(sref.id_ints(ids), _bits(vals).tolist())) == {k: int(np.float64(v).view(np.uint64)) for k, v in want_vals.items()}
    stored = kv.Db(str(tmp_path / "out" / "harmonic"), "f64", str(tmp_path))
    assert dict(stored.items()) == want_vals and len(want_vals) == st["results"]
    with _load(gpu_ctx_factory, tuples) as ctx:
        res = NearestSeed.run(ctx, original, ranks)
        assert res.seeds() == want_seeds and res.top(3)[0] == [v for v, _ in nref.top_order(want_vals, 3)]


# (7) refusals: each leaves the previous result as it was
def _raw(ctx, **fields):
    o = _lib.HbNearestSeedOptions()
    o.struct_size = ctypes.sizeof(_lib.HbNearestSeedOptions)
    o.discount_factor = 0.5
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        setattr(o, k, v)
    st = _lib.HbNearestSeedStats()
    st.struct_size = ctypes.sizeof(_lib.HbNearestSeedStats)
    ctx._check(ctx.lib.hb_nearest_seed(ctx.h, ctypes.byref(o), ctypes.byref(st)))


_ONE_ID, _ONE_VAL, _ONE_KEY = ids_from_ints([1]), np.array([0.5]), np.array([3], dtype=np.uint64)
REFUSALS = {
    "discount NaN": lambda ctx: _call(ctx, [(1, 0.5)], discount=float("nan")),
    "discount infinite": lambda ctx: _call(ctx, [(1, 0.5)], discount=float("inf")),
    "discount negative": lambda ctx: _call(ctx, [(1, 0.5)], discount=-0.5),
    "discount -0.0": lambda ctx: _call(ctx, [(1, 0.5)], discount=-0.0),
    "rounds > 255": lambda ctx: _call(ctx, [(1, 0.5)], rounds=256),
    "image and orig list": lambda ctx: _call(ctx, [(1, 0.5)], from_image=True),
    "image and orig pointer": lambda ctx: _raw(ctx, flags=_lib.HB_SEED_FROM_IMAGE, orig_ids=_ONE_ID),
    "no live image": lambda ctx: _call(ctx, from_image=True),
    "orig ids NULL": lambda ctx: _raw(ctx, orig_vals=_ONE_VAL, orig_count=1),
    "orig vals NULL": lambda ctx: _raw(ctx, orig_ids=_ONE_ID, orig_count=1),
    "key ids NULL": lambda ctx: _raw(ctx, keys=_ONE_KEY, key_count=1),
    "keys NULL": lambda ctx: _raw(ctx, key_ids=_ONE_ID, key_count=1),
    "orig NaN": lambda ctx: _call(ctx, [(1, 0.5), (2, float("nan"))]),
    "orig negative": lambda ctx: _call(ctx, [(1, 0.5), (2, -1.0)]),
    "orig -0.0": lambda ctx: _call(ctx, [(2, -0.0)]),
    "open run": None,
    "opt NULL": lambda ctx: ctx._check(ctx.lib.hb_nearest_seed(ctx.h, None, None)),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusal_keeps_the_previous_result(gpu_ctx_factory, which):
    with _load(gpu_ctx_factory, graphs.lcg_graph(n=40, m=160, seed=9)) as ctx:
        graph = ctx.graph()
        nodes = sref.id_ints(graph[0])
        _check(ctx, graph, [(v, 0.25) for v in nodes[::4]], [(v, v % 3) for v in nodes], 0.5, 2, what="before")
        before = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes(), ctx.nearest_seed_count())
        if which == "image and orig list" or which == "image and orig pointer":
            ctx.run()  # (with a live image: the refusal is about the list)
        if which == "open run":
            ctx.begin()
        with pytest.raises(_lib.HyperballError) as e:
            (REFUSALS[which] or (lambda c: _call(c, [(1, 0.5)])))(ctx)
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_nearest_seed" in str(e.value), which
        if which == "open run":
            ctx.finish()
        after = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes(), ctx.nearest_seed_count())
        assert after == before, which
        assert [len(x) for x in ctx.nearest_seed_copy()] == [before[2]] * 2 and len(ctx.nearest_seed_top(3)[0]) == 3


def test_refusals_of_the_entry(gpu_ctx_factory):
    def refused(fn, who="hb_nearest_seed"):
        with pytest.raises(_lib.HyperballError) as e:
            fn()
        assert e.value.code == _lib.HB_ERR_INVALID and who in str(e.value)

    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        refused(lambda: _call(ctx, [(1, 0.5)]))  # no graph loaded
        refused(ctx.nearest_seed_count, "hb_nearest_seed_count")
        ctx.load_edges(np.zeros(0, dtype=_lib.EDGE))  # an empty graph: an empty result
        st = _call(ctx, [(1, 0.5)], [(2, 1)])
        assert st["unknown_orig"] == 1 and st["unknown_keys"] == 1 and st["results"] == 0 and st["rounds_run"] == 0
        assert ctx.nearest_seed_count() == 0 and len(ctx.nearest_seed_top(4)[0]) == 0 and len(ctx.nearest_seed_all()) == 0
    with _load(gpu_ctx_factory, graphs.lcg_graph(n=40, m=160, seed=9)) as ctx:
        for fn, who in ((ctx.nearest_seed_all, "hb_nearest_seed_all"), (ctx.nearest_seed_copy, "hb_nearest_seed_count"),
                        (lambda: ctx.nearest_seed_top(2), "hb_nearest_seed_top"), (ctx.nearest_seed_seeds, "hb_nearest_seed_seeds")):
            refused(fn, who)  # no result yet
        _call(ctx)  # no orig, no keys: succeeds, nothing has a value
        assert ctx.nearest_seed_count() == 0 and (ctx.nearest_seed_all() == -1.0).all()
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        refused(lambda: _call(ctx, [(1, 0.5)]))


# (8) the original from the live image
def test_original_from_the_live_image(gpu_ctx_factory):
    g = synth.RmatGraph(10, 6_000)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        nodes = sref.id_ints(g.ids)
        keys = ids_from_ints(nodes), np.array(_hash64(4, nodes), dtype=np.uint64)
        for sampled, make in enumerate((ctx.run, lambda: ctx.sampled_harmonic(max_dist=1, sources=g.ids[[5]]))):
            make()
            ids, vals = ctx.results()
            assert 0 < len(ids) < g.n
            for rounds in (1, 3):
                st_list = ctx.nearest_seed(ids, vals, keys[0], keys[1], discount_factor=0.5, rounds=rounds)
                want = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes(), ctx.nearest_seed_copy()[0].tobytes())
                st_img = ctx.nearest_seed(None, None, keys[0], keys[1], discount_factor=0.5, rounds=rounds, from_image=True)
                got = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes(), ctx.nearest_seed_copy()[0].tobytes())
                assert got == want
                assert {k: st_img[k] for k in nref.STAT_KEYS} == {k: st_list[k] for k in nref.STAT_KEYS} and st_img["with_original"] == len(ids)
                assert st_img["filled"][0] > 0 or not sampled  # (after hb_run every node with an in-neighbour has a value of its own)
            r2 = ctx.results()  # the image is only read
            assert r2[0].tobytes() == ids.tobytes() and r2[1].tobytes() == vals.tobytes()


# (9) the neighbours: nothing of theirs moves, and the result outlives each of them
def test_neighbours_and_reload(gpu_ctx_factory):
    g = synth.RmatGraph(11, 14_000)
    graph = (g.ids, g.row_ptr, g.src)
    nodes = sref.id_ints(g.ids)
    orig = [(v, (i % 9) / 16.0) for i, v in enumerate(nodes[::5])]
    keys = list(zip(nodes, _hash64(6, nodes)))
    liked = sref.id_ints(g.ids[[7, 11, 500]])
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(*graph)
        ctx.run()
        h0, r0 = ctx.state_hash(), ctx.results()
        d0 = ctx.distances(g.ids[[11, 500]])[:2]
        b0 = ctx.betweenness(g.ids[[3, 11, 500]])[:2]
        ctx.inbound_similarity(ids_from_ints(liked))
        s0 = ctx.similarity_all()
        ctx.run()
        assert ctx.state_hash() == h0
        before = ctx.stats()["device_bytes"]
        _, _, st = _check(ctx, graph, orig, keys, 0.5, 3, what="first call")
        assert ctx.stats()["device_bytes"] == before + st["device_bytes"]
        mine = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes())

        def still_mine():
            assert (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes()) == mine

        # what the others left is untouched by the call ...
        assert ctx.state_hash() == h0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.distance_copy(), d0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.betweenness_copy(), b0))
        assert ctx.similarity_all().tobytes() == s0.tobytes()
        # ... and each of them computes what it computed before, and leaves the nearest-seed result readable
        ctx.run()
        assert ctx.state_hash() == h0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        still_mine()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.distances(g.ids[[11, 500]])[:2], d0))
        still_mine()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.betweenness(g.ids[[3, 11, 500]])[:2], b0))
        still_mine()
        ctx.inbound_similarity(ids_from_ints(liked))
        assert ctx.similarity_all().tobytes() == s0.tobytes()
        still_mine()
        st2 = _call(ctx, orig, keys, 0.5, 3)
        assert st2["device_bytes"] == st["device_bytes"] and ctx.stats()["device_bytes"] == before + st["device_bytes"]
        still_mine()
        # a second load: nothing of the first graph answers for the new one
        small = graphs.lcg_graph(n=70, m=300, seed=3)
        ctx.load_edges(EdgeListGraph.from_tuples(small).host_edges())
        with pytest.raises(_lib.HyperballError) as e:
            ctx.nearest_seed_all()
        assert e.value.code == _lib.HB_ERR_INVALID
        sgraph = ctx.graph()
        snodes = sref.id_ints(sgraph[0])
        _, _, st3 = _check(ctx, sgraph, [(v, 0.5) for v in snodes[::4]], [(v, v % 5) for v in snodes], 0.3, 2, what="after the reload")
        assert 0 < st3["device_bytes"] < st["device_bytes"]


# (10) C2 size against the numpy form of the restatement (GPU only)
def _numpy_check(ctx, g, tenth_seed, rounds):
    rng = np.random.default_rng(tenth_seed)
    orig_sids = np.sort(rng.choice(g.n, g.n // 10, replace=False))
    orig_vals = rng.random(len(orig_sids))
    lo = np.asarray(g.ids["lo"], dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = lo * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    key = z ^ (z >> np.uint64(31))
    seed, val, has, filled, rounds_run = nref.numpy_form(g.ids, g.row_ptr, g.src, orig_sids, orig_vals, key, 0.5, rounds)
    st = ctx.nearest_seed(g.ids[orig_sids], orig_vals, g.ids, key, discount_factor=0.5, rounds=rounds)
    got_seed, got_has = ctx.nearest_seed_seeds()
    assert np.array_equal(got_has, seed >= 0)
    assert got_seed[got_has].tobytes() == np.ascontiguousarray(g.ids[seed[seed >= 0]]).tobytes()
    assert np.array_equal(_bits(ctx.nearest_seed_all()), _bits(np.where(has, val, -1.0)))
    assert st["filled"] == filled and st["rounds_run"] == rounds_run and st["results"] == int(has.sum()) and st["with_original"] == len(orig_sids)
    return st, seed


def test_numpy_form_on_the_lcg_graph(gpu_ctx_factory):
    """the numpy form is the literal restatement (tests/test_nearest_seed_ref.py) - and the device agrees with both on the graph they share"""
    tuples = graphs.lcg_graph()
    ids, row_ptr, src = graphs.dense_from_tuples(tuples)

    class G:
        pass
    g = G()
    g.ids, g.row_ptr, g.src, g.n = ids, row_ptr, src, len(ids)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(ids, row_ptr, src)
        _numpy_check(ctx, g, 1, 3)


def test_c2_against_numpy(gpu_ctx_factory):
    g = synth.make_config("C2")[0]
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        assert ctx.stats()["virtual_rows"] > 0
        st, seed = _numpy_check(ctx, g, 5, 3)
        # (conditions on the INPUT: a tenth of the nodes has a value, so about a tenth of the others finds one at its seed in round 1)
        assert st["filled"][0] > g.n // 100 and st["filled"][1] > 0 and int((seed >= 0).sum()) > g.n // 2


def test_c2_original_from_a_compact_image(gpu_ctx_factory):
    """The result image is compact (one entry per node WITH in-edges, read through cid_of) only on a graph of 2^20 nodes or more in the
    product library - the switch that forces it at small sizes belongs to the experiments build.  Half of the nodes here have no in-edge."""
    n = (1 << 20) + 64
    v = np.arange(0, n, 2, dtype=np.int64)
    src = np.stack([(v * 7 + 1) % n, (v * 13 + 6) % n], axis=1)
    src = np.where(src == v[:, None], (src + 2) % n, src)
    src = np.sort(src, axis=1)
    assert (src[:, 0] != src[:, 1]).all()
    row_ptr = np.zeros(n + 1, dtype=np.uint64)
    row_ptr[1:] = np.cumsum(np.where(np.arange(n) % 2 == 0, 2, 0))
    ids = np.zeros(n, dtype=_lib.U128)
    ids["lo"] = np.arange(1, n + 1, dtype=np.uint64)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(ids, row_ptr, src.reshape(-1).astype(np.uint32))
        assert ctx.stats()["rows_with_in_edges"] == n // 2
        key = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 20)
        # the sampled image (written whole), then hb_run's (shipped in stages while the passes run, the rest as a list)
        for sampled, make in ((True, lambda: ctx.sampled_harmonic(max_dist=3, sources=ids[[0, 2, 11, 4096, n - 2]])), (False, ctx.run)):
            make()
            rids, rvals = ctx.results()
            assert 0 < len(rids) <= n // 2 and (len(rids) < n // 2 or not sampled)
            ctx.nearest_seed(rids, rvals, ids, key, discount_factor=0.5, rounds=2)
            want = (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes())
            st = ctx.nearest_seed(None, None, ids, key, discount_factor=0.5, rounds=2, from_image=True)
            assert (ctx.nearest_seed_all().tobytes(), ctx.nearest_seed_seeds()[0].tobytes()) == want
            assert st["with_original"] == len(rids) and (st["filled"][0] > 0 or not sampled)
