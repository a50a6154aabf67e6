"""hb_similar_hosts (scored_nodes of SimilarHostsFinder::find_similar_hosts, crates/core/src/similar_hosts.rs:54-272) against the literal
restatement in tests/similar_hosts_ref.py.

Comparison rule: EVERYTHING is exact - candidates and counts as integers, list entries as node ids in list order, every score by its
f64 bit pattern, the stats counters as integers.

The graphs come from similar_hosts_ref.layered(): liked hosts, a layer of sources, a layer of targets, a few thousand nodes.  One
graph (`small`) sits on the switch of the popularity filter (nb = 32 / 33), the caps, the count bound and the 513-entry out-list; the
other (`long`) on the 128 / 512 cuts of the in-lists."""
import ctypes

import numpy as np
import pytest

from stract_amd import _lib
from stract_amd.harmonic import ids_from_ints
from tests import links_ref as lref
from tests import similar_hosts_ref as sref

pytestmark = pytest.mark.gpu

U64_MAX = lref.U64_MAX
SPREAD, NO_SHORTCUT = _lib.HB_LINKS_SPREAD_ORDS, _lib.HB_LINKS_NO_SHORTCUT
A1, A2, LONELY = 1, 2, 3
SRC0, SINGLE0, T9, T10, TALL, X, M12, M8, WIDE0 = 100, 1000, 5000, 5001, 5002, 5003, 6000, 6100, 20000
A3, A4, S3, S4, HUB, FILL0 = 10, 11, 30000, 31000, 40000, 50000


def _mix(v, salt):
    z = (v * 0x9E3779B97F4A7C15 + (salt + 1) * 0xD1B54A32D192ED03) & U64_MAX
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64_MAX
    return z ^ (z >> 31)


def small_graph(S):
    """S sources, all linking to the liked host A1 and the first five to A2 as well: nb = S."""
    src = list(range(SRC0, SRC0 + S))
    liked_in = {A1: src, A2: src[:5]}
    out = {b: list(range(SINGLE0 + 40 * i, SINGLE0 + 40 * i + 40)) for i, b in enumerate(src)}  # 40 targets of its own each: more than 1024 in all
    for i, b in enumerate(src):
        out[b] += [TALL] + ([T9] if i < 9 else []) + ([T10] if i < 10 else []) + ([X] if i < 9 else [])
        out[b] += [M12 + j for j in range(16) if j <= i < j + 12] + [M8 + j for j in range(16) if j <= i < j + 8]  # identical shapes: score ties
    out[src[0]] += list(range(WIDE0, WIDE0 + 480))  # the first source has far more than 512 out-links
    extra = [(LONELY, SRC0)] + [(7000 + j, T9) for j in range(60)]  # LONELY has no in-link; T9 has sixty in-links of its own besides
    return sref.layered(liked_in, out, extra)


def small_keys(graph, salt=0):
    nodes = lref.id_ints(graph[0])
    keys = {v: _mix(v, salt) >> 1 for v in nodes}
    keys[X] = U64_MAX - 1  # the worst key of all: the 513th and later of the first source's out-links
    return sorted(keys.items())


def long_graph():
    """A3 has 513 in-links, A4 129: only the best 128 of each feed B, only the best 512 the BitVec; HUB has more than 512 in-links"""
    s3, s4 = list(range(S3, S3 + 513)), list(range(S4, S4 + 129))
    out = {b: [HUB + i % 50, HUB + 1000 + i % 7] for i, b in enumerate(s3)}
    out.update({b: [HUB + i % 50, HUB + 2000 + i % 3] for i, b in enumerate(s4)})
    extra = [(FILL0 + j, HUB) for j in range(520)] + [(FILL0 + j, HUB + 1) for j in range(300)]
    return sref.layered({A3: s3, A4: s4}, out, extra)


def _load(factory, graph, chunk=0):
    ctx = factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk)
    ctx.load_dense(*graph)
    return ctx


def _set(ctx, keys):
    if keys:
        ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
    else:
        ctx.links_set_keys()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def _check(ctx, graph, keys, liked, k, flags=0):
    want = sref.literal(*graph, keys, liked, k)
    st = ctx.similar_hosts(ids_from_ints(liked), k, flags=flags)
    cids, ccounts = ctx.similar_candidates()
    assert list(zip(lref.id_ints(cids), ccounts.tolist())) == want["candidates"]
    ids, scores = ctx.similar_copy()
    assert lref.id_ints(ids) == [v for v, _ in want["top"]]
    assert _bits(scores) == _bits([s for _, s in want["top"]])
    assert (st["nb"], bool(st["apply"]), st["count_bound"], st["taken"]) == (want["nb"], want["apply"], want["bound"], want["taken"])
    assert st["candidates"] == len(want["candidates"]) and st["written"] == len(want["top"]) == min(k, len(want["candidates"]))
    known = set(lref.id_ints(graph[0]))
    assert st["unknown"] == sum(1 for a in liked if a not in known) and st["liked_distinct"] == len({a for a in liked if a in known})
    assert (st["forward_entries"], st["distinct_targets"]) == (want["forward_entries"], want["distinct_targets"])
    assert (st["pairs_gated"], st["pairs_intersected"]) == (want["gated"], want["intersected"])
    assert st["device_bytes"] > 0 or not st["liked_distinct"]
    return st, want


@pytest.fixture(scope="module")
def small(gpu_ctx_factory):
    cache = {}

    def get(S, chunk=0):
        if (S, chunk) not in cache:
            graph = small_graph(S)
            cache[(S, chunk)] = (_load(gpu_ctx_factory, graph, chunk), graph)
        return cache[(S, chunk)]

    yield get
    for ctx, _ in cache.values():
        ctx.close()


@pytest.fixture(scope="module")
def long(gpu_ctx_factory):
    graph = long_graph()
    ctx = _load(gpu_ctx_factory, graph, 4)
    yield ctx, graph
    ctx.close()


# the switch of the filter and of the cap: nb = 32 keeps everything and takes 1024, nb = 33 drops count > 9 and takes 256
@pytest.mark.parametrize("S", [32, 33])
def test_filter_switch_caps_and_bound(small, S):
    ctx, graph = small(S)
    keys = small_keys(graph)
    _set(ctx, keys)
    st, want = _check(ctx, graph, keys, [A1, A2], 1024)
    cand = dict(want["candidates"])
    if S == 32:
        assert not want["apply"] and want["taken"] == 1024 and st["distinct_targets"] > 1024
        assert len(cand) == 1022 and A1 not in cand and A2 not in cand  # both liked hosts were inside the prefix: two short, not refilled
        assert cand[TALL] == 32 and cand[T10] == 10 and cand[M12] == 12
        singles = [v for v, c in want["candidates"] if c == 1]
        assert singles == sorted(singles) and singles[0] < SINGLE0 + 40 and max(singles) < SINGLE0 + 40 * 32  # the tie across the cap: NodeID ascending
    else:
        assert want["apply"] and want["bound"] == 9 and want["taken"] == 256  # (A1, linked by all 33, fell to the filter first)
        assert len(cand) == 255 and A2 not in cand  # A2 (count 5) was inside the taken prefix: one short, not refilled
        assert cand[T9] == 9 and T10 not in cand and TALL not in cand and M12 not in cand and cand[M8] == 8
        assert sum(1 for c in cand.values() if c == 1) > 0  # the count-1 tie crosses the cap here, too
    assert cand[X] == 8  # nine sources link to X, but it is the 513th or later of the first one's list by key
    # score ties: the M8 targets with the same shape share a score; the larger NodeID comes first
    top = want["top"]
    ties = [(a, b) for a, b in zip(top, top[1:]) if a[1] == b[1]]
    assert ties and all(a[0] > b[0] for a, b in ties)
    assert st["pairs_gated"] > 0 and st["pairs_intersected"] > 0


def test_k_below_at_and_above_the_candidates(small):
    ctx, graph = small(33)
    keys = small_keys(graph)
    _set(ctx, keys)
    for k in (1, 5, 255, 256, 257, 1024):
        st, want = _check(ctx, graph, keys, [A1, A2], k)
        assert st["written"] == min(k, 255)


def test_duplicate_unknown_and_lonely_liked_hosts(small):
    ctx, graph = small(32)
    keys = small_keys(graph, salt=3)
    _set(ctx, keys)
    _, one = _check(ctx, graph, keys, [A1], 50)
    _, dup = _check(ctx, graph, keys, [A1, A1, 999999, A2, A1], 50)  # N = 5: the duplicate counts three times, the unknown id in N only
    assert dup["candidates"][:5] != [] and [s for _, s in dup["top"]] != [s for _, s in one["top"]]
    _, order = _check(ctx, graph, keys, [A2, 999999, A1, A1, A1], 50)  # the same multiset in another order: summed in caller order
    assert order["candidates"] == dup["candidates"]
    st, want = _check(ctx, graph, keys, [LONELY], 10)  # no in-link: B and the result are empty, and the call is OK
    assert want["nb"] == 0 and want["top"] == [] and st["written"] == 0 and ctx.similar_copy()[0].size == 0
    st, want = _check(ctx, graph, keys, [A1, LONELY], 50)  # a liked host with an empty list beside one with candidates: its pairs are neither
    assert st["pairs_gated"] + st["pairs_intersected"] == len(want["candidates"]) > 0 and st["liked_distinct"] == 2
    st, want = _check(ctx, graph, keys, [424242, 424243], 10)  # nothing known
    assert st["liked_distinct"] == 0 and st["unknown"] == 2 and want["top"] == []
    st, want = _check(ctx, graph, keys, [SRC0, LONELY], 10)  # a liked host whose only in-link comes from another liked host
    assert want["nb"] == 1 and want["taken"] == 1 and want["candidates"] == []


def test_the_gated_pair(small):
    ctx, graph = small(32)
    keys = small_keys(graph)
    _set(ctx, keys)
    st, want = _check(ctx, graph, keys, [A2], 1024)
    # T9 shares sources with A2 (a true intersection of 5) but has sixty other in-links: the bloom gate decides, the literal form says how
    assert dict(want["candidates"])[T9] == 5 and st["pairs_gated"] > 0


def test_in_list_cuts_at_128_and_512(long):
    ctx, graph = long
    nodes = lref.id_ints(graph[0])
    for salt in (0, 1):
        keys = [(v, _mix(v, salt) >> 1) for v in nodes]
        _set(ctx, keys)
        st, want = _check(ctx, graph, keys, [A3, A4], 300)
        assert want["nb"] == 256 and want["apply"] and want["bound"] == 64  # 128 of A3's 513 sources and 128 of A4's 129
        assert st["forward_entries"] == 768 and HUB in dict(want["candidates"])  # HUB: a candidate with more than 512 in-links
        _check(ctx, graph, keys, [A4], 300)
        _check(ctx, graph, keys, [A3, A3, 77], 7)


def test_bloom_over_the_512_entries_only(gpu_ctx_factory):
    """The bloom bit of a small id v is (21 v) mod 64 (the multiplier is 21 mod 64).  LIKED has 513 in-links: the 512 with the smallest
    ids (no key set: NodeID order) all carry bit 41, the 513th, FAR, bit 0.  CAND is reached from the best source and has five in-links
    with five different bits, among them 41 and FAR's 0.  With the mask of the 512 entries the gate says 4 x 1 < 5: score 0; a mask of
    the whole in-list would say 4 x 2 >= 5 and intersect."""
    LIKED, CAND, FAR = 7, 50000, 40000
    near = [64 * j + 5 for j in range(1, 513)]
    assert {(21 * v) % 64 for v in near} == {41} and [(21 * v) % 64 for v in (FAR, 40001, 40002, 40003)] == [0, 21, 42, 63]
    graph = sref.layered({LIKED: near + [FAR]}, {near[0]: [CAND], FAR: [CAND]}, [(40001, CAND), (40002, CAND), (40003, CAND)])
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        st, want = _check(ctx, graph, [], [LIKED], 10)
        assert want["candidates"] == [(CAND, 1)] and want["top"] == [(CAND, 0.0)] and (want["gated"], want["intersected"]) == (1, 0)
        assert want["nb"] == 128 and want["forward_entries"] == 129  # (every source of B links to LIKED, the best one to CAND as well)
        # the control: with FAR's key the best of all it is inside the 512, the mask has both bits, and the pair is intersected
        keys = [(FAR, 0)]
        _set(ctx, keys)
        st, want = _check(ctx, graph, keys, [LIKED], 10)
        assert (want["gated"], want["intersected"]) == (0, 1) and want["top"][0][1] > 0.0 and want["candidates"] == [(CAND, 2)]


@pytest.mark.parametrize("flags", [SPREAD, NO_SHORTCUT, SPREAD | NO_SHORTCUT])
def test_debug_flags_change_nothing(small, long, flags):
    ctx, graph = small(33)
    keys = small_keys(graph)
    _set(ctx, keys)
    _check(ctx, graph, keys, [A1, A2], 300, flags)
    ctx, graph = long
    keys = [(v, _mix(v, 5) >> 1) for v in lref.id_ints(graph[0])]
    _set(ctx, keys)
    _check(ctx, graph, keys, [A3, A4], 300, flags)


def test_no_key_set_and_keys_from_ranks(gpu_ctx_factory):
    graph = small_graph(33)
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        _check(ctx, graph, [], [A1, A2], 100)  # before any hb_links_set_keys: NodeID order
        ctx.run()
        ids, _ = ctx.results()
        ranks = ctx.ranks()
        ctx.links_set_keys(from_ranks=True)
        _check(ctx, graph, list(zip(lref.id_ints(ids), ranks.tolist())), [A1, A2, A1], 100)


# refusals and state
def _raw(ctx, **fields):
    o = _lib.HbSimilarOptions()
    o.struct_size = ctypes.sizeof(_lib.HbSimilarOptions)
    o.limit = 3
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        setattr(o, k, v)
    ctx._check(ctx.lib.hb_similar_hosts(ctx.h, ctypes.byref(o), None))


_ONE = ids_from_ints([A1])
REFUSALS = {
    "limit 0": lambda ctx: ctx.similar_hosts(_ONE, 0),
    "limit 1025": lambda ctx: ctx.similar_hosts(_ONE, 1025),
    "no liked host": lambda ctx: ctx.similar_hosts(np.zeros(0, dtype=_lib.U128), 3),
    "nodes NULL": lambda ctx: _raw(ctx, node_count=1),
    "opt NULL": lambda ctx: ctx._check(ctx.lib.hb_similar_hosts(ctx.h, None, None)),
    "257 distinct liked hosts": lambda ctx: ctx.similar_hosts(ids_from_ints(list(range(SINGLE0, SINGLE0 + 257))), 3),
    "open run": lambda ctx: ctx.similar_hosts(_ONE, 3),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusal_keeps_the_previous_results(small, which):
    ctx, graph = small(32)
    keys = small_keys(graph)
    _set(ctx, keys)
    ctx.backlinks(ids_from_ints([A1, A2, T9]), 7)
    links = tuple(a.tobytes() for a in ctx.links_copy())
    _check(ctx, graph, keys, [A1, A2], 40)
    before = tuple(a.tobytes() for a in ctx.similar_copy() + ctx.similar_candidates())
    if which == "open run":
        ctx.begin()
    with pytest.raises(_lib.HyperballError) as e:
        REFUSALS[which](ctx)
    assert e.value.code == _lib.HB_ERR_INVALID and "hb_similar_hosts" in str(e.value), which
    if which == "open run":
        ctx.finish()
    assert tuple(a.tobytes() for a in ctx.similar_copy() + ctx.similar_candidates()) == before
    assert tuple(a.tobytes() for a in ctx.links_copy()) == links  # the user's links result is still readable, across the calls above too
    _check(ctx, graph, keys, [A1, A2], 40)
    assert tuple(a.tobytes() for a in ctx.similar_copy() + ctx.similar_candidates()) == before
    if which == "257 distinct liked hosts":
        ctx.similar_hosts(ids_from_ints(list(range(SINGLE0, SINGLE0 + 256)) + [SINGLE0, 31337]), 3)  # 256 distinct known ones are allowed


def test_refusals_of_the_entry(gpu_ctx_factory):
    def refused(fn, who):
        with pytest.raises(_lib.HyperballError) as e:
            fn()
        assert e.value.code == _lib.HB_ERR_INVALID and who in str(e.value)

    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        refused(lambda: ctx.similar_hosts(_ONE, 3), "hb_similar_hosts")  # no graph loaded
        refused(ctx.similar_copy, "hb_similar_count")
        ctx.load_dense(*small_graph(4))
        refused(ctx.similar_copy, "hb_similar_count")  # no result yet
        refused(ctx.similar_candidates, "hb_similar_candidates")
        ctx.similar_hosts(_ONE, 3)
        ids, scores = ctx.similar_copy()
        assert len(ids) == 3
        small_buf = np.zeros(2, dtype=_lib.U128)
        refused(lambda: ctx._check(ctx.lib.hb_similar_copy(ctx.h, _lib._ptr(small_buf), None, 2)), "hb_similar_copy")
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        refused(lambda: ctx.similar_hosts(_ONE, 3), "hb_similar_hosts")


def test_neighbours_and_reload(gpu_ctx_factory):
    graph = small_graph(33)
    keys = small_keys(graph)
    with gpu_ctx_factory(chunk=4) as ctx:
        ctx.load_dense(*graph)
        ctx.run()
        h0, r0 = ctx.state_hash(), ctx.results()
        d0 = ctx.distances(ids_from_ints([SRC0, SRC0 + 3]))[:2]
        _set(ctx, keys)
        ctx.forwardlinks(ids_from_ints([SRC0, SRC0 + 1]), 9)
        links = tuple(a.tobytes() for a in ctx.links_copy())
        before = ctx.stats()["device_bytes"]
        st, _ = _check(ctx, graph, keys, [A1, A2], 64)
        assert ctx.stats()["device_bytes"] >= before + st["device_bytes"] > before
        mine = tuple(a.tobytes() for a in ctx.similar_copy() + ctx.similar_candidates())
        assert ctx.state_hash() == h0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ctx.distance_copy(), d0))
        assert tuple(a.tobytes() for a in ctx.links_copy()) == links
        ctx.run()
        ctx.backlinks(ids_from_ints([A1]), 3)
        assert ctx.state_hash() == h0 and tuple(a.tobytes() for a in ctx.similar_copy() + ctx.similar_candidates()) == mine
        st2, _ = _check(ctx, graph, keys, [A1, A2], 64)
        assert st2["device_bytes"] == st["device_bytes"]
        ctx.load_dense(*small_graph(5))  # a reload: the result of the first graph does not answer for the second
        with pytest.raises(_lib.HyperballError):
            ctx.similar_copy()
        _check(ctx, small_graph(5), [], [A1, A2], 8)


def test_python_mirror(small):
    from stract_amd import similar_hosts
    ctx, graph = small(32)
    keys = small_keys(graph)
    _set(ctx, keys)
    liked = [A1, A2]
    finder = similar_hosts.SimilarHostsFinder(ctx, max_similar_hosts=50)
    want = sref.literal(*graph, keys, liked, min(20 + 2 + 30, 1024))["top"]
    got = finder.find_similar_hosts(liked, 20)
    assert [v for v, _ in got] == [v for v, _ in want[:20]] and _bits([s for _, s in got]) == _bits([s for _, s in want[:20]])
    assert len(finder.find_similar_hosts(liked, 500)) == 50  # max_similar_hosts
    domain_of = lambda v: None if v % 7 == 0 else v // 16  # noqa: E731  (a host without a root domain is dropped)
    got = finder.find_similar_hosts(liked + [M8], 20, domain_of=domain_of)
    want = sref.literal(*graph, keys, liked + [M8], 20 + 3 + 30)["top"]
    banned = {domain_of(a) for a in liked + [M8]}
    filtered = [(v, s) for v, s in want if domain_of(v) is not None and domain_of(v) not in banned]
    assert [v for v, _ in got] == [v for v, _ in filtered[:20]] and _bits([s for _, s in got]) == _bits([s for _, s in filtered[:20]])
    assert len(filtered) < len(want) and any(M8 // 16 == v // 16 for v, _ in want)  # hosts of a liked domain were there to drop
    assert len({domain_of(v) for v, _ in got}) < len(got)  # two hosts of one other domain both stay (similar_hosts.rs:250-270)


# C2 size, keys from ranks, eight liked hosts of high in-degree, against the numpy form of the restatement (the only case above a second)
def test_c2_against_numpy(gpu_ctx_factory):
    from stract_amd import synth
    g = synth.make_config("C2")[0]
    graph = (np.asarray(g.ids), np.asarray(g.row_ptr), np.asarray(g.src))
    state = sref.numpy_state(*graph)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        rids, _ = ctx.results()
        key = np.full(g.n, U64_MAX, dtype=np.uint64)
        key[sref.sids_of_subset(graph[0], rids)] = ctx.ranks()
        ctx.links_set_keys(from_ranks=True)
        indeg = np.diff(state["rp"])
        top = np.argsort(-indeg, kind="stable")[:8]
        assert int(indeg[top].min()) > 512
        liked = [sref._node(graph[0], int(s)) for s in top]
        want = sref.numpy_form(state, key, liked, 200)
        st = ctx.similar_hosts(graph[0][top], 200)
        cids, ccounts = ctx.similar_candidates()
        assert list(zip(lref.id_ints(cids), ccounts.tolist())) == want["candidates"]
        ids, scores = ctx.similar_copy()
        assert lref.id_ints(ids) == [v for v, _ in want["top"]] and _bits(scores) == _bits([s for _, s in want["top"]])
        assert st["nb"] == want["nb"] > 32 and st["taken"] == want["taken"] > 0 and st["candidates"] == len(want["candidates"]) > 0
        assert (st["forward_entries"], st["distinct_targets"]) == (want["forward_entries"], want["distinct_targets"])
        assert (st["pairs_gated"], st["pairs_intersected"]) == (want["gated"], want["intersected"]) and st["pairs_intersected"] > 0
