"""hb_score_hosts (Scorer::score of the result hosts of one or several searches, include/hyperball.h) against the restatement in
tests/score_hosts_ref.py and against the route it replaces on the same context: hb_inbound_similarity + hb_similarity_lookup.

Comparison rule: EVERYTHING is exact - every score by its f64 bit pattern, every stats counter as an integer.  The restatement's numpy
form is used on the generated graphs (tests/test_score_hosts_ref.py shows it equal to the literal one); the hand-written cases of
tests/golden/score_hosts_cases.json run against the values written into the file."""
import ctypes
import json

import numpy as np
import pytest

from stract_amd import _lib, synth
from stract_amd.harmonic import ids_from_ints
from tests import fans
from tests import graphs
from tests import inbound_similarity_ref as sref
from tests import limited_similarity_ref as lref
from tests import score_hosts_ref as ref
from tests import similar_hosts_ref as shref
from tests.test_score_hosts_ref import GOLDEN

pytestmark = pytest.mark.gpu

SPREAD, NO_SHORTCUT = _lib.HB_LINKS_SPREAD_ORDS, _lib.HB_LINKS_NO_SHORTCUT
COUNTERS = ("requests", "anchors", "nodes", "unknown_anchors", "unknown_nodes", "distinct", "pairs") + ref.CLASSES
STRANGER = 1 << 100


def _load(factory, graph, chunk=0):
    ctx = factory(flags=_lib.HB_FLAG_ALL_RELS, chunk=chunk)
    ctx.load_dense(*graph)
    return ctx


def _set(ctx, keys):
    if keys:
        ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
    else:
        ctx.links_set_keys()


def _arrays(req):
    out = dict(req)
    for k in ("liked", "disliked", "nodes"):
        out[k] = ids_from_ints(list(req.get(k, ())))
    return out


def _raw(scores):
    return [np.asarray(s, dtype=np.float64).tobytes() for s in scores]


def _assert_scores(got, want, what):
    assert len(got) == len(want), what
    for r, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
        assert g.shape == w.shape, (what, r)
        bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
        assert not len(bad), (what, "request %d" % r, bad[:5], g[bad[:5]], w[bad[:5]])


def _score(ctx, requests, limit, **kw):
    st = ctx.score_hosts([_arrays(r) for r in requests], limit=limit, **kw)
    return ctx.score_copy(), st


def _check(ctx, cut, requests, limit, what="", contract=False, **kw):
    """one call against the restatement on the cut graph: the scores of every request, every counter; contract: each request also
    against hb_inbound_similarity + hb_similarity_lookup on this context.  Returns (scores, stats)"""
    want, wst = ref.numpy_form(cut, requests)
    got, st = _score(ctx, requests, limit, **kw)
    tag = "%s limit %d %s" % (what, limit, kw)
    _assert_scores(got, want, tag)
    assert {k: st[k] for k in COUNTERS} == {k: wst[k] for k in COUNTERS}, tag
    assert st["pieces"] >= (1 if st["nodes"] else 0) and st["device_bytes"] > 0
    if contract:
        for r, req in enumerate(requests):
            liked, disliked, nodes, normalized, self_score = ref.fields(req)
            if not liked and not disliked:
                continue  # (hb_inbound_similarity refuses a call without an entry)
            ctx.inbound_similarity(ids_from_ints(liked), ids_from_ints(disliked), normalized=normalized, self_score=req.get("self_score"), limit=limit)
            _assert_scores([ctx.similarity_lookup(ids_from_ints(nodes))], [got[r]], "the lookup route, request %d %s" % (r, tag))
        again = ctx.score_copy()  # the other operator left this one's result alone
        assert _raw(again) == _raw(got)
    return got, st


def _cut(graph, keys, limit):
    return lref.cut_graph(*graph, lref.key_by_sid(graph[0], keys) if keys else None, limit)


# ---- (1) the hand-written cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small_pieces", [False, True])
def test_golden_cases(gpu_ctx_factory, small_pieces):
    with open(GOLDEN) as f:
        g = json.load(f)
    graph = graphs.dense_from_tuples([tuple(e) for e in g["edges"]])
    with _load(gpu_ctx_factory, graph) as ctx:
        for case in g["cases"]:
            (got,), st = _score(ctx, [case], 512, small_pieces=small_pieces)
            _assert_scores([got], [case["expect"]], case["name"])
            assert [st[k] for k in ref.CLASSES] == case["classes"], case["name"]
        got, st = _score(ctx, g["cases"], 512, small_pieces=small_pieces)
        _assert_scores(got, [c["expect"] for c in g["cases"]], "all cases in one call")
        assert [st[k] for k in ref.CLASSES] == [sum(c["classes"][i] for c in g["cases"]) for i in range(4)]
        assert (st["unknown_anchors"], st["unknown_nodes"]) == (1, 2)


# ---- (2) list lengths ---------------------------------------------------------------------------------------------------------------------
FAN_KS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def _fan_graph():
    """the flipped fan - hub h_K has the in-list of length K - plus, per hub, a twin with the same in-list and a half twin with every
    second entry of it: lists of the lengths 0, 1, 63 .. 513 and their halves on both sides of a pair, overlapping in known amounts"""
    fan = fans.Fan(FAN_KS)
    t = fan.tuples(flipped=True)
    nxt = fan.n + 1
    twin, half = {}, {}
    for K in FAN_KS:
        leaves = (fan.leaves(K) + 1).tolist()
        twin[K], half[K] = nxt, nxt + 1
        nxt += 2
        t += [(v, twin[K]) for v in leaves] + [(v, half[K]) for v in leaves[1::2]] + [(twin[K], nxt + 5), (half[K], nxt + 5)]
    return fan, graphs.dense_from_tuples(t), twin, half


def _fan_requests(fan, twin, half):
    hubs = [fan.hub_of(K) + 1 for K in FAN_KS]
    twins = [twin[K] for K in FAN_KS]
    halves = [half[K] for K in FAN_KS]
    leaf = int(fan.leaves(65)[0]) + 1
    every = hubs + twins + halves
    return [dict(liked=hubs + [twins[3], STRANGER], disliked=halves[2:6], nodes=every + [leaf, fan.r + 1, STRANGER], normalized=True),
            dict(liked=twins[::-1], disliked=[hubs[10], hubs[9]], nodes=every[::-1], self_score=0.75),
            dict(liked=[hubs[10]], nodes=twins + [hubs[10]])]


FAN_LIMITS = (1, 2, 64, 512, 1024, 65, 66, 513, 514)  # (64, 65, 66 around h_65; 512, 513, 514 around h_513)


@pytest.fixture(scope="module")
def fan_ctx(gpu_ctx_factory):
    fan, graph, twin, half = _fan_graph()
    made = {}

    def get(chunk):
        if chunk not in made:
            made[chunk] = _load(gpu_ctx_factory, graph, chunk)
        return made[chunk]

    yield get, graph, _fan_requests(fan, twin, half), fan
    for ctx in made.values():
        ctx.close()


def _fan_case(ctx, graph, requests, chunk, contract=False, **kw):
    """case (2) on one context: every limit of FAN_LIMITS without a key set, then limit 64 under a key set that moves the cut and once
    more with the keys cleared; every call against the restatement.  Returns the raw scores of all calls, in order"""
    _set(ctx, [])
    assert ctx.plan()["nv"] > 0
    out = []
    for limit in FAN_LIMITS:
        got, _ = _check(ctx, _cut(graph, [], limit), requests, limit, what="fan chunk %d" % chunk, contract=contract and limit in (64, 512), **kw)
        out.append(_raw(got))
    # a key set that moves the cut: every third leaf becomes the best, so a hub and its half twin keep other shares of each other
    ints = sref.id_ints(graph[0])
    keys = [(v, v % 3) for v in ints]
    _set(ctx, keys)
    a, _ = _check(ctx, _cut(graph, keys, 64), requests, 64, what="fan, keys", contract=contract, **kw)
    _set(ctx, [])
    b, _ = _check(ctx, _cut(graph, [], 64), requests, 64, what="fan, keys cleared", **kw)
    assert _raw(a) != _raw(b)  # (the half twins hold every second leaf: which 64 a cut keeps decides their overlap)
    return out + [_raw(a), _raw(b)]


@pytest.mark.parametrize("chunk", [0, 4])
def test_list_lengths(fan_ctx, chunk):
    get, graph, requests, fan = fan_ctx
    _fan_case(get(chunk), graph, requests, chunk, contract=True)


# ---- (3) the gate at its boundary -----------------------------------------------------------------------------------------------------------
def test_gate_boundary(gpu_ctx_factory):
    # bloom bit of id x = (21 x) & 63: 1 .. 9 carry nine different bits.  A has 8 of them, B all 9, V shares two sources with both:
    # 4 x 2 == 8 == max: intersected; 4 x 2 == 9 - 1 < 9: gated, although the true intersection is 2
    A, B, V = 100, 101, 102
    assert len({(21 * x) & 63 for x in range(1, 10)}) == 9
    graph = graphs.dense_from_tuples([(x, A) for x in range(1, 9)] + [(x, B) for x in range(1, 10)] + [(1, V), (2, V)])
    with _load(gpu_ctx_factory, graph) as ctx:
        (got,), st = _check(ctx, _cut(graph, [], 512), [dict(liked=[A, B], nodes=[V])], 512, what="gate", contract=True)
        assert (st["pairs_gated"], st["pairs_intersected"]) == (1, 1)
        assert got[0] == 2.0 / (np.sqrt(8.0) * np.sqrt(2.0))


def test_bloom_over_the_cut_entries_only(gpu_ctx_factory):
    """tests/test_similar_hosts.py test_bloom_over_the_512_entries_only: LIKED has 513 in-links, the 512 with the smallest ids all carry
    bloom bit 41, the 513th, FAR, bit 0.  CAND has five in-links with five different bits, among them 41 and 0.  Over the 512 best the
    gate says 4 x 1 < 5; with FAR's key the best of all the mask has both bits: 4 x 2 >= 5."""
    LIKED, CAND, FAR = 7, 50000, 40000
    near = [64 * j + 5 for j in range(1, 513)]
    graph = shref.layered({LIKED: near + [FAR]}, {near[0]: [CAND], FAR: [CAND]}, [(40001, CAND), (40002, CAND), (40003, CAND)])
    req = [dict(liked=[LIKED], nodes=[CAND, LIKED])]
    with _load(gpu_ctx_factory, graph, 4) as ctx:
        (got,), st = _check(ctx, _cut(graph, [], 512), req, 512, what="gated", contract=True)
        assert got[0] == 0.0 and st["pairs_gated"] == 1
        keys = [(FAR, 0)]
        _set(ctx, keys)
        (got,), st = _check(ctx, _cut(graph, keys, 512), req, 512, what="not gated", contract=True)
        assert got[0] > 0.0 and st["pairs_gated"] == 0
        (got,), _ = _check(ctx, _cut(graph, keys, 513), req, 513, what="one more entry")
        assert got[0] > 0.0


# ---- (4) request counts ------------------------------------------------------------------------------------------------------------------------
def _lcg(self_links=(3, 50, 120, 199)):
    return graphs.dense_from_tuples(graphs.lcg_graph() + [(v, v) for v in self_links] + [(500, 1)])


def _requests(ints, count):
    """`count` requests over shared hosts: one without nodes, one without anchors, one with disliked hosts only; duplicates, ids that
    are no node, a host without in-links (500), hosts with self links (3, 50)"""
    out = []
    for r in range(count):
        liked = ints[r % 7::11][:3 + r % 5] + [3]
        disliked = ints[(r * 3) % 13::17][:r % 4]
        nodes = ints[r % 5::9][:6 + r % 7] + [3, 500, STRANGER + r % 2]
        req = dict(liked=liked, disliked=disliked, nodes=nodes, normalized=r % 2 == 0)
        if r % 3 == 1:
            req["self_score"] = 0.5 + r
        out.append(req)
    out[0].update(liked=out[0]["liked"] + [out[0]["liked"][0], STRANGER, 500], disliked=[ints[40], ints[40], STRANGER + 7],
                  nodes=out[0]["nodes"] + out[0]["nodes"][:2] + [50])
    if count > 1:
        out[1] = dict(liked=[], disliked=[50, ints[8], 500], nodes=[50, ints[8], ints[9], 500])  # disliked hosts only
    if count > 2:
        out[2] = dict(liked=ints[:5], disliked=ints[5:7], nodes=[])                          # no nodes
        out[3] = dict(nodes=ints[:9] + [STRANGER], normalized=True)                          # no anchors
    return out


@pytest.fixture(scope="module")
def lcg_ctx(gpu_ctx_factory):
    graph = _lcg()
    ctx = _load(gpu_ctx_factory, graph, 4)
    yield ctx, graph, sref.id_ints(graph[0])
    ctx.close()


@pytest.mark.parametrize("count", [1, 2, 33])
def test_request_counts(lcg_ctx, count):
    ctx, graph, ints = lcg_ctx
    _set(ctx, [])
    requests = _requests(ints, count)
    cut = _cut(graph, [], 3)
    got, st = _check(ctx, cut, requests, 3, what="%d requests" % count, contract=count <= 2)
    assert st["requests"] == count and st["distinct"] < st["anchors"] + st["nodes"]  # shared hosts: each looked up once
    order = list(range(count))[::-1]
    back, st2 = _check(ctx, cut, [requests[i] for i in order], 3, what="reversed")
    assert _raw(back) == _raw([got[i] for i in order])
    assert {k: st2[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}
    if count > 2:
        assert len(got[2]) == 0 and got[3].tolist() == [0.0] * 10  # no nodes: an empty slice; no anchors: max(0, 0)


# ---- (5) small pieces and the debug flags of the list selects ---------------------------------------------------------------------------------
VARIANTS = [(0, True, 0), (SPREAD, False, 0), (NO_SHORTCUT, False, 0), (SPREAD | NO_SHORTCUT, True, 5)]


@pytest.mark.parametrize("flags,small_pieces,slots", VARIANTS)
def test_request_counts_under_small_pieces_and_debug_flags(lcg_ctx, flags, small_pieces, slots):
    ctx, graph, ints = lcg_ctx
    _set(ctx, [])
    for count in (1, 2, 33):
        requests = _requests(ints, count)
        plain, st0 = _score(ctx, requests, 3)
        got, st = _check(ctx, _cut(graph, [], 3), requests, 3, what="flags", flags=flags, small_pieces=small_pieces, slots_per_batch=slots)
        assert _raw(got) == _raw(plain)
        order = list(range(count))[::-1]  # the same requests in another order: the same slices
        back, _ = _check(ctx, _cut(graph, [], 3), [requests[i] for i in order], 3, what="flags, reversed", flags=flags, small_pieces=small_pieces,
                         slots_per_batch=slots)
        assert _raw(back) == _raw([plain[i] for i in order])
        if small_pieces:  # 64 pairs a piece: boundaries inside a request and, where a request has more than 64 anchors ..., inside a node's list
            assert st["pieces"] > st0["pieces"] >= 1 and st["pieces"] >= st["pairs"] // 64


@pytest.mark.parametrize("chunk", [0, 4])
@pytest.mark.parametrize("flags,small_pieces,slots", VARIANTS)
def test_list_lengths_under_small_pieces_and_debug_flags(fan_ctx, chunk, flags, small_pieces, slots):
    """everything of test_list_lengths again - every limit, both chunks, the key set that moves the cut - byte-identical"""
    get, graph, requests, fan = fan_ctx
    ctx = get(chunk)
    plain = _fan_case(ctx, graph, requests, chunk)
    assert _fan_case(ctx, graph, requests, chunk, flags=flags, small_pieces=small_pieces, slots_per_batch=slots) == plain
    if small_pieces:
        assert _score(ctx, requests, 512, small_pieces=True)[1]["pieces"] > _score(ctx, requests, 512)[1]["pieces"] == 1


def test_a_piece_boundary_inside_a_nodes_anchor_list(lcg_ctx):
    ctx, graph, ints = lcg_ctx
    _set(ctx, [])
    # 150 liked and 70 disliked entries: with 64 pairs a piece every node's sums cross three boundaries on the liked side and one on the other
    req = [dict(liked=(ints[:60] + [3, STRANGER]) * 3, disliked=ints[20:90][::-1], nodes=ints[10:16] + [3, STRANGER, 500], normalized=True, self_score=1.25),
           dict(liked=ints[5:8], nodes=ints[:30])]
    assert len(req[0]["liked"]) > 128 and len(req[0]["disliked"]) > 64
    plain, st0 = _check(ctx, _cut(graph, [], 4), req, 4, what="whole pieces", contract=True)
    got, st = _check(ctx, _cut(graph, [], 4), req, 4, what="small pieces", small_pieces=True)
    assert _raw(got) == _raw(plain) and st0["pieces"] == 1 and st["pieces"] >= 9 * 4 + 1


# ---- (6) the contract on larger graphs -----------------------------------------------------------------------------------------------------------
def _with_self_links(g, rows):
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    pair = np.unique(np.concatenate([row * len(rp) + np.asarray(g.src, dtype=np.int64), np.asarray(rows, dtype=np.int64) * (len(rp) + 1)]))
    row, src = pair // len(rp), pair % len(rp)
    return np.asarray(g.ids), np.concatenate([[0], np.cumsum(np.bincount(row, minlength=len(rp) - 1))]).astype(np.uint64), src.astype(np.uint32)


@pytest.mark.parametrize("which", ["lcg", "c1"])
def test_contract_with_the_lookup_route(gpu_ctx_factory, which):
    if which == "lcg":
        graph = _lcg()
    else:
        g = synth.make_config("C1")[0]
        indeg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
        graph = _with_self_links(g, np.argsort(-indeg, kind="stable")[[0, 3, 40, 900]])
    ints = sref.id_ints(graph[0])
    indeg = np.diff(np.asarray(graph[1], dtype=np.int64))
    hubs = [ints[i] for i in np.argsort(-indeg, kind="stable")[:40]]
    rng = np.random.default_rng(5)
    rand = [ints[i] for i in rng.integers(0, len(ints), 60)]
    requests = [dict(liked=hubs[:6] + rand[:4], disliked=hubs[6:8] + [rand[5]], nodes=hubs[:20] + rand[:30] + [STRANGER], normalized=True),
                dict(liked=rand[10:14] + [hubs[0], hubs[0]], disliked=[hubs[3]], nodes=hubs[:10] + rand[5:25], self_score=0.25),
                dict(liked=[hubs[1]], nodes=rand + hubs)]
    with _load(gpu_ctx_factory, graph, 4 if which == "lcg" else 0) as ctx:
        for keyed in (False, True):
            keys = []
            if keyed:
                ctx.run()
                ids, _ = ctx.results()
                keys = list(zip(sref.id_ints(ids), ctx.ranks().tolist()))
                ctx.links_set_keys(from_ranks=True)
            for limit in (8, 512):
                _check(ctx, _cut(graph, keys, limit), requests, limit, what="%s keyed %s" % (which, keyed), contract=True)
        # the candidates of hb_similar_hosts as nodes, its liked hosts as the only anchors: its scores
        liked = hubs[:3] + [rand[0]]
        ctx.similar_hosts(ids_from_ints(liked), 1024)
        cids, cscores = ctx.similar_copy()
        assert len(cids) > 3
        got, _ = _score(ctx, [dict(liked=liked, nodes=sref.id_ints(cids), normalized=True)], 512)
        _assert_scores(got, [cscores], "hb_similar_copy")
        ids2, scores2 = ctx.similar_copy()
        assert ids2.tobytes() == cids.tobytes() and scores2.tobytes() == cscores.tobytes()


# ---- (8) refusals ---------------------------------------------------------------------------------------------------------------------------------
_ONE = [dict(liked=[3], nodes=[50])]


def _call(ctx, fill):
    """hb_score_hosts through the raw structs, `fill(options, request)` having its way with them"""
    node = ids_from_ints([50])
    q = _lib.HbScoreRequest()
    q.nodes, q.node_count = node.ctypes.data, 1
    o = _lib.HbScoreOptions()
    o.struct_size = ctypes.sizeof(_lib.HbScoreOptions)
    o.requests, o.request_count, o.limit = ctypes.pointer(q), 1, 4
    fill(o, q)
    ctx._check(ctx.lib.hb_score_hosts(ctx.h, ctypes.byref(o), None))


def _set_attr(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


REFUSALS = {
    "opt NULL": lambda ctx: ctx._check(ctx.lib.hb_score_hosts(ctx.h, None, None)),
    "no request": lambda ctx: ctx.score_hosts([], limit=4),
    "4097 requests": lambda ctx: ctx.score_hosts([dict(nodes=ids_from_ints([50]))] * 4097, limit=4),
    "requests NULL": lambda ctx: _call(ctx, lambda o, q: _set_attr(o, requests=None)),
    "liked NULL": lambda ctx: _call(ctx, lambda o, q: _set_attr(q, liked_count=2)),
    "disliked NULL": lambda ctx: _call(ctx, lambda o, q: _set_attr(q, disliked_count=2)),
    "nodes NULL": lambda ctx: _call(ctx, lambda o, q: _set_attr(q, nodes=None)),
    "limit 0": lambda ctx: ctx.score_hosts([_arrays(r) for r in _ONE], limit=0),
    "limit 1025": lambda ctx: ctx.score_hosts([_arrays(r) for r in _ONE], limit=1025),
    "slots_per_batch": lambda ctx: ctx.score_hosts([_arrays(r) for r in _ONE], limit=4, slots_per_batch=65537),
    "too many entries": lambda ctx: _call(ctx, lambda o, q: _set_attr(q, node_count=(1 << 24) + 1)),
    "open run": lambda ctx: ctx.score_hosts([_arrays(r) for r in _ONE], limit=4),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusal_keeps_the_previous_results(lcg_ctx, which):
    ctx, graph, ints = lcg_ctx
    _set(ctx, [])
    ctx.backlinks(ids_from_ints(ints[:5]), 7)
    links = tuple(a.tobytes() for a in ctx.links_copy())
    ctx.similar_hosts(ids_from_ints(ints[:3]), 20)
    similar = tuple(a.tobytes() for a in ctx.similar_copy())
    ctx.inbound_similarity(ids_from_ints(ints[:4]), limit=3)
    sim = ctx.similarity_all().tobytes()
    requests = _requests(ints, 2)
    before, _ = _check(ctx, _cut(graph, [], 3), requests, 3, what="before")
    if which == "open run":
        ctx.begin()
        ctx.step()
    with pytest.raises(_lib.HyperballError) as e:
        REFUSALS[which](ctx)
    assert e.value.code == _lib.HB_ERR_INVALID and "hb_score_hosts" in str(e.value), which
    if which == "open run":
        ctx.step()
        ctx.finish()
    assert _raw(ctx.score_copy()) == _raw(before)
    assert tuple(a.tobytes() for a in ctx.links_copy()) == links and tuple(a.tobytes() for a in ctx.similar_copy()) == similar
    assert ctx.similarity_all().tobytes() == sim
    _check(ctx, _cut(graph, [], 3), requests, 3, what="after")


def _refused(fn, who):
    with pytest.raises(_lib.HyperballError) as e:
        fn()
    assert e.value.code == _lib.HB_ERR_INVALID and who in str(e.value)


def test_refusals_of_the_entry(gpu_ctx_factory):
    """no graph, no result yet, a short buffer, world_size > 1.  A context without a graph and a multi-rank context can hold no
    previous result of any of these operators (each of them refuses there), so there is nothing to read back after these two"""
    one = [_arrays(r) for r in _ONE]
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        _refused(lambda: ctx.score_hosts(one, limit=4), "hb_score_hosts")  # no graph loaded
        _refused(ctx.score_copy, "hb_score_count")
        ctx.load_dense(*_lcg())
        _refused(ctx.score_copy, "hb_score_count")  # no result yet
        ctx.score_hosts(one, limit=4)
        (got,) = ctx.score_copy()
        assert len(got) == 1
        ctx.score_hosts([dict(nodes=ids_from_ints([3, 50, 7]))], limit=4)
        small = np.zeros(2, dtype=np.float64)
        _refused(lambda: ctx._check(ctx.lib.hb_score_copy(ctx.h, None, _lib._ptr(small), 2)), "hb_score_copy")
        offsets = np.zeros(2, dtype=np.uint64)
        ctx._check(ctx.lib.hb_score_copy(ctx.h, _lib._ptr(offsets), None, 0))  # the offsets alone need no room for scores
        assert offsets.tolist() == [0, 3]
    with gpu_ctx_factory(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL) as ctx:
        _refused(lambda: ctx.score_hosts(one, limit=4), "hb_score_hosts")


def _star(n):
    """n + 1 nodes: node 1 (sid 0) has every other node as an in-neighbour"""
    all_ids = np.zeros(n + 1, dtype=_lib.U128)
    all_ids["lo"] = np.arange(1, n + 2, dtype=np.uint64)
    row_ptr = np.zeros(n + 2, dtype=np.uint64)
    row_ptr[1:] = n
    return all_ids, row_ptr, np.arange(1, n + 1, dtype=np.uint32)


def test_too_many_distinct_hosts(gpu_ctx_factory):
    """the one refusal that comes after the ids are resolved: 262145 distinct known hosts, on a context that holds a score result and
    the results of the links, similar-hosts and similarity operators - all four are read back unchanged"""
    n = 262145
    all_ids, row_ptr, src = _star(n)
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        ctx.load_dense(all_ids, row_ptr, src)
        ctx.backlinks(all_ids[:3], 7)
        links = tuple(a.tobytes() for a in ctx.links_copy())
        ctx.similar_hosts(all_ids[:1], 20)
        similar = tuple(a.tobytes() for a in ctx.similar_copy())
        ctx.inbound_similarity(all_ids[:2], limit=3)
        sim = ctx.similarity_lookup(all_ids[:50]).tobytes()
        ctx.score_hosts([dict(liked=all_ids[:2], nodes=all_ids[:9])], limit=3)
        before = _raw(ctx.score_copy())
        _refused(lambda: ctx.score_hosts([dict(nodes=all_ids[:n])], limit=1), "262144")
        assert _raw(ctx.score_copy()) == before
        assert tuple(a.tobytes() for a in ctx.links_copy()) == links and tuple(a.tobytes() for a in ctx.similar_copy()) == similar
        assert ctx.similarity_lookup(all_ids[:50]).tobytes() == sim


def test_262144_distinct_hosts_are_allowed(gpu_ctx_factory):
    all_ids, row_ptr, src = _star(262145)
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        ctx.load_dense(all_ids, row_ptr, src)
        st = ctx.score_hosts([dict(liked=all_ids[:1], nodes=all_ids[:262144])], limit=1, slots_per_batch=65536)
        assert st["distinct"] == 262144 and st["pairs_self"] == 1
        (got,) = ctx.score_copy()
        assert got[0] == 1.0 and not got[1:].any()


# ---- (9) state -----------------------------------------------------------------------------------------------------------------------------------------
def test_state_of_the_other_operators_and_reload(gpu_ctx_factory):
    g = synth.RmatGraph(11, 14_000)
    graph = (np.asarray(g.ids), np.asarray(g.row_ptr), np.asarray(g.src))
    ints = sref.id_ints(graph[0])
    requests = [dict(liked=[ints[i] for i in (7, 11, 500)], disliked=[ints[-5]], nodes=ints[:40] + [STRANGER], normalized=True),
                dict(liked=[ints[3]], nodes=ints[100:130])]
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(*graph)
        loaded = ctx.stats()["device_bytes"]
        b0 = ctx.betweenness(g.ids[[3, 11, 500]])  # (the two operators that borrow the HyperBall rows come before the run whose state is hashed)
        ctx.inbound_similarity(g.ids[[7, 11]], limit=4)
        i0 = ctx.similarity_all()
        ctx.run()
        h0, r0 = ctx.state_hash(), ctx.results()
        ctx.distances(g.ids[[11, 500]])
        d0 = ctx.distance_all()
        ctx.links_set_keys(from_ranks=True)
        keys = list(zip(sref.id_ints(r0[0]), ctx.ranks().tolist()))
        ctx.nearest_seed(from_image=True)
        n0 = ctx.nearest_seed_all()
        ctx.backlinks(g.ids[:50], 5)
        l0 = ctx.links_copy()
        ctx.similar_hosts(g.ids[[7, 11]], 50)
        s0 = ctx.similar_copy()
        before = ctx.stats()["device_bytes"]
        mine, st = _check(ctx, _cut(graph, keys, 4), requests, 4, what="state")
        assert ctx.stats()["device_bytes"] >= before + st["device_bytes"] > before
        assert ctx.state_hash() == h0 and all(a.tobytes() == b.tobytes() for a, b in zip(ctx.results(), r0))
        assert np.array_equal(ctx.distance_all(), d0) and n0.tobytes() == ctx.nearest_seed_all().tobytes()
        b1 = ctx.betweenness_copy()
        assert b0[0].tobytes() == b1[0].tobytes() and b0[1].tobytes() == b1[1].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(l0, ctx.links_copy()))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(s0, ctx.similar_copy())) and i0.tobytes() == ctx.similarity_all().tobytes()
        ctx.begin()  # between two hb_steps: refused, and the run goes on to the same end
        ctx.step()
        with pytest.raises(_lib.HyperballError) as e:
            _score(ctx, requests, 4)
        assert e.value.code == _lib.HB_ERR_INVALID and "hb_score_hosts" in str(e.value)
        while ctx.step():
            pass
        ctx.finish()
        assert ctx.state_hash() == h0 and _raw(ctx.score_copy()) == _raw(mine)
        ctx.forwardlinks(g.ids[:50], 5)
        ctx.similar_hosts(g.ids[[3]], 5)
        assert _raw(ctx.score_copy()) == _raw(mine)  # ... until the next successful call
        _, st2 = _check(ctx, _cut(graph, keys, 4), requests, 4, what="again")
        assert st2["device_bytes"] == st["device_bytes"]  # the holders only grow, and the same call needs no more
        ctx.load_dense(*graph)
        assert ctx.stats()["device_bytes"] == loaded < before  # back at the level of the first load
        with pytest.raises(_lib.HyperballError):
            ctx.score_copy()
        _check(ctx, _cut(graph, [], 4), requests, 4, what="after the reload")


# ---- (10) the Python mirror ----------------------------------------------------------------------------------------------------------------------------------
def test_python_mirror(lcg_ctx):
    from stract_amd import inbound_scorer
    ctx, graph, ints = lcg_ctx
    _set(ctx, [])
    pages = [50, 3, 50, ints[20], STRANGER, 3, 500]  # host ids of a result list: several pages of one host
    cut = _cut(graph, [], 3)
    (want,), _ = ref.numpy_form(cut, [dict(liked=[3, 50, 7], disliked=[9], nodes=pages, self_score=0.5)])
    s = inbound_scorer.InboundScorer.new(ctx, [3, 50, 7], [9], limit=3)
    s.set_self_score(0.5)
    _assert_scores([s.compute(pages)], [want], "compute")
    assert s.stats["nodes"] == 5 and s.stats["distinct"] == 6  # the unique hosts of the list, each looked up once
    searches = [([3, 50, 7], [9], pages), ([ints[5]], [], ints[:12]), ([], [], [3])]
    (many, _) = inbound_scorer.compute_many(ctx, searches, limit=3)
    want, _ = ref.numpy_form(cut, [dict(liked=a, disliked=b, nodes=c) for a, b, c in searches])
    _assert_scores(many, want, "compute_many")


# ---- (11) C2 size against the numpy form (the only case above a second) -------------------------------------------------------------------------------------------
def test_c2_against_numpy(gpu_ctx_factory):
    g = synth.make_config("C2")[0]
    graph = (np.asarray(g.ids), np.asarray(g.row_ptr), np.asarray(g.src))
    indeg = np.diff(np.asarray(graph[1], dtype=np.int64))
    top = np.argsort(-indeg, kind="stable")
    rng = np.random.default_rng(11)
    node = lambda s: (int(graph[0]["hi"][s]) << 64) | int(graph[0]["lo"][s])  # noqa: E731
    liked = [node(s) for s in top[:8]] + [node(s) for s in rng.integers(0, g.n, 8)]
    disliked = [node(s) for s in top[8:16]] + [node(s) for s in rng.integers(0, g.n, 8)]
    nodes = [node(s) for s in top[:150]] + [node(s) for s in rng.integers(0, g.n, 150)]
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        rids, _ = ctx.results()
        key = np.full(g.n, lref.U64_MAX, dtype=np.uint64)
        key[shref.sids_of_subset(graph[0], rids)] = ctx.ranks()
        ctx.links_set_keys(from_ranks=True)
        requests = [dict(liked=liked, disliked=disliked, nodes=nodes)]
        _, st = _check(ctx, ref.cut_for(*graph, key, 512, requests), requests, 512, what="C2")
        assert st["pairs"] == 32 * 300 and st["pairs_intersected"] > 0 and int(indeg[top[149]]) > 512
