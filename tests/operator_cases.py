"""One body per plan-reading operator, shared by tools/diff_fuzz.py and tests/test_layouts.py, and the layout recipe both draw from.

A body takes a loaded context, its graph() and an rng, draws its calls, and asserts every call against the CPU restatement of that
operator under the comparison rule of the operator's own suite:

    distances      tests/distance_ref.py (the literal dijkstra_multi with the u8 rule), exact
    betweenness    tests/betweenness_ref.py under bref.rtol, the rule of tests/test_betweenness.py
    similarity     tests/inbound_similarity_ref.py over the BitVecs of tests/limited_similarity_ref.py, bit for bit
    score_hosts    tests/score_hosts_ref.py and the hb_inbound_similarity + hb_similarity_lookup route, bit for bit
    nearest_seed   tests/nearest_seed_ref.py, exact
    backlinks      the _run of tests/test_links.py (tests/links_ref.py numpy_form and the stats counters), exact
    forwardlinks   the _run of tests/test_forwardlinks.py (tests/forwardlinks_ref.py), exact
    similar_hosts  the _check of tests/test_similar_hosts.py (tests/similar_hosts_ref.py), exact
    sampled        the _check of tests/test_sampled_harmonic.py (values and sample_ref.dijkstra_histogram), exact

Called with ctx = None a body only draws and runs what decides whether a call is compared at all (the betweenness restatement hitting
HB_ERR_LIMIT, a similarity round with two empty lists): the draws do not depend on anything the context answers, so the tally of such
a dry run is the tally of the run on the device.  `picks` are sids the caller read from the plan - hubs of chunk trees and members of
their lists - that the body puts among its queries, sources, liked hosts and keys besides the random ones."""
import numpy as np

from stract_amd import _lib
from stract_amd.harmonic import EdgeListGraph, ids_from_ints
from tests import graphs

NONE = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1
LIMITS = (1, 2, 3, 8, 17, 512)
SLOTS = (0, 3)
CHUNKS = (4, 8, 16, 64)
BAND_LOG2 = (1, 4, 5, 6)  # tune[3]: 1 = banding off; plan_tune() of hb_api.hip ignores 2 and 3
LAYOUT_FLAGS = (0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP, _lib.HB_FLAG_HOST_PLAN, _lib.HB_FLAG_NO_SPARSE)
PLAN_FLAGS = _lib.HB_FLAG_NO_REORDER | _lib.HB_FLAG_NO_XCD_MAP  # what the planner reads of them
UNKNOWN = 1 << 100  # ids from here on are no node of any graph of graphs.random_graph


class Picks:
    """sids read from a plan: the node rows on top of chunk trees, and sources inside those trees"""

    def __init__(self, hubs=(), members=()):
        self.hubs = [int(x) for x in hubs]
        self.members = [int(x) for x in members]

    def all(self):
        return sorted(set(self.hubs + self.members))


class Tally:
    """calls and compared calls per operator and per (operator, graph kind)"""

    def __init__(self):
        self.calls, self.compared = {}, {}

    def count(self, op, kind, compared=True):
        for key in (op, (op, kind)):
            self.calls[key] = self.calls.get(key, 0) + 1
            self.compared[key] = self.compared.get(key, 0) + int(bool(compared))

    def add(self, other):
        for key in other.calls:
            self.calls[key] = self.calls.get(key, 0) + other.calls[key]
            self.compared[key] = self.compared.get(key, 0) + other.compared[key]

    def as_dict(self):
        return {str(k): (self.compared[k], self.calls[k]) for k in sorted(self.calls, key=str)}


# ---- the layout recipe ----------------------------------------------------------------------------------------------------------------
def draw_graph(rng, kind=None):
    """graphs.random_graph (drawn again while it has no edge; kind "dead_fringe": graphs.dead_fringe_graph) with a self link on an eighth
    of its nodes"""
    while True:
        got, tuples = graphs.dead_fringe_graph(rng) if kind == "dead_fringe" else graphs.random_graph(rng, kind)
        if tuples:
            break
    nodes = sorted({x for e in tuples for x in e[:2]})
    return got, sorted(set(tuples) | {(v, v) for v in nodes if rng.integers(0, 8) == 0})


def draw_layout(rng, chunk=None):
    """(chunk, tune, flags): the cut and split knobs of the planner and two draws of the layout flags"""
    chunk = int(rng.choice(CHUNKS)) if chunk is None else int(chunk)
    tune = (0, 0, 0, int(rng.choice(BAND_LOG2)), int(rng.integers(1, 9)), int(rng.integers(0, chunk + 1)), 0)
    flags = _lib.HB_FLAG_ALL_RELS | int(rng.choice(LAYOUT_FLAGS)) | int(rng.choice(LAYOUT_FLAGS))
    return chunk, tune, flags


def load(factory, tuples, chunk, tune, flags):
    ctx = factory(flags=flags, chunk=chunk, tune=tune)
    ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
    return ctx


# ---- reading a plan -------------------------------------------------------------------------------------------------------------------
def entries(plan, row):
    rp = plan["row_ptr"]
    e = plan["src"][int(rp[row]):int(rp[row + 1])]
    return e[e != NONE].astype(np.int64)


def tree(plan, row):
    """the list of node row `row` as its lowest-level chunks in list order, [(chunk row, [node rows]), ...], and the depth of the tree;
    None for a row that reads no chunk row"""
    e = entries(plan, row)
    if not len(e) or (e < plan["n_pad"]).all():
        return None

    def below(r):
        x = entries(plan, r)
        if len(x) and (x >= plan["n_pad"]).all():
            out, depth = [], 0
            for c in x.tolist():
                sub, d = below(c)
                out += sub
                depth = max(depth, d + 1)
            return out, depth
        assert (x < plan["n_pad"]).all()
        return [(r, x.tolist())], 0

    return below(row)


CONDITIONS = ("a", "b", "c", "d", "e", "f")
LIVE_CONDITIONS = ("g", "h")  # what only a live-first plan shows


def layout_conditions(plan, row_ptr, chunk, n_live=None):
    """{condition: (hub sid, [member sids])} for the conditions the plan shows, read from the first node row that shows each:
      a  a hub with a non-final lowest-level chunk shorter than `chunk` (a band cut): the first and last entry of that chunk and the
         first entry of the chunk behind it
      b  a hub whose lowest-level chunk rows are not consecutive row numbers: the first entries of the two chunks around the gap
      c  a one-chunk tree, a node row whose list is a single chunk row: the first and the last entry of the chunk
      d  a split row whose in-degree is <= chunk: the first and the last entry of its list
      e  a tree of depth >= 3 (three levels of chunk rows under the node row): the first, a middle and the last entry of its list
      f  no chunk row at all: (None, [])
    and, where `n_live` says that the plan is a live-first one (device rows from n_live on are the hosts without an in-link, "dead"):
      g  a lowest-level chunk row whose sources are all dead: its first and its last entry
      h  a lowest-level chunk row that mixes live and dead sources: its last live and its first dead entry
    so that the hub, a live member and a dead member of such trees are among the picks."""
    if plan["nv"] == 0:
        return {"f": (None, [])}
    order = plan["order"].astype(np.int64)
    indeg = np.diff(np.asarray(row_ptr, dtype=np.int64))
    rp = plan["row_ptr"].astype(np.int64)
    found = {}

    def note(cond, hub, rows):
        if cond not in found:
            found[cond] = (int(hub), [int(order[r]) for r in rows])

    for d in range(len(order)):  # (the host planner hands out the order without its padding rows)
        sid = int(order[d])
        if sid == NONE:
            continue
        t = tree(plan, d)
        if t is None:
            continue
        chunks, depth = t
        flat = [r for _, ch in chunks for r in ch]
        assert len(flat) == indeg[sid] and all(int(rp[c + 1] - rp[c]) == len(ch) for c, ch in chunks)  # a chunk row holds no padding
        for i, (_, ch) in enumerate(chunks[:-1]):
            if len(ch) < chunk:
                note("a", sid, [ch[0], ch[-1], chunks[i + 1][1][0]])
        for (ra, ca), (rb, cb) in zip(chunks[:-1], chunks[1:]):
            if rb != ra + 1:
                note("b", sid, [ca[0], cb[0]])
        if len(entries(plan, d)) == 1:
            assert len(chunks) == 1
            note("c", sid, [flat[0], flat[-1]])
        if indeg[sid] <= chunk:
            note("d", sid, [flat[0], flat[-1]])
        if depth >= 3:
            note("e", sid, [flat[0], flat[len(flat) // 2], flat[-1]])
        if n_live is not None:
            for _, ch in chunks:
                dead = [r for r in ch if r >= n_live]
                if dead and len(dead) == len(ch):
                    note("g", sid, [ch[0], ch[-1]])
                elif dead:
                    assert ch == sorted(ch) and dead == ch[-len(dead):]  # ascending device rows: the dead sources are the list's tail
                    note("h", sid, [ch[-len(dead) - 1], dead[0]])
    return found


def picks_of(conditions):
    hubs = [hub for hub, _ in conditions.values() if hub is not None]
    members = [m for _, ms in conditions.values() for m in ms]
    return Picks(hubs, members)


def plan_equal(a, b, n):
    return (a["n_pad"] == b["n_pad"] and a["nv"] == b["nv"] and np.array_equal(a["level_begin"], b["level_begin"])
            and np.array_equal(a["order"][:n], b["order"][:n]) and np.array_equal(a["row_ptr"], b["row_ptr"]) and np.array_equal(a["src"], b["src"]))


# ---- what the bodies share ------------------------------------------------------------------------------------------------------------
def _ints(graph):
    from tests import inbound_similarity_ref as sref
    return sref.id_ints(graph[0])


def _few_keys(rng, n):
    """a key per sid from four values, u64::MAX (not listed) among them: ties around every cut"""
    key = rng.integers(0, 3, n).astype(np.uint64)
    key[rng.random(n) < 0.25] = np.uint64(U64_MAX)
    return key


def _queries(rng, graph, picks, count):
    """(sids with -1 for an unknown id, ids): random nodes, the picks, duplicates and unknown ids"""
    n = len(graph[0])
    qsids = np.concatenate((rng.integers(0, n, count), np.asarray(picks, dtype=np.int64), [-1, -1])).astype(np.int64)
    qsids = np.concatenate((qsids, qsids[:3]))  # duplicates
    qsids = qsids[rng.permutation(len(qsids))]
    ids = np.zeros(len(qsids), dtype=_lib.U128)
    known = qsids >= 0
    ids[known] = graph[0][qsids[known]]
    ids["hi"][~known] = np.uint64(1 << 36)  # 2^100 and up
    ids["lo"][~known] = np.arange(int((~known).sum()), dtype=np.uint64)
    return qsids, ids


def _key_list(ints, key):
    return [(v, int(k)) for v, k in zip(ints, key.tolist()) if k != U64_MAX]


def draw_entries(rng, ints, k):
    """k liked or disliked hosts of hb_inbound_similarity: random nodes; where there is room, an id that is no node and a duplicate"""
    n = len(ints)
    e = [ints[int(x)] for x in rng.integers(0, n, k)]
    if k > 2:
        e[int(rng.integers(0, k))] = UNKNOWN + int(rng.integers(0, 3))  # no node of the graph
        e[int(rng.integers(0, k))] = e[0]  # a duplicate
    return e


def draw_shared_pool(rng, ints, picks):
    """what the requests of one hb_score_hosts call share: twelve random nodes, two ids that are no node, the picks"""
    return [ints[int(x)] for x in rng.integers(0, len(ints), 12)] + [UNKNOWN + 1, UNKNOWN + 2] + [ints[s] for s in picks]


def draw_from_pool(rng, ints, pool, k):
    """k hosts of a request: every third from the shared pool, the others any node"""
    return [pool[int(rng.integers(0, len(pool)))] if rng.integers(0, 3) == 0 else ints[int(rng.integers(0, len(ints)))] for _ in range(k)]


def draw_liked(rng, ints, count, picks):
    """the liked hosts of hb_similar_hosts: `count` random nodes, the picks, an id that is no node and a duplicate"""
    liked = [ints[int(x)] for x in rng.integers(0, len(ints), count)] + [ints[s] for s in picks]
    return liked + [UNKNOWN + 3, liked[0]]


# ---- the bodies -----------------------------------------------------------------------------------------------------------------------
def distances_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_distances: random source set x direction x max_dist x forced step, against the host restatement"""
    from tests import distance_ref as dref
    ids, row_ptr, src = graph
    n, passes = len(ids), 0
    for r in range(4):
        srcs = sorted(set([int(x) for x in rng.integers(0, n, int(rng.integers(1, 5)))] + (picks.all() if r < 2 else [])))
        rev = bool(rng.integers(0, 2)) if r >= 2 else bool(r)  # the picks once along and once against the edges
        md = [None, 0, 1, 7, 15, 200][int(rng.integers(0, 6))]
        mode = [None, "top_down", "bottom_up"][int(rng.integers(0, 3))]
        if tally is not None:
            tally.count("distances", what["kind"])
        if ctx is None:
            continue
        want = dref.dijkstra(n, row_ptr, src, srcs, reversed=rev, max_dist=md)
        gids, gdist, st = ctx.distances(ids[np.asarray(srcs, dtype=np.int64)], reversed=rev, max_dist=md, mode=mode)
        keep = want != dref.UNREACHED
        run = dict(what, sources=srcs, reversed=rev, max_dist=md, mode=mode)
        assert np.array_equal(gids, ids[keep]) and np.array_equal(gdist, want[keep]), ("distance list", run)
        assert np.array_equal(ctx.distance_all(), want) and st["reached"] == int(keep.sum()) == sum(st["frontier"]), ("distance array / counters", run)
        passes += st["levels"]
    return passes


def betweenness_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_betweenness: random source set x forced mode, against the host restatement under the rule of tests/test_betweenness.py"""
    from tests import betweenness_ref as bref
    ids, row_ptr, src = graph
    n, passes = len(ids), 0
    for r in range(3):
        srcs = sorted(set([int(x) for x in rng.integers(0, n, int(rng.integers(1, 20)))] + (picks.all() if r == 0 else [])))
        mode = [None, "dense", "sparse"][int(rng.integers(0, 3))]
        raw = bool(rng.integers(0, 2))
        run = dict(what, sources=srcs, mode=mode, raw=raw)
        res = bref.literal(n, row_ptr, src, srcs)
        limit = res.max_dist > 254 or max(max(s) for s in res.sigma) >= 2 ** 64 - 1  # (HB_ERR_LIMIT cases: tests/test_betweenness.py)
        if tally is not None:
            tally.count("betweenness", what["kind"], not limit)
        if limit or ctx is None:
            continue
        tol = bref.rtol(n, row_ptr, src, res)
        gids, gvals, st = ctx.betweenness(ids[np.asarray(srcs, dtype=np.int64)], raw=raw, mode=mode)
        want = res.values(raw)[res.reached]
        assert np.array_equal(gids, ids[res.reached]) and st["max_dist"] == res.max_dist and st["results"] == len(gids), ("result set / max_dist", run)
        assert np.array_equal(np.isnan(gvals), np.isnan(want)) and np.array_equal(np.isinf(gvals), np.isinf(want)), ("NaN / inf pattern", run)
        fin = np.isfinite(want)
        assert not gvals[fin & (want == 0.0)].view(np.uint64).any(), ("+0.0 values", run)
        assert (np.abs(gvals[fin] - want[fin]) <= tol * np.abs(want[fin])).all(), ("values", run, tol)
        dist, sigma, delta = ctx.debug_betweenness_batch()
        first = (len(srcs) - 1) // 8 * 8
        for lane, k in enumerate(range(first, len(srcs))):
            assert np.array_equal(dist[:, lane], np.where(res.dist[k] < 0, 255, res.dist[k]).astype(np.uint8)), ("dist of source %d" % k, run)
            assert [int(x) for x in sigma[:, lane]] == res.sigma[k], ("sigma of source %d" % k, run)
            assert (np.abs(delta[:, lane] - res.delta[k]) <= tol * np.abs(res.delta[k])).all(), ("delta of source %d" % k, run)
        passes += st["levels_forward"] + st["levels_backward"]
    return passes


def similarity_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_inbound_similarity: random entry lists (duplicates, unknown ids, an entry equal to a scored node - every known entry is one) x
    a limit (0 = whole in-lists, and values that cut) x a key set (few distinct keys: ties are common) x the three mode settings, against
    the host restatement, bit for bit.  Tallied as `similarity` at limit 0 and as `similarity_cut` otherwise."""
    from tests import inbound_similarity_ref as sref
    from tests import limited_similarity_ref as lref
    ids = graph[0]
    ints = _ints(graph)
    n, passes = len(ints), 0

    for r in range(3):
        liked, disliked = draw_entries(rng, ints, int(rng.integers(0, 40))), draw_entries(rng, ints, int(rng.integers(0, 20)))
        if r < 2:  # the picks once under the whole in-lists and once under a cut
            liked += [ints[s] for s in picks.hubs]
            disliked += [ints[s] for s in picks.members[:2]]
        normalized = bool(rng.integers(0, 2))
        self_score = [None, 0.25, 3.0][int(rng.integers(0, 3))]
        limit = 0 if r == 0 else int(rng.choice(LIMITS)) if r == 1 else int(rng.choice((0,) + LIMITS))
        keys = [(v, int(rng.integers(0, 4))) for v in ints if rng.integers(0, 2)] if rng.integers(0, 2) else []
        k = int(rng.integers(1, n + 3))
        op = "similarity" if limit == 0 else "similarity_cut"
        empty = not liked and not disliked
        if tally is not None:
            tally.count(op, what["kind"], not empty)
        if empty or ctx is None:
            continue
        if keys:
            ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
        else:
            ctx.links_set_keys()
        bv = lref.bitvecs(*graph, keys, limit)
        want = sref.literal(*graph, liked, disliked, normalized, 1.0 if self_score is None else self_score, bv=bv)
        last = (liked + disliked)[(len(liked) + len(disliked) - 1) // 16 * 16:]
        for mode in (None, "dense", "sparse"):
            run = dict(what, liked=liked, disliked=disliked, normalized=normalized, self_score=self_score, mode=mode, limit=limit, keys=keys)
            st = ctx.inbound_similarity(ids_from_ints(liked), ids_from_ints(disliked), normalized=normalized, self_score=self_score, mode=mode,
                                        limit=limit)
            assert ctx.similarity_all().tobytes() == want.tobytes(), ("scores", run)
            counts, bloom, length = ctx.debug_similarity_batch()
            assert np.array_equal(counts[:, :len(last)], sref.counts(bv, ids, last)), ("counts of the last batch", run)
            assert [int(x) for x in bloom] == [bv[v].fold() for v in ints], ("bloom", run)
            assert [int(x) for x in length] == [len(bv[v].ranks) for v in ints], ("len", run)
            passes += sum(st["levels_mode"])
        asked = liked[:3] + [UNKNOWN, 5]
        assert ctx.similarity_lookup(ids_from_ints(asked)).tobytes() == \
            sref.lookup(bv, liked, disliked, normalized, 1.0 if self_score is None else self_score, asked).tobytes(), ("lookup", what)
        tids, tvals = ctx.similarity_top(k)
        order = sref.top_order(ids, want, k)
        assert sref.id_ints(tids) == [v for _, v in order] and tvals.tolist() == [x for x, _ in order], ("top", what, k)
    return passes


def score_hosts_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_score_hosts: a key set (few distinct keys) x a limit x 1 to 5 requests that share hosts, with unknown ids and duplicates on every
    side x the piece size and the debug flags of the list selects, against the route it replaces on the same context and against the
    literal restatement: every score bit for bit, every counter."""
    from tests import score_hosts_ref as ref
    ints = _ints(graph)
    n, passes = len(ints), 0
    pool = draw_shared_pool(rng, ints, picks.all())

    def draw(k):
        return draw_from_pool(rng, ints, pool, k)

    for r in range(2):
        limit = int(rng.choice(LIMITS))
        keys = [(v, int(rng.integers(0, 4))) for v in ints if rng.integers(0, 2)] if rng.integers(0, 2) else []
        requests = [dict(liked=draw(int(rng.integers(0, 40))), disliked=draw(int(rng.integers(0, 20))), nodes=draw(int(rng.integers(0, 30))),
                         normalized=bool(rng.integers(0, 2)), self_score=[None, 0.25, 3.0][int(rng.integers(0, 3))]) for _ in range(int(rng.integers(1, 6)))]
        if r == 0:  # the hubs of the plan's trees are scored, against liked hosts inside those trees
            requests[0]["nodes"] += [ints[s] for s in picks.hubs]
            requests[0]["liked"] += [ints[s] for s in picks.all()]
        sflags = int(rng.choice([0, _lib.HB_LINKS_SPREAD_ORDS, _lib.HB_LINKS_NO_SHORTCUT]))
        small = bool(rng.integers(0, 2))
        slots = int(rng.choice(SLOTS))
        if tally is not None:
            tally.count("score_hosts", what["kind"])
        if ctx is None:
            continue
        if keys:
            ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
        else:
            ctx.links_set_keys()
        want, wst = ref.literal(ref.tables(*graph, keys, limit), requests)
        run = dict(what, limit=limit, keys=keys, requests=requests, sflags=sflags, small_pieces=small, slots=slots)
        st = ctx.score_hosts([dict(q, liked=ids_from_ints(q["liked"]), disliked=ids_from_ints(q["disliked"]), nodes=ids_from_ints(q["nodes"])) for q in requests],
                             limit=limit, flags=sflags, small_pieces=small, slots_per_batch=slots)
        got = ctx.score_copy()
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], ("scores against the restatement", run)
        assert {k: st[k] for k in wst} == wst, ("stats", run, st)
        for q, g in zip(requests, got):
            if q["liked"] or q["disliked"]:
                ctx.inbound_similarity(ids_from_ints(q["liked"]), ids_from_ints(q["disliked"]), normalized=q["normalized"], self_score=q["self_score"], limit=limit)
                assert ctx.similarity_lookup(ids_from_ints(q["nodes"])).tobytes() == g.tobytes(), ("scores against the lookup route", run)
        passes += st["pieces"]
    return passes


def nearest_seed_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_nearest_seed: random original / key lists (duplicates, unknown ids, 0.0, few distinct keys so that ties are common, u64::MAX) x
    rounds x discount, against the host restatement: the seed of every node, every value bit for bit, every counter, the top order."""
    from tests import inbound_similarity_ref as sref
    from tests import nearest_seed_ref as nref
    ints = _ints(graph)
    n, passes = len(ints), 0
    for r in range(3):
        share = [0.02, 0.1, 0.5][int(rng.integers(0, 3))]
        orig = [(ints[int(x)], [0.0, float(rng.random()), float(rng.integers(0, 4)) / 4.0][int(rng.integers(0, 3))])
                for x in rng.integers(0, n, max(1, int(n * share)))]
        orig += [(UNKNOWN + 1, 0.5), orig[0]]
        spread = int(rng.choice([1, 3, 1 << 62]))
        keys = [(v, int(rng.integers(0, spread)) if rng.random() < 0.9 else nref.U64_MAX) for v in ints if rng.random() < 0.8]
        if r == 0:  # the members of the plan's trees carry the smallest keys of all, the last of them the very smallest
            inside = {ints[s] for s in picks.members}
            keys = [(v, k + 2 if k < nref.U64_MAX - 2 else k) for v, k in keys if v not in inside]
            keys += [(ints[s], 1) for s in sorted(set(picks.members[:-1]) - set(picks.members[-1:]))] + [(ints[s], 0) for s in picks.members[-1:]]
        keys += [(UNKNOWN + 2, 0)] + keys[:2]
        discount = [0.5, 0.3, 0.0, 1.0][int(rng.integers(0, 4))]
        rounds = int(rng.choice([0, 1, 2, 5, 255]))
        k = int(rng.integers(1, n + 3))
        if tally is not None:
            tally.count("nearest_seed", what["kind"])
        if ctx is None:
            continue
        run = dict(what, discount=discount, rounds=rounds, orig=len(orig), keys=len(keys), spread=spread)
        seeds, vals, want = nref.literal(*graph, orig, keys, discount, rounds)
        st = ctx.nearest_seed(ids_from_ints([v for v, _ in orig]), np.array([x for _, x in orig]), ids_from_ints([v for v, _ in keys]),
                              np.array([k for _, k in keys], dtype=np.uint64), discount_factor=discount, rounds=rounds)
        got_seed, got_has = ctx.nearest_seed_seeds()
        assert {v: s for v, s, h in zip(ints, sref.id_ints(got_seed), got_has.tolist()) if h} == seeds, ("seeds", run)
        want_all = np.array([vals.get(v, -1.0) for v in ints], dtype=np.float64)
        assert ctx.nearest_seed_all().tobytes() == want_all.tobytes(), ("values", run)
        cids, cvals = ctx.nearest_seed_copy()
        assert sref.id_ints(cids) == [v for v in ints if v in vals] and cvals.tobytes() == want_all[want_all >= 0.0].tobytes(), ("copy", run)
        assert {k: st[k] for k in nref.STAT_KEYS} == want, ("stats", run, {k: st[k] for k in nref.STAT_KEYS}, want)
        tids, tvals = ctx.nearest_seed_top(k)
        order = nref.top_order(vals, k)
        assert sref.id_ints(tids) == [v for v, _ in order] and tvals.tolist() == [x for _, x in order], ("top", run, k)
        passes += st["rounds_run"]
    return passes


def backlinks_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_backlinks: a key per node from four values, u64::MAX among them x queries with unknown ids and duplicates, the hubs of the
    plan's trees among them x the limits x the batch size, as tests/test_links.py compares: offsets, ids, keys, degrees, counters."""
    n = len(graph[0])
    for r in range(2):
        key = _few_keys(rng, n)
        draws = [(int(rng.choice(LIMITS)), int(rng.choice(SLOTS)), _queries(rng, graph, picks.hubs, min(n, 30))) for _ in range(3)]
        if tally is not None:
            for _ in draws:
                tally.count("backlinks", what["kind"])
        if ctx is None:
            continue
        from tests import test_links as tl
        tl._set_keys(ctx, graph, key)
        for limit, slots, (qsids, qids) in draws:
            tl._run(ctx, graph, key, qsids, limit, slots=slots, query_ids=qids, what=str(what))
    return 6 if ctx is not None else 0


def forwardlinks_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_forwardlinks: the same draws, the members of the plan's trees among the queries (each finds its hub from inside the tree), as
    tests/test_forwardlinks.py compares."""
    n = len(graph[0])
    for r in range(2):
        key = _few_keys(rng, n)
        draws = [(int(rng.choice(LIMITS)), int(rng.choice(SLOTS)), _queries(rng, graph, picks.all(), min(n, 30))) for _ in range(3)]
        if tally is not None:
            for _ in draws:
                tally.count("forwardlinks", what["kind"])
        if ctx is None:
            continue
        from tests import test_forwardlinks as tf
        from tests import test_links as tl
        fgraph = tf._forward(graph)
        tl._set_keys(ctx, graph, key)
        for limit, slots, (qsids, qids) in draws:
            tf._run(ctx, fgraph, key, qsids, limit, slots=slots, query_ids=qids, what=str(what))
    return 6 if ctx is not None else 0


def similar_hosts_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_similar_hosts: liked hosts with duplicates and unknown ids, the hubs of the plan's trees among them (their in-lists are B) x
    k x a key set from four values, as tests/test_similar_hosts.py compares: candidates, list, every score bit, counters."""
    ints = _ints(graph)
    n = len(ints)
    for r in range(3):
        key = _few_keys(rng, n)
        keys = _key_list(ints, key) if r else []
        liked = draw_liked(rng, ints, int(rng.integers(1, 9)), picks.hubs if r < 2 else picks.members[:3])
        k = int(rng.choice(LIMITS))
        if tally is not None:
            tally.count("similar_hosts", what["kind"])
        if ctx is None:
            continue
        from tests import test_similar_hosts as ts
        ts._set(ctx, keys)
        ts._check(ctx, graph, keys, liked, k)
    return 3 if ctx is not None else 0


def sampled_case(ctx, graph, rng, what, picks=Picks(), tally=None):
    """hb_sampled_harmonic: explicit sources (distinct and known, as the entry demands; the picks among them) and the seeded sampler x
    max_dist, as tests/test_sampled_harmonic.py compares: the histogram, the values bit for bit."""
    n, passes = len(graph[0]), 0
    for r in range(3):
        srcs = sorted(set([int(x) for x in rng.integers(0, n, int(rng.integers(1, 30)))] + picks.all())) if r < 2 else None
        md = int(rng.choice([1, 7, 15]))
        seed, samples = int(rng.integers(0, 1 << 30)), int(rng.choice([0, 3, 40])) if srcs is None else 0
        if tally is not None:
            tally.count("sampled", what["kind"])
        if ctx is None:
            continue
        from tests import test_sampled_harmonic as th
        st, _ = th._check(ctx, sources_sids=srcs, max_dist=md, seed=seed, samples=samples)
        passes += st["levels"]
    return passes


BODIES = {"sampled": sampled_case, "distances": distances_case, "betweenness": betweenness_case, "similarity": similarity_case,
          "nearest_seed": nearest_seed_case, "backlinks": backlinks_case, "forwardlinks": forwardlinks_case,
          "similar_hosts": similar_hosts_case, "score_hosts": score_hosts_case}
OPERATORS = ("sampled", "distances", "betweenness", "similarity", "similarity_cut", "nearest_seed", "backlinks", "forwardlinks",
             "similar_hosts", "score_hosts")  # what a Tally counts: hb_inbound_similarity with limit = 0 and with a cutting limit apart


def body_rng(seed, case, name):
    """every body of a case draws from a stream of its own: one body more or less moves no other"""
    return np.random.default_rng([int(seed), int(case), sorted(BODIES).index(name)])


def run_bodies(ctx, graph, seed, case, what, picks=Picks(), tally=None, names=None):
    passes = 0
    for name in names or BODIES:
        passes += BODIES[name](ctx, graph, body_rng(seed, case, name), dict(what, body=name), picks, tally)
    return passes
