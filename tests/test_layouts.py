"""Every plan-reading operator under plan layouts the operator suites never load: band cuts inside a hub's list, chunk rows of one hub
that are not neighbours, one-chunk trees, split rows no longer than `chunk`, trees of three and more levels, and no chunk row at all.

A seeded list of cases; each is one context - a graph of graphs.random_graph with self links, a chunk, the planner's cut and split
knobs tune[3..5] and two layout flags - on which all nine bodies of tests/operator_cases.py run, each against the CPU restatement of
its operator under the comparison rule of that operator's own suite.  The sids the bodies are handed besides their random draws are
read from the plan: for every layout condition the context shows, the node row on top of such a tree and sources inside it.

The conditions are asserted, not assumed (test_layout_conditions), and so is the share of calls that really compare (test_cap).  Both
count over the whole list from the host planner and the restatements alone; test_operators_under_layout asserts that the plan in HBM
is that plan and that its calls were the counted ones.  One crafted case, a small flipped fan under two banded layouts, has closed
answers.  HB_LAYOUT_CASES = N runs the first N cases only (tests/test_layouts_simt.py).

A second list (LIVE_CASES, its own seed) draws from the same recipe with HB_FLAG_LIVE_FIRST on every context and graph kinds that have
hosts without an in-link: the live-first device order of DESIGN.md section 32, in which every graph of 2^20 hosts and more is planned.
Two more conditions are read from such a plan - a lowest-level chunk row whose sources are all dead, and one that mixes live and dead
sources - and the hub, a live member and a dead member of such a tree go to the bodies: a dead host is a forward-link query, a walk
source and a scored host there.  HB_LIVE_LAYOUT_CASES = N runs the first N of them only."""
import os

import numpy as np
import pytest

from stract_amd import _lib
from tests import fans
from tests import graphs
from tests import operator_cases as oc

pytestmark = pytest.mark.gpu

SEED = 977
RANDOM_CASES = 40
STARS_EVERY = 5  # after every five random cases one `stars` graph at chunk = 4 (cases 2, 8, 14, ...): the trees of depth >= 3, scarce in the random draws
KINDS = ("uniform", "stars", "chains", "dense_core", "bipartite")
LIVE_SEED = 4
LIVE_COUNT = 16
LIVE_KINDS = ("stars", "bipartite", "uniform", "dead_fringe")  # the kinds with hosts that have no in-link


class Case:
    def __init__(self, index, kind, tuples, chunk, tune, flags, seed=SEED):
        self.index, self.kind, self.tuples, self.chunk, self.tune, self.flags, self.seed = index, kind, tuples, chunk, tune, flags, seed
        self.name = "%02d-%s-chunk%d-tune%d.%d.%d-flags%x-seed%d" % (index, kind, chunk, tune[3], tune[4], tune[5], flags, seed)
        self._dry = None

    def what(self):
        return dict(case=self.index, kind=self.kind, chunk=self.chunk, tune=self.tune, flags=self.flags, seed=self.seed)

    def dry(self):
        """(graph, host plan, conditions, picks, tally): what the case is before any context exists"""
        if self._dry is None:
            graph = graphs.dense_from_tuples(self.tuples)
            plan = _lib.host_plan(graph[1], graph[2], self.flags & (oc.PLAN_FLAGS | _lib.HB_FLAG_LIVE_FIRST), self.chunk, self.tune)
            cond = oc.layout_conditions(plan, graph[1], self.chunk, plan["n_live"] if plan["live_first"] else None)
            picks = oc.picks_of(cond)
            tally = oc.Tally()
            oc.run_bodies(None, graph, self.seed, self.index, self.what(), picks, tally)
            self._dry = (graph, plan, cond, picks, tally)
        return self._dry


def _cases():
    rng = np.random.default_rng(SEED)
    out = []
    while len(out) < RANDOM_CASES + RANDOM_CASES // STARS_EVERY:
        stars = len(out) % (STARS_EVERY + 1) == 2
        kind, tuples = oc.draw_graph(rng, "stars" if stars else None)
        chunk, tune, flags = oc.draw_layout(rng, 4 if stars else None)
        out.append(Case(len(out), kind, tuples, chunk, tune, flags))
    return out


def _live_cases():
    """the recipe of _cases() with HB_FLAG_LIVE_FIRST on every context, the kinds of LIVE_KINDS in turn; contexts 0, 5, 10 and 15 - one of every kind -
    at chunk = 4"""
    rng = np.random.default_rng(LIVE_SEED)
    out = []
    while len(out) < LIVE_COUNT:
        kind, tuples = oc.draw_graph(rng, LIVE_KINDS[len(out) % len(LIVE_KINDS)])
        chunk, tune, flags = oc.draw_layout(rng, 4 if len(out) % 4 == len(out) // 4 else None)
        out.append(Case(len(out), kind, tuples, chunk, tune, flags | _lib.HB_FLAG_LIVE_FIRST, LIVE_SEED))
    return out


CASES = _cases()
LIVE_CASES = _live_cases()
RUN = CASES[:int(os.environ.get("HB_LAYOUT_CASES", len(CASES)))] + LIVE_CASES[:int(os.environ.get("HB_LIVE_LAYOUT_CASES", len(LIVE_CASES)))]
LIVE = {}  # (seed, case index) -> the tally of its run on the context


@pytest.mark.parametrize("case", RUN, ids=[c.name for c in RUN])
def test_operators_under_layout(gpu_ctx_factory, case):
    graph, plan, cond, picks, _ = case.dry()
    with oc.load(gpu_ctx_factory, case.tuples, case.chunk, case.tune, case.flags) as ctx:
        got = ctx.graph()
        assert all(np.array_equal(a, b) for a, b in zip(got, graph)), case.name
        assert oc.plan_equal(ctx.plan(), plan, len(graph[0])), case.name  # the conditions below are those of the plan in HBM
        assert ctx.plan_live() == (plan["live_first"], plan["n_live"], plan["n_live_pad"]), case.name
        tally = oc.Tally()
        oc.run_bodies(ctx, got, case.seed, case.index, case.what(), picks, tally)
    LIVE[case.seed, case.index] = tally


def test_layout_conditions():
    """Every condition of operator_cases.layout_conditions in at least three contexts of the list, and (a) to (e) in at least one whose
    bodies are handed the hub of such a tree and sources inside it.  Counts of the committed seed, out of 48 contexts: (a) 10, (b) 26,
    (c) 17, (d) 20, (e) 7, (f) 16; every context with one of (a) to (e) hands such picks to its bodies (picks_of).

    The live-first list: the order is in use in every context that does not keep the id order, every graph has hosts with and without an
    in-link, and (g) and (h) each show in at least three contexts whose bodies are handed the hub, and for (g) two dead members, for (h) a
    live and a dead member of such a chunk.  Counts of its seed, out of 16 contexts: (a) 7, (b) 11, (c) 7, (d) 8, (e) 3, (f) 3, (g) 10,
    (h) 8, all of (g) and (h) with their picks inside; 11 contexts hand a dead host to their bodies."""
    count = dict.fromkeys(oc.CONDITIONS, 0)
    targeted = dict.fromkeys(oc.CONDITIONS, 0)
    for case in CASES:
        graph, plan, cond, picks, _ = case.dry()
        for c, (hub, members) in cond.items():
            count[c] += 1
            if hub is not None and hub in picks.hubs and set(members) <= set(picks.members) and members:
                targeted[c] += 1
    print("layout conditions over %d contexts: %s; with picks inside: %s" % (len(CASES), count, targeted))
    assert all(count[c] >= 3 for c in oc.CONDITIONS), count
    assert all(targeted[c] >= 1 for c in "abcde"), targeted
    count = dict.fromkeys(oc.CONDITIONS + oc.LIVE_CONDITIONS, 0)
    targeted = dict.fromkeys(oc.LIVE_CONDITIONS, 0)
    dead_picks = 0
    for case in LIVE_CASES:
        graph, plan, cond, picks, _ = case.dry()
        # the order is in use wherever the context does not keep the id order, and every such graph has hosts of both kinds
        assert plan["live_first"] == (not case.flags & _lib.HB_FLAG_NO_REORDER) and 0 < plan["n_live"] < len(graph[0]), case.name
        indeg = np.diff(graph[1].astype(np.int64))
        for c, (hub, members) in cond.items():
            count[c] += 1
            if c in targeted and hub in picks.hubs and set(members) <= set(picks.members):
                assert indeg[hub] > 0 and indeg[members[-1]] == 0 and (c == "g") == (indeg[members[0]] == 0), (case.name, c)
                targeted[c] += 1
        dead_picks += any(indeg[s] == 0 for s in picks.all())
    print("live-first list, layout conditions over %d contexts: %s; (g) / (h) with picks inside: %s; contexts that hand a dead host to the bodies: %d"
          % (len(LIVE_CASES), count, targeted, dead_picks))
    assert all(count[c] >= 3 and targeted[c] >= 3 for c in oc.LIVE_CONDITIONS), (count, targeted)


def test_cap():
    """Over the whole list every operator is compared in at least 90 % of its calls and at least once per graph kind.  A betweenness call
    is not compared when the restatement itself hits HB_ERR_LIMIT, a similarity round not when both lists are empty.  Counts of the
    committed seed (compared / calls): sampled 144 / 144, distances 192 / 192, betweenness 144 / 144, similarity 54 / 54,
    similarity_cut 90 / 90, nearest_seed 144 / 144, backlinks 288 / 288, forwardlinks 288 / 288, similar_hosts 144 / 144,
    score_hosts 96 / 96: no call of the committed list is left out.  The live-first list under the same rule and its own four kinds:
    sampled 48 / 48, distances 64 / 64, betweenness 48 / 48, similarity 21 / 21, similarity_cut 27 / 27, nearest_seed 48 / 48,
    backlinks 96 / 96, forwardlinks 96 / 96, similar_hosts 48 / 48, score_hosts 32 / 32."""
    for cases, kinds in ((CASES, KINDS), (LIVE_CASES, LIVE_KINDS)):
        total = oc.Tally()
        for case in cases:
            dry = case.dry()[4]
            total.add(dry)
            if (case.seed, case.index) in LIVE:  # the calls made on the context are the counted ones
                assert LIVE[case.seed, case.index].as_dict() == dry.as_dict(), case.name
        print("compared / calls over %d contexts: %s" % (len(cases), {op: (total.compared.get(op, 0), total.calls.get(op, 0)) for op in oc.OPERATORS}))
        for op in oc.OPERATORS:
            assert total.calls.get(op, 0) > 0 and total.compared[op] * 10 >= total.calls[op] * 9, (op, total.as_dict())
            for kind in kinds:
                assert total.compared.get((op, kind), 0) >= 1, (op, kind, total.as_dict())


# ---- the crafted case: a small flipped fan under two banded layouts, exact answers ------------------------------------------------------
FAN_KS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257)
CUT_KS = tuple(K for K in FAN_KS if K >= 17)
FAN_LIMITS = (1, 4, 5, 64, 65, 256)
# both have 16- or 32-counter bands; under the second a list of more than 8 entries is split although it fits one 64-entry chunk
FAN_LAYOUTS = {"chunk16-band16": dict(chunk=16, tune=(0, 0, 0, 4, 1, 0, 0)), "chunk64-band32-split8": dict(chunk=64, tune=(0, 0, 0, 5, 3, 8, 0))}
_FAN = []


def _fan():
    if not _FAN:
        _FAN.append(fans.Fan(Ks=FAN_KS))
    return _FAN[0]


@pytest.fixture(scope="module")
def fan_loaded(gpu_ctx_factory):
    cache = {}

    def get(name):
        if name not in cache:
            fan = _fan()
            ctx = oc.load(gpu_ctx_factory, fan.tuples(flipped=True), FAN_LAYOUTS[name]["chunk"], FAN_LAYOUTS[name]["tune"], _lib.HB_FLAG_ALL_RELS)
            graph = ctx.graph()
            assert np.array_equal(graph[0]["lo"], np.arange(1, fan.n + 1, dtype=np.uint64)) and not graph[0]["hi"].any()  # sid == node index
            plan = ctx.plan()
            order = plan["order"].astype(np.int64)
            row_of = np.full(fan.n, -1, dtype=np.int64)
            row_of[order[order != oc.NONE]] = np.flatnonzero(order != oc.NONE)
            cuts = {}
            for K in CUT_KS:
                chunks, _ = oc.tree(plan, int(row_of[fan.hub_of(K)]))
                lists = [[int(order[r]) for r in ch] for _, ch in chunks]
                assert sorted(v for ch in lists for v in ch) == fan.leaves(K).tolist(), K
                # THE layout condition of this case: the hub's list is cut at a band boundary inside it - a lowest-level chunk that is
                # not the last one and is shorter than `chunk`.  The first such chunk and the one behind it:
                short = [i for i, ch in enumerate(lists[:-1]) if len(ch) < FAN_LAYOUTS[name]["chunk"]]
                assert short, (name, K, [len(ch) for ch in lists])
                cuts[K] = (lists[short[0]], lists[short[0] + 1])
            cache[name] = (fan, ctx, graph, cuts)
        return cache[name]

    yield get
    for _, ctx, _, _ in cache.values():
        ctx.close()


POSITIONS = {"first of the short chunk": lambda short, after: short[0], "last of the short chunk": lambda short, after: short[-1],
             "first of the chunk behind it": lambda short, after: after[0]}


@pytest.mark.parametrize("layout", sorted(FAN_LAYOUTS))
def test_fan_backlinks_across_band_cuts(fan_loaded, layout):
    from tests import test_links as tl
    fan, ctx, graph, cuts = fan_loaded(layout)
    assert np.array_equal(np.diff(graph[1].astype(np.int64))[fan.hub], np.array(fan.Ks))
    for salt in (0, 1):
        key = tl._hash64(salt, fan.n)
        tl._set_keys(ctx, graph, key)
        for limit in FAN_LIMITS:
            _, res = tl._run(ctx, graph, key, fan.hub, limit, what="%s salt %d" % (layout, salt))
            for K, lst in zip(FAN_KS, tl._lists(res)):
                leaves = fan.leaves(K)
                assert lst == (leaves[np.lexsort((leaves, key[leaves]))][:limit] + 1).tolist(), (layout, K, limit)


@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("layout", sorted(FAN_LAYOUTS))
def test_fan_nearest_seed_minimum_at_a_band_cut(fan_loaded, layout, where):
    from tests import test_links as tl
    from tests import test_nearest_seed as tn
    fan, ctx, graph, cuts = fan_loaded(layout)
    placed = {K: POSITIONS[where](*cuts[K]) for K in CUT_KS}
    key = tl._hash64(13, fan.n) | np.uint64(1 << 40)  # far above the placed keys
    for i, K in enumerate(CUT_KS):
        key[placed[K]] = i  # the minimum of h_K's list
    keys = [(v + 1, int(k)) for v, k in enumerate(key.tolist())]
    seeds, _, _ = tn._check(ctx, graph, orig=[(int(fan.leaves(257)[0]) + 1, 1.0)], keys=keys, rounds=1, what="%s, %s" % (layout, where))
    for K in CUT_KS:
        assert seeds[fan.hub_of(K) + 1] == placed[K] + 1, (layout, where, K)


@pytest.mark.parametrize("layout", sorted(FAN_LAYOUTS))
def test_fan_forwardlinks_from_the_band_cuts(fan_loaded, layout):
    from tests import test_forwardlinks as tf
    from tests import test_links as tl
    fan, ctx, graph, cuts = fan_loaded(layout)
    fgraph = tf._forward(graph)
    key = tl._hash64(8, fan.n)
    tl._set_keys(ctx, graph, key)
    queries, hubs = [], []
    for K in CUT_KS:
        for where in sorted(POSITIONS):
            queries.append(POSITIONS[where](*cuts[K]))
            hubs.append(fan.hub_of(K))
    for limit in (1, 3):
        _, res = tf._run(ctx, fgraph, key, queries, limit, what=layout)
        assert tl._lists(res) == [[h + 1] for h in hubs], layout  # a leaf links to its hub alone, and finds it from inside the tree
