"""The live-first device order on the GPU (HB_FLAG_LIVE_FIRST): hosts without an in-edge ("dead") lie behind the
others, and from pass 1 on the dense passes do not gather them and the node-row launches end at the last live row.  Nothing that is
computed may move: the device planner equals the host planner entry for entry, every pass leaves the oracle's registers, Kahan words,
sizes and changed count in every pass mode, the per-pass statistics and the result bits equal those of the plain order, contexts the
argument does not cover plan as before, and the plan-reading operators give their restatements' answers on such a plan.

The crafted graphs (`_fan`) hold what the shortened launches and the gather limit can get wrong: a node row fed only by dead sources, a
hub row (chunk = 4) with a chunk of dead sources only and one that mixes live and dead ones, n_live of 63, 64, 65 and 128 (the tile
boundary of the shortened launch), a graph without dead hosts and one whose sources are all dead.

The tile family (`TILES`) walks n_live and n_dead over both sides of a 64-row tile: dead rows inside the last live tile (n_live_pad =
n_pad: no row is skipped and no changed word cleared), exactly one tile of dead rows behind it, a live part that ends on a tile
boundary - read back from the plan in HBM - in the default, the bitmap and the sweep mode.  One context takes its hosts from an
explicit node list that names hosts with neither an in- nor an out-link."""
import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib, synth
from tests import graphs
from tests import operator_cases as oc

pytestmark = pytest.mark.gpu

ON = _lib.HB_FLAG_LIVE_FIRST
OFF = _lib.HB_FLAG_NO_LIVE_FIRST


def _fan(n_live, n_dead=70):
    """n_live hosts with an in-edge - a ring with chords 1 .. n_live - 2, X and H - and n_dead hosts without one (ids above 1000).
    X is fed by three dead hosts only; H by six ring nodes and nine dead hosts (at chunk = 4: a chunk of live sources, one of two live
    and two dead ones, two of dead ones); ring node 1 by its ring neighbours, X, H and 20 dead hosts; every dead host links to a ring
    node, so each has an out-degree and a place in the order."""
    L = n_live - 2
    ring = list(range(1, L + 1))
    X, H = L + 1, L + 2
    dead = [1001 + i for i in range(n_dead)]
    e = set()
    for i, v in enumerate(ring):
        e.add((v, ring[(i + 1) % L]))
        e.add((v, ring[(i * 7 + 3) % L]))
    for v in ring[1:6]:
        e.add((v, 1))                      # live sources of the hub
    for d in dead[:3]:
        e.add((d, X))                      # X: a row fed by dead sources only
    e.add((X, 1))
    for v in ring[10:16]:
        e.add((v, H))
    for d in dead[23:32]:
        e.add((d, H))
    e.add((H, 1))
    for d in dead[3:23]:
        e.add((d, 1))                      # the hub's dead sources: whole chunks of them at chunk = 4
    for i, d in enumerate(dead):
        e.add((d, ring[(5 * i + 2) % L]))
    return sorted((f, t, 0) for f, t in e if f != t)


def _no_dead(n=150):
    return sorted({(v, (v % n) + 1, 0) for v in range(1, n + 1)} | {(v, (v * 11 + 5) % n + 1, 0) for v in range(1, n + 1) if (v * 11 + 5) % n + 1 != v})


def _all_sources_dead(sources=200, sinks=90):
    """sources -> sinks: every source is dead, every sink live and without out-edge; sink 1 is a hub whose whole tree is dead"""
    e = {(1000 + s, 1 + (s * 7) % sinks, 0) for s in range(sources)} | {(1000 + s, 1 + (s * 13 + 1) % sinks, 0) for s in range(sources)}
    return sorted(e | {(1000 + s, 1, 0) for s in range(0, sources, 3)})


def _ring_fringe(n_live, n_dead):
    """the plainer graph of the tile family: a ring of n_live hosts with one chord each, and n_dead hosts (ids above 1000) that link into it"""
    e = {(v, v % n_live + 1) for v in range(1, n_live + 1)} | {(v, (v * 7 + 3) % n_live + 1) for v in range(1, n_live + 1)}
    e |= {(1001 + d, (5 * d + 2) % n_live + 1) for d in range(n_dead)}
    return sorted((f, t, 0) for f, t in e if f != t)


# The tile shapes of the shortened launches (row_hi = n_live_pad) and of the one-time clearing of the dead rows' changed words: n_live and
# n_live + n_dead on either side of a 64-row tile boundary.  _fan where it has the dead hosts its rows need (32), the ring otherwise.
TILE_LIVE, TILE_DEAD = (63, 64, 65, 127, 128, 129), (1, 63, 64, 65)
TILES = {"tile%dx%d" % (nl, nd): (nl, nd) for nl in TILE_LIVE for nd in TILE_DEAD}
TILE_MODES = ("default", "bitmap_always", "sweep_always")


def _tile_shapes(n, n_pad, n_live, n_live_pad):
    """which of the three shapes a layout has: dead rows inside the last live tile (no row is skipped, no word cleared), exactly one
    tile of dead rows behind the last live tile, a live part that ends on a tile boundary"""
    return {"dead_rows_in_the_last_live_tile": n_live < n and n_live_pad == n_pad, "one_dead_tile": n_pad - n_live_pad == 64,
            "n_live_multiple_of_64": n_live % 64 == 0}


def _pad(x):
    return (x + 63) // 64 * 64


# ... as the family was laid out (n_pad = n rounded up to 64 rows on one rank); the test reads the same three from the plan in HBM
TILE_SHAPES = {name: _tile_shapes(nl + nd, _pad(nl + nd), nl, _pad(nl)) for name, (nl, nd) in TILES.items()}
assert TILE_SHAPES["tile63x1"] == dict(dead_rows_in_the_last_live_tile=True, one_dead_tile=False, n_live_multiple_of_64=False)
assert TILE_SHAPES["tile64x64"] == dict(dead_rows_in_the_last_live_tile=False, one_dead_tile=True, n_live_multiple_of_64=True)
assert TILE_SHAPES["tile129x63"] == dict(dead_rows_in_the_last_live_tile=True, one_dead_tile=False, n_live_multiple_of_64=False)
assert TILE_SHAPES["tile127x65"] == dict(dead_rows_in_the_last_live_tile=False, one_dead_tile=True, n_live_multiple_of_64=False)
assert all(sum(s[k] for s in TILE_SHAPES.values()) >= 6 for k in TILE_SHAPES["tile63x1"])


def _tile_tuples(name):
    nl, nd = TILES[name]
    return _fan(nl, nd) if nd >= 32 else _ring_fringe(nl, nd)


GRAPHS = {
    "fan63": lambda: graphs.dense_from_tuples(_fan(63)),
    "fan64": lambda: graphs.dense_from_tuples(_fan(64)),
    "fan65": lambda: graphs.dense_from_tuples(_fan(65)),
    "fan128": lambda: graphs.dense_from_tuples(_fan(128)),
    "no_dead": lambda: graphs.dense_from_tuples(_no_dead()),
    "all_sources_dead": lambda: graphs.dense_from_tuples(_all_sources_dead()),
    "rmat10": lambda: (lambda g: (g.ids.copy(), g.row_ptr.copy(), g.src.copy()))(synth.RmatGraph(10, 6000)),  # (copies: the arrays outlive g)
}
GRAPHS.update({name: (lambda name=name: graphs.dense_from_tuples(_tile_tuples(name))) for name in TILES})
_BUILT = {}


def _graph(name):
    if name not in _BUILT:
        ids, row_ptr, src = GRAPHS[name]()
        _BUILT[name] = (ids, row_ptr, src, np.ascontiguousarray(ids["lo"]))
    return _BUILT[name]


# every graph at chunk = 4 (hub rows become trees); the pass mode forced by the tune thresholds (tune[2] > 100: never dense after pass 0,
# tune[6] = 1: sweep whenever a bitmap pass would run, tune[6] huge: never sweep)
MODES = {
    "default": dict(),
    "dense_only": dict(flags=_lib.HB_FLAG_NO_FRONTIER),
    "bitmap_always": dict(tune=(0, 0, 101, 0, 0, 0, 1000000)),
    "sweep_always": dict(tune=(0, 0, 101, 0, 0, 0, 1)),
    "no_init_pass": dict(flags=_lib.HB_FLAG_NO_INIT_PASS),
    "no_init_pass_bitmap": dict(flags=_lib.HB_FLAG_NO_INIT_PASS, tune=(0, 0, 101, 0, 0, 0, 1000000)),
    "unroll4_node_rows": dict(tune=(0, 4)),
}
EXPECT_MODES = {"dense_only": {0}, "bitmap_always": {0, 1}, "sweep_always": {0, 2}, "no_init_pass_bitmap": {0, 1}}


def _ctx(factory, mode, extra_flags, chunk=4):
    kw = dict(MODES[mode])
    kw["flags"] = kw.get("flags", 0) | extra_flags
    return factory(chunk=chunk, **kw)


def _crafted_conditions(name, plan, n, n_live):
    """what the graph was built for, read from the plan in HBM"""
    rp, src, n_pad = plan["row_ptr"].astype(np.int64), plan["src"].astype(np.int64), plan["n_pad"]
    lb = plan["level_begin"].astype(np.int64)
    kinds = set()
    for row in list(range(n_pad)) + list(range(int(lb[0]), int(lb[1]) if len(lb) > 1 else int(lb[0]))):
        s = src[rp[row]:rp[row + 1]]
        if len(s) == 0 or s.min() >= n_pad:
            continue
        dead = s >= n_live
        where = "node" if row < n_pad else "chunk"
        kinds.add((where, "dead" if dead.all() else "mixed" if dead.any() else "live"))
    if name.startswith("fan") or (name in TILES and TILES[name][1] >= 32):
        assert {("node", "dead"), ("chunk", "dead"), ("chunk", "mixed"), ("chunk", "live")} <= kinds, (name, kinds)
    if name == "no_dead":
        assert n_live == n and all(k[1] == "live" for k in kinds), (name, kinds)
    if name == "all_sources_dead":
        assert kinds and all(k[1] == "dead" for k in kinds) and ("chunk", "dead") in kinds, (name, kinds)


@pytest.mark.parametrize("name,mode", [(name, mode) for mode in sorted(MODES) for name in sorted(set(GRAPHS) - set(TILES))] +
                         [(name, mode) for mode in TILE_MODES for name in sorted(TILES)])
def test_per_pass_state_matches_oracle_with_the_order_on(gpu_ctx_factory, name, mode):
    ids, row_ptr, src, id_low = _graph(name)
    n = len(ids)
    indeg = np.diff(row_ptr.astype(np.int64))
    o = hbo.Dense(id_low, row_ptr, src)
    with _ctx(gpu_ctx_factory, mode, ON) as ctx:
        ctx.load_dense(ids, row_ptr, src)
        on, n_live, n_live_pad = ctx.plan_live()
        assert on and n_live == int((indeg > 0).sum()) and n_live_pad == (n_live + 63) // 64 * 64
        if name.startswith("fan"):
            assert n_live == int(name[3:])
        plan = ctx.plan()
        if name in TILES:
            assert (n_live, n - n_live) == TILES[name]
            assert _tile_shapes(n, plan["n_pad"], n_live, n_live_pad) == TILE_SHAPES[name], (name, plan["n_pad"], n_live_pad)
        order = plan["order"][:n].astype(np.int64)
        assert np.all(indeg[order[:n_live]] > 0) and np.all(indeg[order[n_live:]] == 0)
        _crafted_conditions(name, plan, n, n_live)
        ctx.begin()  # (the state is NOT read here: the lean pass 0 runs where the mode has one)
        has, t, modes = True, 0, set()
        while has:
            has = ctx.step()  # the hb_step-by-step route
            ohas, ost = o.step(hbo.FRONTIER)
            assert has == ohas, t
            assert np.array_equal(ctx.registers(), o.registers()), "registers differ after pass %d" % t
            s, e = ctx.kahan()
            os_, oe = o.kahan()
            assert np.array_equal(s.view(np.uint64), os_.view(np.uint64)), "Kahan sum differs after pass %d" % t
            assert np.array_equal(e.view(np.uint64), oe.view(np.uint64)), "Kahan err differs after pass %d" % t
            assert np.array_equal(ctx.sizes(), o.sizes()), t
            assert ctx.state_hash() == o.state_hash(), t
            ps = ctx.pass_stats()[t]
            assert ps["changed"] == ost["changed"] and ps["active_edges"] == ost["active_edges"], t
            if ps["mode"] != 0:
                assert ps["touched"] <= ost["touched"], t
            modes.add(ps["mode"])
            t += 1
        ctx.finish()
        vals, keep, k = o.finish()
        assert ctx.stats()["passes"] == t
        got_ids, got_vals = ctx.results()
        assert len(got_vals) == k and np.array_equal(got_ids, ids[keep])
        assert np.array_equal(got_vals.view(np.uint64), vals[keep].view(np.uint64)), "the final list differs"
        assert np.array_equal(ctx.ranks(), hbo.rank_results(vals[keep]))
        if mode in EXPECT_MODES and t > 2:
            assert EXPECT_MODES[mode] <= modes, (name, mode, modes)
        # the same context again through hb_run (pipelined tail, staged bookkeeping): same passes, same bits
        st = ctx.run()
        assert st["passes"] == t
        ids2, vals2 = ctx.results()
        assert np.array_equal(ids2, got_ids) and np.array_equal(vals2.view(np.uint64), got_vals.view(np.uint64))


def test_isolated_hosts_from_the_node_list(gpu_ctx_factory):
    """hb_load_edges with an explicit node list that names hosts with neither an in- nor an out-link: they are dead hosts without a
    place by out-degree either, behind everybody else.  The faithful oracle learns of them from records under a skipped flag (their
    endpoints count as hosts, harmonic.rs:131); the device is handed the unflagged records alone and the hosts by the node list."""
    from stract_amd.harmonic import EdgeListGraph, ids_from_ints
    tuples = _fan(65, 40)
    lonely = [5001 + i for i in range(7)]
    fids, fvals, fst = hbo.faithful_run(EdgeListGraph.from_tuples(tuples + [(a, b, graphs.NOFOLLOW) for a, b in zip(lonely, lonely[1:] + lonely[:1])]).host_edges())
    e = EdgeListGraph.from_tuples(tuples).host_edges()
    nodes = np.concatenate([np.unique(np.concatenate([e["from"], e["to"]])), ids_from_ints(lonely)])
    for mode in TILE_MODES:
        with _ctx(gpu_ctx_factory, mode, ON) as ctx:
            ctx.load_edges(e, nodes[::-1])
            ids, row_ptr, src = ctx.graph()
            n = len(ids)
            assert n == 65 + 40 + len(lonely) == fst["n"] and ctx.plan_live() == (True, 65, 128)
            isolated = (np.diff(row_ptr.astype(np.int64)) == 0) & (np.bincount(src, minlength=n) == 0)
            assert int(isolated.sum()) == len(lonely)
            order = ctx.plan()["order"][:n].astype(np.int64)
            assert isolated[order[-len(lonely):]].all(), "hosts without any link lie last"
            st = ctx.run()
            got_ids, got_vals = ctx.results()
            assert (st["n"], st["m_eff"], st["passes"]) == (fst["n"], fst["m_eff"], fst["passes"]), mode
            assert np.array_equal(got_ids, fids) and np.array_equal(got_vals.view(np.uint64), fvals.view(np.uint64)), mode


def test_state_read_between_begin_and_pass0(gpu_ctx_factory):
    """looking at the state right after hb_begin materialises it (pass 0 then runs on memory, not lean): same passes"""
    ids, row_ptr, src, id_low = _graph("fan65")
    o = hbo.Dense(id_low, row_ptr, src)
    with _ctx(gpu_ctx_factory, "default", ON) as ctx:
        ctx.load_dense(ids, row_ptr, src)
        ctx.begin()
        assert np.array_equal(ctx.registers(), o.registers()) and np.array_equal(ctx.sizes(), o.sizes())
        has = True
        while has:
            has = ctx.step()
            assert has == o.step(hbo.FRONTIER)[0]
            assert np.array_equal(ctx.registers(), o.registers()) and ctx.state_hash() == o.state_hash()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["fan65", "rmat10", "all_sources_dead"])
@pytest.mark.parametrize("chunk", [4096, 4])
def test_on_and_off_give_the_same_statistics_and_bits(gpu_ctx_factory, chunk, name, mode):
    """The same graph with the order forced on and forced off: T, every pass' changed / active_edges / touched / mode, the final list
    and the ranks are equal.

    `touched` of a bitmap or sweep pass counts a SPLIT row when one of its chunk partials changed (hb_pass_stats), and whether a
    partial changes depends on which sources share a chunk: a changed source that raises its chunk's maximum but not the row's touches
    the row under one chunking and not under another.  That holds between any two layouts of the parent as well (chunk = 4 against
    chunk = 8), and the two orders cut a hub's list differently, so the count is compared where it is a property of the graph - chunk =
    4096, no row of these graphs is split - and at chunk = 4 both are held to the bound the suite holds it to everywhere: at most the
    number of rows with an in-edge.  Measured at chunk = 4, fan65, bitmap passes: 63 against 64 in pass 5, 54 against 55 in pass 6."""
    ids, row_ptr, src, _ = _graph(name)
    got, touched = {}, {}
    for flag in (ON, OFF):
        with _ctx(gpu_ctx_factory, mode, flag, chunk) as ctx:
            ctx.load_dense(ids, row_ptr, src)
            assert ctx.plan_live()[0] == (flag == ON)
            assert (ctx.plan()["nv"] == 0) == (chunk == 4096)
            st = ctx.run()
            ps = [(p["changed"], p["active_edges"], p["mode"]) for p in ctx.pass_stats()]
            touched[flag] = [p["touched"] for p in ctx.pass_stats()]
            rid, rv = ctx.results()
            got[flag] = (st["passes"], ps, rid.tobytes(), rv.tobytes(), ctx.ranks().tobytes())
            assert max(touched[flag]) <= st["rows_with_in_edges"]
    print("touched per pass, order on / off:", touched[ON], touched[OFF])
    assert got[ON] == got[OFF]
    if chunk == 4096:
        assert touched[ON] == touched[OFF]


@pytest.mark.parametrize("knobs", [dict(), dict(chunk=4), dict(chunk=8, tune=(0, 0, 0, 4, 2)), dict(flags=_lib.HB_FLAG_NO_XCD_MAP, chunk=16, tune=(0, 0, 0, 6, 4))],
                         ids=["default", "chunk4", "chunk8-band16-minc2", "chunk16-band64-no-xcd-map"])
def test_device_plan_equals_host_plan_with_the_order_on(gpu_ctx_factory, knobs):
    for g in (synth.RmatGraph(12, 30_000), synth.RmatGraph(14, 150_000)):
        kw = dict(knobs)
        kw["flags"] = kw.get("flags", 0) | ON
        with gpu_ctx_factory(**kw) as ctx:
            ctx.load_dense(g.ids, g.row_ptr, g.src)
            dev, live, st = ctx.plan(), ctx.plan_live(), ctx.stats()
        host = _lib.host_plan(g.row_ptr, g.src, flags=kw["flags"], chunk=kw.get("chunk", 0), tune=kw.get("tune", ()))
        assert host["live_first"] and live == (True, host["n_live"], host["n_live_pad"]) and 0 < host["n_live"] < g.n
        assert st["rows_with_in_edges"] == host["n_live"]
        assert oc.plan_equal(dev, host, g.n) and np.all(dev["order"][g.n:] == oc.NONE), (g.n, knobs)


def test_contexts_that_ignore_the_option(gpu_ctx_factory):
    """a multi-rank context, a destination-partition context and a counting context plan exactly as without the flag"""
    g = synth.RmatGraph(11, 15_000)
    cases = [dict(world_size=2, rank=1, flags=_lib.HB_FLAG_NO_RCCL), dict(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL | _lib.HB_FLAG_DEST_PARTITION),
             dict(flags=_lib.HB_FLAG_PASS_STATS), dict(flags=_lib.HB_FLAG_UNFUSED), dict(flags=_lib.HB_FLAG_NO_REORDER)]
    for kw in cases:
        plans = []
        for extra in (0, ON):
            k = dict(kw)
            k["flags"] |= extra
            with gpu_ctx_factory(chunk=16, **k) as ctx:
                ctx.load_dense(g.ids, g.row_ptr, g.src)
                plans.append(ctx.plan())
                assert ctx.plan_live()[0] is False and ctx.plan_live()[2] == plans[-1]["n_pad"], kw
        assert oc.plan_equal(plans[0], plans[1], len(plans[0]["order"])), kw


OPERATOR_SEED = 4201


@pytest.mark.parametrize("index,kind,chunk", [(0, "stars", 4), (1, "bipartite", 8), (2, "uniform", 16), (3, "dense_core", 4)])
def test_operators_on_a_live_first_plan(gpu_ctx_factory, index, kind, chunk):
    """the bodies of tests/operator_cases.py once on a plan with the order forced on"""
    rng = np.random.default_rng([OPERATOR_SEED, index])
    _, tuples = oc.draw_graph(rng, kind)
    _, tune, _ = oc.draw_layout(rng, chunk)
    flags = _lib.HB_FLAG_ALL_RELS | ON
    graph = graphs.dense_from_tuples(tuples)
    plan = _lib.host_plan(graph[1], graph[2], ON, chunk, tune)
    assert plan["live_first"]
    picks = oc.picks_of(oc.layout_conditions(plan, graph[1], chunk))
    what = dict(case=index, kind=kind, chunk=chunk, tune=tune, flags=flags, seed=OPERATOR_SEED)
    dry = oc.Tally()
    oc.run_bodies(None, graph, OPERATOR_SEED, index, what, picks, dry)
    with oc.load(gpu_ctx_factory, tuples, chunk, tune, flags) as ctx:
        got = ctx.graph()
        assert all(np.array_equal(a, b) for a, b in zip(got, graph))
        assert ctx.plan_live() == (True, plan["n_live"], plan["n_live_pad"])
        assert oc.plan_equal(ctx.plan(), plan, len(graph[0]))
        tally = oc.Tally()
        oc.run_bodies(ctx, got, OPERATOR_SEED, index, what, picks, tally)
    assert tally.as_dict() == dry.as_dict()
    assert sum(tally.compared.get(op, 0) for op in oc.OPERATORS) > 0
