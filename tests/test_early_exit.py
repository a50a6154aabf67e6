"""A dense row leaves its gather loop once its accumulator has reached U (HB_FLAG_NO_EARLY_EXIT switches it off,
HB_FLAG_FORCE_EARLY_EXIT on from pass 1).  Every source counter and every hub-chunk partial is <= U register by register, so once a
row's accumulator - its own counter merged with the sources gathered so far; for a hub chunk the sources alone - is >= U in all 64
registers, what is still to come cannot change it.  Nothing that is computed may move: every pass leaves the oracle's registers, Kahan
words, sizes, `changed` and `active_edges`, by hb_step and twice by hb_run, with the exit forced, off and under the default rule; and the
number of work rows the kernels report as having left early is exactly what a host model of the launched rounds gives on the exported plan.

The crafted graphs.  Every host that is not a record holder has an id that sets register 3 to 5, so U is {3: 5} plus the holders'
registers and the slot at which a row reaches U is the slot of the last holder register it still misses:
  row40(p)   T with 40 direct sources s1..s40 of strictly decreasing out-degree (si also feeds the sinks 1..40-i: rows of 39..1 sources,
             among them exactly 4 UNROLL and 4 UNROLL + 1).  Holders feed s1 (20: 25), s2 (40: 20) and sp (55: 30): after pass 0 they sit
             in the sources, T's own counter has register 3 only, and in pass 1 T reaches U at slot p - the last slot of round one, the
             first slot of round two, or its last source (every other register of U present after round one).  Z, a sink whose own
             register (60: 40) lies above U, is fed by copies of the holders directly: after pass 0 its own counter alone is >= U.
  hub200     H with 200 sources (its list is cut into hub chunks), sinks fed by prefixes of them (192..8 sources).  Holders (55: 30)
             feed h5 and h70, holders (10: 28) reach h6 and h71 one pass later through an intermediate host: in pass 1 nobody reaches
             U, in pass 2 the chunks that hold both registers leave early and the others do not.
  rmat10     an R-MAT graph.
The row and chunk order is read from the plan export."""
import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib, synth
from tests import graphs
from tests import test_saturation as sat_tests

pytestmark = pytest.mark.gpu

FORCE, OFF = _lib.HB_FLAG_FORCE_EARLY_EXIT, _lib.HB_FLAG_NO_EARLY_EXIT
WAYS = {"forced": FORCE, "off": OFF, "default": 0}
CONFIGS = {"u2c64": (64, 0), "u1c64": (64, 1), "u4c64": (64, 4), "u1c16": (16, 1)}  # chunk, tune[1] low byte (0: node rows 2, hub chunks 4)
MODES = {
    "default": 0,
    "dense_only": _lib.HB_FLAG_NO_FRONTIER,
    "no_init_pass": _lib.HB_FLAG_NO_INIT_PASS | _lib.HB_FLAG_NO_FRONTIER,
    "live_first_dense": _lib.HB_FLAG_LIVE_FIRST | _lib.HB_FLAG_NO_FRONTIER,
}
POSITIONS = ("last_slot_of_a_round", "first_slot_of_the_next_round", "last_source")


def _unrolls(cfg):
    t = CONFIGS[cfg][1]
    return (t or 2), (t or 4)  # node rows, hub chunks (hb_api_pass.inc pass_unroll)


class _Ids:
    def __init__(self):
        self.place = 0

    def node(self, low):
        self.place += 1
        return (self.place << 64) | low

    def plain(self):
        return self.node(graphs.crafted_id_low(3, 5, self.place + 1))

    def holder(self, index, value):
        return self.node(graphs.crafted_id_low(index, value, self.place + 1))


def _row40(p):
    ids = _Ids()
    t = ids.plain()
    s = [ids.plain() for _ in range(40)]
    sinks = [ids.plain() for _ in range(39)]
    z = ids.node(graphs.crafted_id_low(60, 40, 7))
    e = [(s[i], t) for i in range(40)]
    e += [(s[i], sinks[k]) for i in range(40) for k in range(39 - i)]  # sink k: s1 .. s(39 - k)
    e += [(ids.holder(20, 25), s[0]), (ids.holder(40, 20), s[1]), (ids.holder(55, 30), s[p - 1])]
    e += [(s[i], z) for i in range(20)] + [(ids.holder(20, 25), z), (ids.holder(40, 20), z), (ids.holder(55, 30), z)]
    return e, dict(t=t, z=z)


def _hub200():
    ids = _Ids()
    hub = ids.plain()
    h = [ids.plain() for _ in range(200)]
    sinks = [ids.plain() for _ in range(24)]
    e = [(x, hub) for x in h]
    e += [(h[i], sinks[k]) for i in range(200) for k in range((199 - i) // 8)]
    for at in (4, 69):
        e.append((ids.holder(55, 30), h[at]))
    for at in (5, 70):
        mid = ids.plain()
        e += [(ids.holder(10, 28), mid), (mid, h[at])]
    return e, dict(hub=hub)


class _Reference:
    """A graph, U, and the oracle's state after every pass (computed once per graph, read-only)."""

    def __init__(self, name):
        self.named = {}
        if name == "rmat10":
            g = synth.RmatGraph(10, 6000)
            self.ids, self.row_ptr, self.src = g.ids.copy(), g.row_ptr.copy(), g.src.copy()
        elif name in ("hubs", "tendril"):
            self.ids, self.row_ptr, self.src = sat_tests._graph(name)[:3]
        else:
            kind, _, arg = name.partition(":")
            e, named = _row40(int(arg)) if kind == "row40" else _hub200()
            self.ids, self.row_ptr, self.src = graphs.dense_from_tuples([(f, t, 0) for f, t in e])
            all_ids = [(int(r["hi"]) << 64) | int(r["lo"]) for r in self.ids]
            self.named = {k: all_ids.index(v) for k, v in named.items()}
        self.n = len(self.ids)
        self.id_low = np.ascontiguousarray(self.ids["lo"])
        self.outdeg = np.bincount(self.src, minlength=self.n)
        self.u = np.zeros(64, dtype=np.uint8)
        for (j, v), od in zip(sat_tests._jp(self.id_low), self.outdeg):
            if od:
                self.u[j] = max(self.u[j], v)
        o = hbo.Dense(self.id_low, self.row_ptr, self.src)
        self.initial = o.registers().copy()
        self.passes = []
        has = True
        while has:
            has, st = o.step(hbo.FRONTIER)
            ks, ke = o.kahan()
            self.passes.append(dict(has=has, changed=int(st["changed"]), active=int(st["active_edges"]), regs=o.registers().copy(), ks=ks.copy(),
                                    ke=ke.copy(), sizes=o.sizes().copy(), hash=o.state_hash()))
        self.vals, self.keep, self.k = o.finish()
        self.vals, self.keep = self.vals.copy(), self.keep.copy()
        o.close()


_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = _Reference(name)
    return _REF[name]


def _model(plan, live, n, prev_regs, node_sat, virt_sat, u, unroll_node, unroll_hub):
    """One dense pass t >= 1 of the EARLY instances on the exported plan: per work row that enters its gather loop, (the 1-based slot at
    which the prefix maximum - merged with the own counter for a node row - is >= U or None, whether it left the loop with rounds to
    go).  prev_regs: the oracle's counters before the pass (input order); *_sat: the bitmap before the pass."""
    live_first, n_live, _ = live
    n_pad, nv = plan["n_pad"], plan["nv"]
    rp, src, order = plan["row_ptr"].astype(np.int64), plan["src"].astype(np.int64), plan["order"].astype(np.int64)
    state = np.zeros((n_pad + nv, 64), dtype=np.uint8)
    sat = np.zeros(n_pad + nv, dtype=bool)
    real = order < n
    state[:n_pad][real] = prev_regs[order[real]]
    sat[:n_pad][real] = node_sat[order[real]]
    sat[n_pad:] = virt_sat
    out = {}

    def walk(row, node_row):
        rounds = 4 * (unroll_node if node_row else unroll_hub)
        beg, end = int(rp[row]), int(rp[row + 1])
        if beg == end or sat[row]:
            return
        real_src = src[beg] < n_pad
        assert ((src[beg:end] < n_pad) == real_src).all()
        limit = n_live if (live_first and real_src) else 1 << 62
        acc = state[row].copy() if node_row else np.zeros(64, dtype=np.uint8)
        gathered = src[beg:end][src[beg:end] < limit]
        full = np.maximum(acc, state[gathered].max(axis=0)) if len(gathered) else acc
        if src[beg] < limit:
            reach = None
            for k, s in enumerate(src[beg:end].tolist()):
                if s < limit:
                    acc = np.maximum(acc, state[s])
                if reach is None and (acc >= u).all():
                    reach = k + 1
            left = False
            if reach is not None:
                stop = -(-reach // rounds) * rounds  # the test comes after the round's merges
                left = stop < end - beg
                if not node_row:
                    assert (full == u).all(), "a chunk that leaves early holds the true maximum, exactly U"
            out[row] = (reach, left)
        if not node_row:
            state[row] = full

    lb = [int(x) for x in plan["level_begin"]]
    for l in range(len(lb) - 1):
        for row in range(lb[l], lb[l + 1]):
            walk(row, False)
    for row in range(n_pad):
        walk(row, True)
    return out


def _drive(factory, ref, cfg, mode, way, expect=None):
    """One context through every pass by hb_step against the reference, then twice by hb_run; returns what the three ways must agree on
    and, for the forced way, the model's rows per dense pass t >= 1."""
    chunk, tune1 = CONFIGS[cfg]
    un, uh = _unrolls(cfg)
    models = []
    with factory(chunk=chunk, flags=MODES[mode] | WAYS[way], tune=(0, tune1)) as ctx:
        ctx.load_dense(ref.ids, ref.row_ptr, ref.src)
        plan, live = ctx.plan(), ctx.plan_live()
        on, u, _, _ = ctx.saturation()
        assert on and np.array_equal(u, ref.u)
        assert ctx.early_exit() == (False, 0)
        ctx.begin()
        stats, prev = [], ref.initial
        for t, want in enumerate(ref.passes):
            _, _, node_sat, virt_sat = ctx.saturation()
            has = ctx.step()
            assert has == want["has"], t
            assert np.array_equal(ctx.registers(), want["regs"]), "registers differ after pass %d (%s)" % (t, way)
            s, e = ctx.kahan()
            assert np.array_equal(s.view(np.uint64), want["ks"].view(np.uint64)), "Kahan sum differs after pass %d (%s)" % (t, way)
            assert np.array_equal(e.view(np.uint64), want["ke"].view(np.uint64)), "Kahan err differs after pass %d (%s)" % (t, way)
            assert np.array_equal(ctx.sizes(), want["sizes"]), t
            assert ctx.state_hash() == want["hash"], t
            ps = ctx.pass_stats()[t]
            assert ps["changed"] == want["changed"] and ps["active_edges"] == want["active"], (t, way)
            ran, count = ctx.early_exit()
            if way == "off" or t == 0:
                assert (ran, count) == (False, 0), (t, way)
            if way == "forced" and t >= 1 and ps["mode"] == 0:
                rows = _model(plan, live, ref.n, prev, node_sat, virt_sat, ref.u, un, uh)
                models.append((t, rows))
                want_count = sum(1 for _, left in rows.values() if left)
                print("pass %d: %d rows enter their loop, %d reach U, %d leave early (device: %d)" % (
                    t, len(rows), sum(1 for r, _ in rows.values() if r), want_count, count))
                assert ran, "pass %d did not run the EARLY instances" % t
                assert count == want_count, "rows that left early in pass %d: device %d, model %d" % (t, count, want_count)
            stats.append((ps["changed"], ps["active_edges"], ps["mode"]))
            prev = want["regs"]
        assert not has
        ctx.finish()
        got_ids, got_vals = ctx.results()
        assert len(got_vals) == ref.k and np.array_equal(got_ids, ref.ids[ref.keep])
        assert np.array_equal(got_vals.view(np.uint64), ref.vals[ref.keep].view(np.uint64)), "the final list differs (%s)" % way
        ranks = ctx.ranks()
        assert np.array_equal(ranks, hbo.rank_results(ref.vals[ref.keep]))
        for _ in range(2):  # the same context again through hb_run: hb_begin resets the rule's sum
            st = ctx.run()
            assert st["passes"] == len(ref.passes)
            assert np.array_equal(ctx.results()[1].view(np.uint64), got_vals.view(np.uint64)), way
            assert [(p["changed"], p["active_edges"], p["mode"]) for p in ctx.pass_stats()] == stats
    return (stats, got_vals.tobytes(), ranks.tobytes()), models, plan


def _three_ways(factory, name, cfg, mode):
    ref = _ref(name)
    got = {way: _drive(factory, ref, cfg, mode, way) for way in WAYS}
    assert got["forced"][0] == got["off"][0] == got["default"][0]
    return ref, got["forced"][1], got["forced"][2]


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("position", POSITIONS)
def test_a_node_row_leaves_at_the_round_in_which_it_reaches_u(gpu_ctx_factory, position, cfg):
    un, _ = _unrolls(cfg)
    rounds = 4 * un
    p = {"last_slot_of_a_round": rounds, "first_slot_of_the_next_round": rounds + 1, "last_source": 40}[position]
    ref, models, plan = _three_ways(gpu_ctx_factory, "row40:%d" % p, cfg, "dense_only")
    t1, rows = models[0]
    assert t1 == 1
    dev_of = {int(s): r for r, s in enumerate(plan["order"].tolist())}
    lens = np.diff(plan["row_ptr"].astype(np.int64))

    def direct(r):
        return r < plan["n_pad"] and plan["src"][plan["row_ptr"][r]] < plan["n_pad"]

    z = dev_of[ref.named["z"]]
    assert (ref.passes[0]["regs"][ref.named["z"]] >= ref.u).all() and ref.passes[0]["regs"][ref.named["z"]][60] == 40 > ref.u[60]
    assert rows[z][0] == 1, "Z's own counter alone is >= U"
    if direct(z):
        assert lens[z] == 23 and rows[z] == (1, True), "... so it leaves after its first round"
    t = dev_of[ref.named["t"]]
    if direct(t):  # (at chunk = 16 T is a hub row: its chunks are modelled all the same)
        assert lens[t] == 40
        assert rows[t] == (p, -(-p // rounds) * rounds < 40), rows[t]
        by_len = {int(lens[r]): rows[r] for r in rows if direct(r) and lens[r] > 1}
        assert rounds in by_len and rounds + 1 in by_len, "rows of exactly 4 UNROLL and 4 UNROLL + 1 sources"
        if p == rounds:
            assert by_len[rounds] == (rounds, False) and by_len[rounds + 1] == (rounds, True)
    if direct(z) or p < 40:  # (at chunk = 16 Z and T are hub rows; with the holder on s40 no chunk of theirs holds all of U before its end)
        assert sum(left for _, r in models for _, left in r.values()) >= 1


@pytest.mark.parametrize("mode", ["dense_only", "live_first_dense"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_some_chunks_of_a_hub_leave_early_and_some_do_not(gpu_ctx_factory, cfg, mode):
    ref, models, plan = _three_ways(gpu_ctx_factory, "hub200", cfg, mode)
    n_pad, nv = plan["n_pad"], plan["nv"]
    assert nv > 0 and len(plan["level_begin"]) >= 2
    _, uh = _unrolls(cfg)
    lens = np.diff(plan["row_ptr"].astype(np.int64))
    left = {r for _, rows in models for r, (_, x) in rows.items() if x and r >= n_pad}
    stayed = {r for _, rows in models for r, (reach, _) in rows.items() if reach is None and r >= n_pad and lens[r] > 4 * uh}
    assert left, "no chunk left early"
    if mode == "dense_only":  # (under the live-first order the live sources lead every list: the chunks behind them hold dead sources only)
        assert stayed - left, "no chunk of more than one round that never reaches U: %r / %r" % (sorted(left), sorted(stayed))
    first = min(t for t, rows in models if any(x for _, x in rows.values()))
    assert first == 2, "the second holder register arrives a pass late: nobody reaches U in pass 1"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_rmat_every_pass_three_ways(gpu_ctx_factory, cfg, mode):
    """(few rows of this sparse graph ever hold all of U: the crafted graphs are where exits are asserted to occur; here the count is
    compared, whatever it is, and the passes that test every round for nothing must not move a bit)"""
    _three_ways(gpu_ctx_factory, "rmat10", cfg, mode)


@pytest.mark.parametrize("mode", ["default", "no_init_pass", "live_first_dense"])
def test_the_crafted_row_in_the_other_modes(gpu_ctx_factory, mode):
    _three_ways(gpu_ctx_factory, "row40:8", "u2c64", mode)


def _early_per_pass(factory, ref, flags, chunk=4):
    """per pass: (mode, the pass ran the EARLY instances)"""
    out = []
    with factory(chunk=chunk, flags=flags) as ctx:
        ctx.load_dense(ref.ids, ref.row_ptr, ref.src)
        plan, live = ctx.plan(), ctx.plan_live()
        ctx.begin()
        has, t = True, 0
        while has:
            has = ctx.step()
            assert np.array_equal(ctx.registers(), ref.passes[t]["regs"]), t
            ran, count = ctx.early_exit()
            assert ran or count == 0
            out.append((ctx.pass_stats()[t]["mode"], ran))
            t += 1
        assert t == len(ref.passes)
    return out, plan, live


def test_nothing_saturates_nothing_runs_early(gpu_ctx_factory):
    ref = _ref("tendril")
    for flags in (0, _lib.HB_FLAG_NO_FRONTIER):
        got, _, _ = _early_per_pass(gpu_ctx_factory, ref, flags)
        assert not any(ran for _, ran in got), got


def test_the_first_early_pass_is_the_one_the_sum_predicts(gpu_ctx_factory):
    """the rule: pass t runs EARLY when the rows found saturated by the dense passes 1 .. t - 1 of the run hold at least m / 64 of the
    edges as sources; on the slow ring the hubs saturate tens of passes before the ring does"""
    ref = _ref("hubs")
    got, plan, live = _early_per_pass(gpu_ctx_factory, ref, _lib.HB_FLAG_NO_FRONTIER)
    assert all(mode == 0 for mode, _ in got)
    order = plan["order"][:min(live[2], plan["n_pad"])]
    visited = np.zeros(ref.n, dtype=bool)
    visited[order[order < ref.n]] = True
    m = len(ref.src)
    want = [False, False]  # pass 0 never; pass 1: no dense pass t >= 1 has looked for saturated rows yet
    for t in range(2, len(ref.passes)):
        sat = visited & (ref.passes[t - 1]["regs"] >= ref.u).all(axis=1)
        want.append(int(ref.outdeg[sat].sum()) * 64 >= m)
    assert [ran for _, ran in got] == want, (got, want)
    assert True in want and want.index(True) + 5 < len(want), "the hubs saturate long before the ring does: %r" % (want,)
    off, _, _ = _early_per_pass(gpu_ctx_factory, ref, _lib.HB_FLAG_NO_FRONTIER | OFF)
    assert not any(ran for _, ran in off)
    nosat, _, _ = _early_per_pass(gpu_ctx_factory, ref, _lib.HB_FLAG_NO_FRONTIER | FORCE | _lib.HB_FLAG_NO_SATURATION)
    assert not any(ran for _, ran in nosat), "HB_FLAG_NO_SATURATION implies HB_FLAG_NO_EARLY_EXIT"


def test_contexts_outside_the_gate_never_run_early(gpu_ctx_factory):
    ref = _ref("hubs")
    cases = [dict(flags=_lib.HB_FLAG_PASS_STATS), dict(flags=_lib.HB_FLAG_UNFUSED),
             dict(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL | _lib.HB_FLAG_DEST_PARTITION)]
    for kw in cases:
        seen = []
        for extra in (0, FORCE):
            k = dict(kw)
            k["flags"] |= extra | _lib.HB_FLAG_NO_FRONTIER
            with gpu_ctx_factory(chunk=4, **k) as ctx:
                ctx.load_dense(ref.ids, ref.row_ptr, ref.src)
                assert ctx.early_exit() == (False, 0)
                if "world_size" in kw:
                    continue
                st = ctx.run()
                assert ctx.early_exit() == (False, 0), kw
                seen.append((st["passes"], ctx.results()[1].tobytes(), [(p["changed"], p["active_edges"], p["mode"], p["touched"]) for p in ctx.pass_stats()]))
        assert len(seen) != 2 or seen[0] == seen[1], kw
