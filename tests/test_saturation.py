"""Saturated rows in the dense passes (HB_FLAG_NO_SATURATION switches it off).  U is the register-wise maximum of
the initial counters of the hosts with an out-link; a node row whose counter is >= U in every register can never change again, so from
then on the dense passes t >= 1 neither gather for it nor compute the hub chunks below it.  Nothing that is computed may move: every
pass leaves the oracle's registers, Kahan words, sizes and changed count, by hb_step and by hb_run, on against off, and the bitmap the
kernels keep is exactly {row visited: oracle counter >= U} after every dense pass t >= 1, handed down to every chunk of a saturated
hub row's tree in the same pass.

The crafted graphs (ids 1.. are ring hosts; all at chunk = 4, where a hub row becomes a tree):
  ring63 / 64 / 65 / 128  a ring with chords: strongly connected, small diameter - everything saturates within a few passes; the node
                          counts put the last 16-row word of the bitmap on either side of a tile
  ring_sink               the ring plus a sink (no out-link) whose own register lies ABOVE U: the test is >=, not ==
  tendril                 the ring plus a record holder whose only out-link goes to a host without out-links: its register is part of U
                          and never reaches the ring - nothing saturates, every pass takes the path it took before
  hubs                    a slow ring (diameter n / 2: tens of passes) with two hubs fed from all around it - a two-level and a
                          three-level tree (read back from the plan) - that saturate long before the ring does: rows that saturate in
                          pass t and carry their counter over in t + 1 while Kahan-dirty, chunks skipped while their sources still
                          change, and (default thresholds) bitmap and sweep passes over the stale partials afterwards
  rmat10                  an R-MAT graph: dead hosts, sinks, hubs by chance

Dense passes "through the last pass" are forced with HB_FLAG_NO_FRONTIER, the switch the mode tests of the suite use for it."""
import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib, synth
from tests import graphs

pytestmark = pytest.mark.gpu

OFF = _lib.HB_FLAG_NO_SATURATION
SINK = graphs.crafted_id_low(5, 30)      # register 5 = 30: far above anything a few hundred small ids set
HOLDER = graphs.crafted_id_low(9, 33)
TENDRIL_END = 5000


def _jp(id_low):
    """(register index, value) of HyperLogLog::default() + add(id) for every id (hyperloglog.rs:4385-4400)"""
    out = []
    for v in id_low.tolist():
        h = (int(v) * graphs.HLL_MUL) % (1 << 64)
        w = (h << 6) % (1 << 64)
        out.append((h >> 58, 65 if w == 0 else 64 - w.bit_length() + 1))
    return np.array(out, dtype=np.int64)


def _ring(n, chords=True):
    e = {(v, v % n + 1) for v in range(1, n + 1)}
    e |= {(v, (v * 7 + 3) % n + 1) for v in range(1, n + 1)} if chords else {(v, (v + 1) % n + 1) for v in range(1, n + 1)}
    return {(f, t) for f, t in e if f != t}


def _ring_sink(n=90):
    return _ring(n) | {(v, SINK) for v in range(1, 7)}


def _tendril(n=90):
    return _ring(n) | {(HOLDER, TENDRIL_END)}


def _hubs(n=60):
    a, b = n + 1, n + 2
    e = _ring(n, chords=False)
    e |= {(v, a) for v in range(1, n + 1, 6)} | {(a, 1)}                  # 10 sources
    e |= {(v, b) for v in range(1, n + 1) if v % 6 != 3} | {(b, 2)}       # 50 sources
    return e


GRAPHS = {"ring63": lambda: _ring(63), "ring64": lambda: _ring(64), "ring65": lambda: _ring(65), "ring128": lambda: _ring(128),
          "ring_sink": _ring_sink, "tendril": _tendril, "hubs": _hubs}
ALL_SATURATE = ("ring63", "ring64", "ring65", "ring128", "ring_sink", "hubs")  # strongly connected but for the sink
_BUILT = {}


def _graph(name):
    if name not in _BUILT:
        if name == "rmat10":
            g = synth.RmatGraph(10, 6000)
            ids, row_ptr, src = g.ids.copy(), g.row_ptr.copy(), g.src.copy()
        else:
            ids, row_ptr, src = graphs.dense_from_tuples(sorted((f, t, 0) for f, t in GRAPHS[name]()))
        id_low = np.ascontiguousarray(ids["lo"])
        jp = _jp(id_low)
        outdeg = np.bincount(src, minlength=len(ids))
        u = np.zeros(64, dtype=np.uint8)
        for (j, p), od in zip(jp, outdeg):
            if od:
                u[j] = max(u[j], p)
        _BUILT[name] = (ids, row_ptr, src, id_low, u, jp, outdeg)
    return _BUILT[name]


MODES = {
    "default": dict(),
    "dense_only": dict(flags=_lib.HB_FLAG_NO_FRONTIER),
    "no_init_pass": dict(flags=_lib.HB_FLAG_NO_INIT_PASS | _lib.HB_FLAG_NO_FRONTIER),
    "sweep_after_dense": dict(tune=(0, 0, 0, 0, 0, 0, 1)),
    "live_first_dense": dict(flags=_lib.HB_FLAG_LIVE_FIRST | _lib.HB_FLAG_NO_FRONTIER),
    "unroll4_node_rows": dict(flags=_lib.HB_FLAG_NO_FRONTIER, tune=(0, 4)),
}


def _ctx(factory, mode, extra_flags=0, chunk=4):
    kw = dict(MODES[mode])
    kw["flags"] = kw.get("flags", 0) | extra_flags
    return factory(chunk=chunk, **kw)


def _roots(plan, n):
    """sid of the node row at the top of every hub chunk's tree, and the chunk levels below every hub row (a tree of that many + 1 levels)"""
    rp, src, n_pad, nv = plan["row_ptr"].astype(np.int64), plan["src"].astype(np.int64), plan["n_pad"], plan["nv"]
    order = plan["order"].astype(np.int64)
    root = np.full(nv, -1, dtype=np.int64)
    depth = np.zeros(nv, dtype=np.int64)
    for row in list(range(n_pad)) + list(range(n_pad + nv - 1, n_pad - 1, -1)):
        s = src[rp[row]:rp[row + 1]]
        if len(s) == 0 or s[0] < n_pad:
            continue
        root[s - n_pad] = order[row] if row < n_pad else root[row - n_pad]
        depth[s - n_pad] = 1 if row < n_pad else depth[row - n_pad] + 1
    used = np.diff(rp)[n_pad:] > 0  # (the levels are padded to whole tiles with empty rows: nobody's chunks)
    assert (root[used] >= 0).all() and (root < n).all() and (root[~used] == -1).all()
    deepest = {}
    for r, d in zip(root[used].tolist(), depth[used].tolist()):
        deepest[r] = max(deepest.get(r, 0), d)
    return root, deepest


@pytest.mark.parametrize("name", sorted(GRAPHS) + ["rmat10"])
def test_u_is_the_maximum_over_the_hosts_with_an_out_link(gpu_ctx_factory, name):
    ids, row_ptr, src, id_low, u, jp, outdeg = _graph(name)
    with _ctx(gpu_ctx_factory, "default") as ctx:
        ctx.load_dense(ids, row_ptr, src)
        on, got, node, virt = ctx.saturation()
        assert on and np.array_equal(got, u), (got, u)
        assert not node.any() and not virt.any()
    if name == "ring_sink":
        s = int(np.flatnonzero(id_low == SINK)[0])
        assert outdeg[s] == 0 and tuple(jp[s]) == (5, 30) and u[5] < 30, "the sink's register is left out of U"
    if name == "tendril":
        h = int(np.flatnonzero(id_low == HOLDER)[0])
        assert outdeg[h] == 1 and u[9] == 33


@pytest.mark.parametrize("name,mode", [(name, mode) for mode in sorted(MODES) for name in sorted(GRAPHS) + ["rmat10"]])
def test_per_pass_state_and_bitmap_match_the_oracle(gpu_ctx_factory, name, mode):
    ids, row_ptr, src, id_low, u, jp, outdeg = _graph(name)
    n = len(ids)
    indeg = np.diff(row_ptr.astype(np.int64))
    o = hbo.Dense(id_low, row_ptr, src)
    with _ctx(gpu_ctx_factory, mode) as ctx:
        ctx.load_dense(ids, row_ptr, src)
        plan = ctx.plan()
        _, _, n_live_pad = ctx.plan_live()
        visited = np.zeros(n, dtype=bool)  # by the node-row launches of the passes t >= 1
        visited[plan["order"][:min(n_live_pad, plan["n_pad"])][plan["order"][:min(n_live_pad, plan["n_pad"])] < n]] = True
        root, deepest = _roots(plan, n)
        if name == "hubs":
            assert sorted(deepest.values()) == [1, 2], "a two-level and a three-level tree at chunk = 4: %r" % (deepest,)
        ctx.begin()
        has, t, modes = True, 0, []
        node_prev, virt_prev = np.zeros(n, dtype=bool), np.zeros(plan["nv"], dtype=bool)
        first_sat, carried_dirty = None, 0
        while has:
            regs_before, kerr_before = o.registers().copy(), o.kahan()[1].copy()
            has = ctx.step()
            ohas, ost = o.step(hbo.FRONTIER)
            assert has == ohas, t
            oregs = o.registers()
            assert np.array_equal(ctx.registers(), oregs), "registers differ after pass %d" % t
            s, e = ctx.kahan()
            os_, oe = o.kahan()
            assert np.array_equal(s.view(np.uint64), os_.view(np.uint64)), "Kahan sum differs after pass %d" % t
            assert np.array_equal(e.view(np.uint64), oe.view(np.uint64)), "Kahan err differs after pass %d" % t
            assert np.array_equal(ctx.sizes(), o.sizes()), t
            assert ctx.state_hash() == o.state_hash(), t
            ps = ctx.pass_stats()[t]
            assert ps["changed"] == ost["changed"] and ps["active_edges"] == ost["active_edges"], t
            on, got_u, node, virt = ctx.saturation()
            assert on and np.array_equal(got_u, u)
            if ps["mode"] == 0 and t >= 1:
                want = visited & (oregs >= u).all(axis=1)
                assert np.array_equal(node, want), "bitmap after dense pass %d: %r against %r" % (t, np.flatnonzero(node), np.flatnonzero(want))
                assert np.array_equal(virt, np.where(root >= 0, node[root], False)), "hub chunks after dense pass %d" % t
                # rows that were saturated BEFORE this pass, changed in the pass before it (carry-over store) with a Kahan error word to flush
                was = node_prev & (regs_before != o_prev_regs).any(axis=1) if t >= 2 else np.zeros(n, dtype=bool)
                carried_dirty += int((was & (kerr_before != 0.0)).sum())
            else:
                assert np.array_equal(node, node_prev) and np.array_equal(virt, virt_prev), "only dense passes t >= 1 write the bitmap (pass %d)" % t
            assert not (node_prev & ~node).any()
            if first_sat is None and node.any():
                first_sat = t
            node_prev, virt_prev, o_prev_regs = node, virt, regs_before
            modes.append(ps["mode"])
            t += 1
        ctx.finish()
        vals, keep, k = o.finish()
        got_ids, got_vals = ctx.results()
        assert len(got_vals) == k and np.array_equal(got_ids, ids[keep])
        assert np.array_equal(got_vals.view(np.uint64), vals[keep].view(np.uint64)), "the final list differs"
        assert np.array_equal(ctx.ranks(), hbo.rank_results(vals[keep]))
        live = indeg > 0
        dense_to_the_end = mode != "default" and mode != "sweep_after_dense"
        if dense_to_the_end:
            assert set(modes) == {0}
        if name == "tendril":
            assert first_sat is None, "the holder's register never reaches the ring: nothing saturates"
        elif name in ALL_SATURATE:
            assert first_sat is not None and first_sat < t - 1, (first_sat, t)
            if dense_to_the_end:
                assert node[live].all(), "every live row is saturated by the end: %r" % (np.flatnonzero(live & ~node),)
        if name == "ring_sink" and dense_to_the_end:
            s_ = int(np.flatnonzero(id_low == SINK)[0])
            assert node[s_] and oregs[s_][5] == 30 > u[5]
        if name == "hubs":
            if dense_to_the_end:
                assert carried_dirty > 0, "no saturated row carried its counter over while Kahan-dirty"
                hub_rows = [r for r in deepest]
                sat_at = first_sat
                assert sat_at is not None and sat_at + 5 < t, "the hubs saturate long before the ring does"
                assert all(node[r] for r in hub_rows)
            else:
                assert first_sat is not None and set(modes[first_sat + 1:]) & {1, 2}, "bitmap / sweep passes follow the dense skipping: %r" % (modes,)
        # the same context again through hb_run: hb_begin clears the bits, same passes, same result bits
        st = ctx.run()
        assert st["passes"] == t
        ids2, vals2 = ctx.results()
        assert np.array_equal(ids2, got_ids) and np.array_equal(vals2.view(np.uint64), got_vals.view(np.uint64))
        st = ctx.run()
        assert st["passes"] == t and np.array_equal(ctx.results()[1].view(np.uint64), got_vals.view(np.uint64))
        ctx.begin()
        assert not ctx.saturation()[2].any() and not ctx.saturation()[3].any(), "hb_begin clears the bitmap"


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ["hubs", "ring_sink", "tendril", "rmat10"])
@pytest.mark.parametrize("chunk", [4096, 4])
def test_on_and_off_give_the_same_statistics_and_bits(gpu_ctx_factory, chunk, name, mode):
    """T, every pass' changed / active_edges / mode, the final list and the ranks are equal with the skipping on and off; `touched`
    (layout-dependent on split rows; a stale partial may also change where a fresh one would not) is compared
    where no row is split."""
    ids, row_ptr, src = _graph(name)[:3]
    got, touched = {}, {}
    for flag in (0, OFF):
        with _ctx(gpu_ctx_factory, mode, flag, chunk) as ctx:
            ctx.load_dense(ids, row_ptr, src)
            assert ctx.saturation()[0] == (flag == 0)
            st = ctx.run()
            ps = [(p["changed"], p["active_edges"], p["mode"]) for p in ctx.pass_stats()]
            touched[flag] = [p["touched"] for p in ctx.pass_stats()]
            rid, rv = ctx.results()
            got[flag] = (st["passes"], ps, rid.tobytes(), rv.tobytes(), ctx.ranks().tobytes())
            assert max(touched[flag]) <= st["rows_with_in_edges"]
    print("touched per pass, skipping on / off:", touched[0], touched[OFF])
    assert got[0] == got[OFF]
    if chunk == 4096:
        assert touched[0] == touched[OFF]


def test_contexts_outside_the_gate_run_as_before(gpu_ctx_factory):
    """a multi-rank context, a destination-partition context, a counting and an unfused context keep no bitmap, with or without the flag,
    and plan and run exactly alike"""
    ids, row_ptr, src = _graph("hubs")[:3]
    cases = [dict(world_size=2, rank=1, flags=_lib.HB_FLAG_NO_RCCL), dict(world_size=2, rank=0, flags=_lib.HB_FLAG_NO_RCCL | _lib.HB_FLAG_DEST_PARTITION),
             dict(flags=_lib.HB_FLAG_PASS_STATS), dict(flags=_lib.HB_FLAG_UNFUSED)]
    for kw in cases:
        seen = []
        for extra in (0, OFF):
            k = dict(kw)
            k["flags"] |= extra
            with gpu_ctx_factory(chunk=4, **k) as ctx:
                ctx.load_dense(ids, row_ptr, src)
                assert ctx.saturation() == (False, None, None, None), kw
                plan = ctx.plan()
                if "world_size" in kw:
                    seen.append((plan["row_ptr"].tobytes(), plan["src"].tobytes()))
                    continue
                st = ctx.run()
                seen.append((plan["row_ptr"].tobytes(), plan["src"].tobytes(), st["passes"], ctx.results()[1].tobytes(),
                             [(p["changed"], p["active_edges"], p["mode"], p["touched"]) for p in ctx.pass_stats()]))
        assert seen[0] == seen[1], kw
