"""The live-first device order (HB_FLAG_LIVE_FIRST) in the host planner: the hosts with an in-edge first, the
hosts without one ("dead") behind them, each part by descending out-degree; everything else about the plan as before.  Host only."""
import numpy as np
import pytest

from stract_amd import _lib, synth

ON = _lib.HB_FLAG_LIVE_FIRST
OFF = _lib.HB_FLAG_NO_LIVE_FIRST


def _expand(plan, row, n_pad):
    out = []
    for s in plan["src"][int(plan["row_ptr"][row]):int(plan["row_ptr"][row + 1])]:
        out.extend(_expand(plan, int(s), n_pad) if s >= n_pad else [int(s)])
    return out


def _same_plan(a, b):
    return (a["n_pad"] == b["n_pad"] and a["nv"] == b["nv"] and np.array_equal(a["level_begin"], b["level_begin"])
            and np.array_equal(a["order"], b["order"]) and np.array_equal(a["row_ptr"], b["row_ptr"]) and np.array_equal(a["src"], b["src"]))


@pytest.fixture(scope="module")
def graph():
    return synth.RmatGraph(12, 40_000)


@pytest.mark.parametrize("chunk,tune", [(0, ()), (4, ()), (16, ()), (16, (0, 0, 0, 6, 4)), (8, (0, 0, 0, 4, 2))])
def test_live_first_order_and_trees(graph, chunk, tune):
    g = graph
    plan = _lib.host_plan(g.row_ptr, g.src, ON, chunk, tune)
    n, n_pad = g.n, plan["n_pad"]
    indeg = np.diff(g.row_ptr.astype(np.int64))
    outdeg = np.bincount(g.src, minlength=n)
    n_live = int((indeg > 0).sum())
    assert 0 < n_live < n                                                   # the graph has both kinds
    assert plan["live_first"] and plan["n_live"] == n_live and plan["n_live_pad"] == (n_live + 63) // 64 * 64
    order = plan["order"].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n))                         # a permutation
    assert np.all(indeg[order[:n_live]] > 0) and np.all(indeg[order[n_live:]] == 0)  # every live host precedes every dead one
    for part in (order[:n_live], order[n_live:]):
        assert np.all(np.diff(outdeg[part]) <= 0)                           # hottest first inside each part ...
        ties = np.diff(outdeg[part]) == 0
        assert np.all(np.diff(part)[ties] > 0)                              # ... ties by sid
    dev_of = np.zeros(n, np.int64)
    dev_of[order] = np.arange(n)
    rp = plan["row_ptr"].astype(np.int64)
    assert np.diff(rp).max() <= (chunk or 64)
    assert np.all(np.diff(rp)[n_live:n_pad] == 0)                           # a dead row has no list
    lb = plan["level_begin"].astype(np.int64)
    dead_tails = mixed = all_dead = 0
    for row in list(range(n_live)) + list(range(int(lb[0]), int(lb[1]) if len(lb) > 1 else int(lb[0]))):
        s = plan["src"][rp[row]:rp[row + 1]].astype(np.int64)
        if len(s) == 0 or s.min() >= n_pad:
            continue
        assert s.max() < n and np.all(np.diff(s) > 0)                       # real sources, ascending device rows ...
        dead = s >= n_live
        assert not np.any(dead[:-1] & ~dead[1:])                            # ... so the dead ones are the tail of the list
        dead_tails += bool(dead.any())
        mixed += bool(dead.any() and not dead.all())
        all_dead += bool(dead.all())
    assert dead_tails and mixed and all_dead, (dead_tails, mixed, all_dead)
    for d in range(n):
        sid = order[d]
        want = sorted(dev_of[g.src[int(g.row_ptr[sid]):int(g.row_ptr[sid + 1])]].tolist())
        assert sorted(_expand(plan, d, n_pad)) == want                      # the tree covers exactly the row's in-edges


@pytest.mark.parametrize("chunk,tune", [(0, ()), (4, ()), (16, (0, 0, 0, 6, 4))])
def test_forced_off_is_the_plain_out_degree_order(graph, chunk, tune):
    g = graph
    base = _lib.host_plan(g.row_ptr, g.src, 0, chunk, tune)                 # (n < 2^20: off by default)
    assert not base["live_first"] and base["n_live_pad"] == base["n_pad"]
    assert base["n_live"] == int((np.diff(g.row_ptr.astype(np.int64)) > 0).sum())
    outdeg = np.bincount(g.src, minlength=g.n)
    assert np.array_equal(base["order"], np.lexsort((np.arange(g.n), -outdeg.astype(np.int64))))  # descending out-degree, ties by sid
    for flags in (OFF, ON | OFF):
        got = _lib.host_plan(g.row_ptr, g.src, flags, chunk, tune)
        assert _same_plan(got, base) and not got["live_first"], flags
    on = _lib.host_plan(g.row_ptr, g.src, ON, chunk, tune)
    assert not np.array_equal(on["order"], base["order"])


@pytest.mark.parametrize("flags,tune", [(_lib.HB_FLAG_NO_REORDER, ()), (_lib.HB_FLAG_PASS_STATS, ()), (_lib.HB_FLAG_UNFUSED, ()),
                                        (_lib.HB_FLAG_REFERENCE_TAIL, ()), (0, (0, 0, 0, 0, 0, 0, 0, 2)), (0, (0, 0, 0, 0, 0, 0, 0, 3))])
def test_plans_that_ignore_the_option(graph, flags, tune):
    """no reorder, counting passes, unfused passes, owner slices (tune[7] = world): the plan is the one without the flag"""
    g = graph
    base = _lib.host_plan(g.row_ptr, g.src, flags, 16, tune)
    got = _lib.host_plan(g.row_ptr, g.src, flags | ON, 16, tune)
    assert _same_plan(got, base) and not got["live_first"] and got["n_live_pad"] == got["n_pad"]


THRESHOLD = 1 << 20  # live_first_by_flags (hb_api.hip): on by itself from this many hosts


def _ring_with_dead(n_dead, ring=THRESHOLD - 2):
    """a ring of `ring` hosts and n_dead hosts without an in-edge that link to ring host 0, as (row_ptr, src)"""
    deg = np.ones(ring + n_dead, dtype=np.uint64)
    deg[0], deg[ring:] = 1 + n_dead, 0
    row_ptr = np.concatenate(([0], np.cumsum(deg))).astype(np.uint64)
    src = np.concatenate(([ring - 1], np.arange(ring, ring + n_dead), np.arange(ring - 1))).astype(np.uint32)
    return row_ptr, src


def test_the_size_gate_and_the_flags_that_close_it():
    """Without either flag the order is on from 2^20 hosts and off one host below; NO_LIVE_FIRST, NO_REORDER, UNFUSED, PASS_STATS,
    REFERENCE_TAIL and DEST_PARTITION keep it off at 2^20; LIVE_FIRST turns it on below."""
    below, at = _ring_with_dead(1), _ring_with_dead(2)
    assert len(below[0]) - 1 == THRESHOLD - 1 and len(at[0]) - 1 == THRESHOLD
    assert _lib.host_plan_live(*below) == (False, THRESHOLD - 2, THRESHOLD)       # off: n_live_pad = n_pad
    assert _lib.host_plan_live(*at) == (True, THRESHOLD - 2, THRESHOLD)           # on: n_live rounded up to a tile (here n_pad as well)
    assert _lib.host_plan_live(*below, ON) == (True, THRESHOLD - 2, THRESHOLD)
    for name in ("NO_LIVE_FIRST", "NO_REORDER", "UNFUSED", "PASS_STATS", "REFERENCE_TAIL", "DEST_PARTITION"):
        flag = getattr(_lib, "HB_FLAG_" + name)
        assert _lib.host_plan_live(*at, flag)[0] is False, name
        assert _lib.host_plan_live(*at, flag | ON)[0] is False, name
    # the order itself at that size: the two dead hosts lie behind every ring host
    order = _lib.host_plan(*at)["order"]
    assert sorted(order[-2:].tolist()) == [THRESHOLD - 2, THRESHOLD - 1]


def test_graphs_without_dead_or_without_live_hosts():
    ring = np.arange(100, dtype=np.uint32)
    rp = np.arange(101, dtype=np.uint64)
    plan = _lib.host_plan(rp, np.roll(ring, 1), ON, 4)                      # a ring: nobody is dead
    assert plan["live_first"] and plan["n_live"] == 100 and plan["n_live_pad"] == plan["n_pad"] == 128
    assert np.array_equal(plan["order"], _lib.host_plan(rp, np.roll(ring, 1), 0, 4)["order"])
    plan = _lib.host_plan(np.zeros(51, dtype=np.uint64), np.zeros(0, dtype=np.uint32), ON, 4)  # no edge: everybody is
    assert plan["live_first"] and plan["n_live"] == 0 and plan["n_live_pad"] == 0 and np.array_equal(plan["order"], np.arange(50))
    plan = _lib.host_plan(np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), ON, 4)   # no node
    assert plan["n_live"] == 0 and plan["n_live_pad"] == 0 and plan["n_pad"] == 0
