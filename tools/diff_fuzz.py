#!/usr/bin/env python3
"""Differential fuzzing of the pass driver against the oracle: random small graphs of several shapes x random layout / mode knobs,
compared after EVERY pass (registers, Kahan words, cached sizes, changed count, pass count) and at the end (final list).
Runs against whatever library HB_LIB_PATH names: the gfx950 library on a GPU box, or - on a machine without a GPU - the
interpreted test build of the device sources (tests/simt, with HB_ALLOW_SIMT_INTERPRETER=1; add the AddressSanitizer preload
for the `make asan` build).  A failure prints the seed and case that reproduce it and makes the exit code non-zero.

--ids extreme relabels a random 10 to 50 % of each case's nodes (passes, ranks, records) with ids whose hash sets a chosen register to a chosen
value, weighted towards 40..58 and 65 (tests/graphs.py crafted_id_low): the estimator's sequential fold, saturated sizes and the six-bit
wire codes above 47, which ids 1..n never reach; mixed alternates between plain and extreme.

The operator modes (distances ... sampled; `operators` alternates over all nine) run the bodies of tests/operator_cases.py, each against the
CPU restatement of its operator, on contexts of that module's layout recipe: chunk 4 / 8 / 16 / 64, tune[3..5] (band width, minimum
sources before a band cut, largest row that is not split) and two of NO_REORDER / NO_XCD_MAP / HOST_PLAN / NO_SPARSE.

--order decides the device order of the passes, records and operator contexts: plain draws nothing and replays the
cases this tool drew before it knew the option; live puts HB_FLAG_LIVE_FIRST on every context - the order every graph of 2^20 hosts and
more is planned in; mixed (the default) draws one of nothing / HB_FLAG_LIVE_FIRST / HB_FLAG_NO_LIVE_FIRST per case.  Under live and mixed
the graphs also include `dead_fringe`, and every loaded context's plan_live() is held against the host planner's on the same graph and flags;
one case in three of them also runs with HB_FLAG_NO_SATURATION (the dense passes gather for saturated rows as well),
and every case draws one of nothing / HB_FLAG_FORCE_EARLY_EXIT / HB_FLAG_NO_EARLY_EXIT (a dense row leaves its gather
loop once its accumulator has reached U - under the default rule, from pass 1 on, never).

--mode ampc drives the AMPC shard (stract_amd/ampc.py) instead of a context: every case is one sequence of tests/ampc_model.py - 60 to 240
interleaved calls on tables, graphs and filters that stay alive, each answer against the model, the whole content of every table and
filter after every eighth call.  A failure prints the case's seed, the operation index and the operations so far.

--mode context drives ONE context through interleaved calls of every call family (tests/context_model.py): every case
draws a sequence seed, a context (nothing / NO_SPARSE / LIVE_FIRST, chunk 0 / 4 / 8 / 16 / 64) and a length of 40 to 160 operations - hb_run,
hb_begin .. hb_finish, the ten operators with changing arguments, loads of other graphs, hb_release_cached_memory, refusals -, each answer
as the operator's suite compares it, every reader of every operator after every sixth call.  A failure prints as in --mode ampc.

usage: tools/diff_fuzz.py [--mode passes|records|tail|ranks|mixed|operators|ampc|context|distances|betweenness|similarity|nearest_seed|score_hosts|backlinks|forwardlinks|similar_hosts|sampled]
                          [--ids plain|extreme|mixed] [--order plain|live|mixed] [--seconds S] [--seed N] [--max-nodes N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import hbo  # noqa: E402
from stract_amd import _lib  # noqa: E402
from stract_amd.harmonic import EdgeListGraph  # noqa: E402
from tests import graphs  # noqa: E402
from tests import operator_cases as oc  # noqa: E402

FLAG_POOL = ["NO_REORDER", "NO_XCD_MAP", "UNFUSED", "NO_SPARSE", "NO_FRONTIER", "PASS_STATS", "HOST_PLAN", "NO_INIT_PASS"]


ORDER_FLAGS = {"": 0, "LIVE_FIRST": _lib.HB_FLAG_LIVE_FIRST, "NO_LIVE_FIRST": _lib.HB_FLAG_NO_LIVE_FIRST}


def draw_order(rng, order, what):
    """The device order of one case, a flag for its context: nothing under `plain` (and nothing is drawn), HB_FLAG_LIVE_FIRST under `live`,
    one of the three under `mixed`.  Called behind a case's other draws; recorded in `what` where the option is in use."""
    if order == "plain":
        return 0
    name = "LIVE_FIRST" if order == "live" else ("", "LIVE_FIRST", "NO_LIVE_FIRST")[int(rng.integers(0, 3))]
    what["order"] = name
    # ... and, with it, whether the dense passes skip saturated rows (the default) or gather for every row
    what["saturation"] = bool(rng.integers(0, 3))
    # ... and whether a dense row may leave its gather loop once it has reached U: under the rule of the sum of
    # saturated out-degrees, from pass 1 on, or never
    what["early_exit"] = ("rule", "forced", "off")[int(rng.integers(0, 3))]
    early = {"rule": 0, "forced": _lib.HB_FLAG_FORCE_EARLY_EXIT, "off": _lib.HB_FLAG_NO_EARLY_EXIT}[what["early_exit"]]
    return ORDER_FLAGS[name] | (0 if what["saturation"] else _lib.HB_FLAG_NO_SATURATION) | early


def check_plan_live(ctx, flags, chunk, tune, what):
    """the loaded context's (live-first in use, n_live, n_live_pad) is the host planner's for the same graph, flags and knobs - also
    where the context must ignore the flag (NO_REORDER, UNFUSED, PASS_STATS)"""
    _, row_ptr, src = ctx.graph()
    got, want = ctx.plan_live(), _lib.host_plan_live(row_ptr, src, flags, chunk, tune)
    assert got == want, ("plan_live: context %s, host planner %s" % (got, want), what)
    return got


def big_graph(rng, max_nodes, order="plain"):
    """Shapes the test-suite generator does not reach: hubs above 4096 in-edges (three-level chunk trees at small chunks), many
    isolated / source-only nodes, a heavy-tailed in-degree, long chains hanging off a dense core; where the device order is an option, a
    quarter of the draws is a `dead_fringe` instead (graphs.dead_fringe_graph: n_live = 64 k - 1, 64 k, 64 k + 1 for k = 1 .. 8, n_dead of
    1, 63, 64, 65, 200 - the launches that end at n_live_pad and the dead rows' words behind it)."""
    n = int(rng.integers(2, max_nodes))
    kind = ("heavy_tail", "mega_hub", "core_and_chains")[int(rng.integers(0, 3))]
    if order != "plain" and rng.integers(0, 4) == 0:
        return graphs.dead_fringe_graph(rng)
    e = set()
    if kind == "heavy_tail":
        m = int(rng.integers(n, 8 * n))
        dst = np.minimum((rng.pareto(1.1, m) * 3).astype(np.int64) + 1, n)
        src = rng.integers(1, n + 1, m)
        e = set(zip(src.tolist(), dst.tolist()))
    elif kind == "mega_hub":
        k = int(rng.integers(1, 4))
        for h in range(1, k + 1):
            for s in rng.choice(np.arange(1, n + 1), size=int(rng.integers(n // 2, n)), replace=False).tolist():
                e.add((int(s), h))
        for _ in range(2 * n):
            e.add((int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))))
    else:
        core = max(2, n // 20)
        for a in range(1, core + 1):
            for b in rng.integers(1, core + 1, 8).tolist():
                e.add((a, int(b)))
        at = core + 1
        while at < n:
            length = int(rng.integers(1, 60))
            prev = int(rng.integers(1, core + 1))
            for v in range(at, min(at + length, n + 1)):
                e.add((prev, v))
                prev = v
            at += length
    return kind, sorted((a, b) for a, b in e if a != b)


def crafted_low(rng):
    """Low id half for a random register index and a value weighted towards 40..58 and 65."""
    u = rng.random()
    value = 65 if u < 0.2 else int(rng.integers(40, 59)) if u < 0.7 else int(rng.integers(1, 59))
    return graphs.crafted_id_low(int(rng.integers(0, 64)), value, int(rng.integers(0, 1 << 62)))


def relabel_extreme(rng, edges):
    """The same graph with a random 10 to 50 % of its nodes under crafted ids; the high half tells apart ids whose low halves collide."""
    nodes = sorted({x for e in edges for x in e})
    picked = rng.choice(len(nodes), max(1, int(len(nodes) * rng.uniform(0.1, 0.5))), replace=False).tolist()
    new, used = {}, set(nodes)
    for k in picked:
        low = crafted_low(rng)
        new[nodes[k]] = low if low not in used else ((nodes[k] + 1) << 64) | low
        used.add(low)
    assert len(set(new.values())) == len(new)
    return sorted((new.get(a, a), new.get(b, b)) for a, b in edges)


def one_case(rng, max_nodes, case, extreme=False, order="plain"):
    if rng.random() < 0.5:
        kind, edges = graphs.random_graph(rng)
    else:
        kind, edges = big_graph(rng, max_nodes, order)
    if not edges:
        return None
    if extreme:
        edges = relabel_extreme(rng, edges)
    ids, row_ptr, src = graphs.dense_from_tuples(edges)
    chunk = int(rng.choice([4, 8, 16, 32, 64, 128, 256]))
    # (tune[1] above its low byte: switches of the experiments build, stract_amd/csrc/hb_experiments.h)
    tune = (int(rng.choice([0, 0, 1, 2, 7])), int(rng.choice([0, 1, 2, 4])) | int(rng.choice([0, 0, _lib.HB_X_TILE_EPILOGUE, _lib.HB_X_SEED_3LAUNCH, _lib.HB_X_BITMAP_SLOTWISE])) | int(rng.choice([0, 0, _lib.HB_X_SNAPSHOT_EVERY_PASS, _lib.HB_X_SNAPSHOT_EVERY_PASS | _lib.HB_X_ONE_SNAPSHOT, _lib.HB_X_SNAPSHOT_EVERY_PASS | _lib.HB_X_SHORT_FINAL_LIST | _lib.HB_X_ONE_SNAPSHOT])) | int(rng.choice([0, 0, _lib.HB_X_TAIL_KERNEL, _lib.HB_X_TAIL_KERNEL_ANY])) | int(rng.choice([0, 0, _lib.HB_X_FULL_INIT])) | int(rng.choice([0, 0, _lib.HB_X_SCATTER_TRANSPOSE])),  # (+ the single-workgroup tail kernel: on / on after any pass; round 6: full init, transposition by scatter)
            int(rng.choice([0, 0, 30, 101])),
            int(rng.integers(4, 17)), int(rng.integers(1, 9)), int(rng.integers(0, chunk + 1)), int(rng.choice([0, 0, 1, 4, 1000000])))
    names = sorted(set(rng.choice(FLAG_POOL, size=int(rng.integers(0, 3))).tolist()))
    flags = 0
    for nm in names:
        flags |= getattr(_lib, "HB_FLAG_" + nm)
    what = dict(case=case, kind=kind, n=int(len(ids)), m=int(len(src)), chunk=chunk, tune=tune, flags=names, extreme_ids=extreme)
    flags |= draw_order(rng, order, what)
    o = hbo.Dense(ids["lo"].copy(), row_ptr, src)
    with _lib.Context(flags=flags, chunk=chunk, tune=tune) as ctx:
        ctx.load_dense(ids, row_ptr, src)
        check_plan_live(ctx, flags, chunk, tune, what)
        ctx.begin()
        assert np.array_equal(ctx.registers(), o.registers()), ("initial registers", what)
        has, t = True, 0
        while has:
            has = ctx.step()
            ohas, ost = o.step(hbo.FRONTIER)
            assert has == ohas, ("has_changes after pass %d" % t, what)
            assert np.array_equal(ctx.registers(), o.registers()), ("registers after pass %d" % t, what)
            s, e = ctx.kahan()
            os_, oe = o.kahan()
            assert np.array_equal(s.view(np.uint64), os_.view(np.uint64)) and np.array_equal(e.view(np.uint64), oe.view(np.uint64)), ("Kahan words after pass %d" % t, what)
            assert np.array_equal(ctx.sizes(), o.sizes()), ("sizes after pass %d" % t, what)
            ps = ctx.pass_stats()[t]
            assert ps["changed"] == ost["changed"], ("changed count of pass %d" % t, what)
            # A_t where the suite compares it (tests/test_gpu.py): counted edge by edge in a bitmap pass under PASS_STATS, the out-degree
            # sum of the hosts that changed in pass t - 1 otherwise - a dead row wrongly left "changed" shows here first
            if not flags & _lib.HB_FLAG_PASS_STATS or ps["mode"] == 1:
                assert ps["active_edges"] == ost["active_edges"], ("active edges of pass %d" % t, what)
            t += 1
        ctx.finish()
        vals, keep, k = o.finish()
        gids, gvals = ctx.results()
        assert len(gvals) == k and np.array_equal(gids, ids[keep]) and np.array_equal(gvals.view(np.uint64), vals[keep].view(np.uint64)), ("final list", what)
    what["passes"] = t
    return what


SKIPPED_BITS = [8, 10, 11, 13, 14, 15, 16, 17, 18, 19, 21, 22]  # HB_SKIPPED_REL_MASK = 0x6FED00
HARMLESS_BITS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 20]


def records_case(rng, max_nodes, case, extreme=False, order="plain"):
    """The record boundary: a random stream of SmallEdge records - 128-bit ids (equal low halves, different high halves among them),
    duplicates of a pair with other flags before and after it, skipped and harmless rel flags, self links - handed over in random
    batches (hb_append_edges ... hb_finalize, the device ingest: hash table of provisional ids, one stable sort) or at once, with and
    without an explicit node list; node / edge counts, pass count and the final list against the faithful (map-based) oracle."""
    n = int(rng.integers(2, max(3, max_nodes // 4)))
    m = int(rng.integers(1, 6 * n))
    pool_lo = rng.integers(1, 1 << 62, n, dtype=np.uint64)
    pool_hi = rng.integers(0, 3, n, dtype=np.uint64) if rng.random() < 0.5 else rng.integers(0, 1 << 63, n, dtype=np.uint64)
    if rng.random() < 0.3:
        pool_lo[: n // 2] = pool_lo[n // 2: n // 2 + n // 2]  # same low half, told apart only by the high half
    if extreme:
        used = set(pool_lo.tolist())
        for k in rng.choice(n, max(1, int(n * rng.uniform(0.1, 0.5))), replace=False).tolist():
            low = crafted_low(rng)
            pool_lo[k] = low
            if low in used:
                pool_hi[k] = (1 << 40) + k
            used.add(low)
    e = np.zeros(m, dtype=_lib.EDGE)
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    if rng.random() < 0.5:  # a hub destination
        b[rng.random(m) < 0.3] = 0
    e["from"]["lo"], e["from"]["hi"], e["to"]["lo"], e["to"]["hi"] = pool_lo[a], pool_hi[a], pool_lo[b], pool_hi[b]
    flags = np.zeros(m, dtype=np.uint64)
    for k in np.nonzero(rng.random(m) < 0.25)[0]:
        bits = SKIPPED_BITS if rng.random() < 0.6 else HARMLESS_BITS
        flags[k] = np.uint64(1) << np.uint64(int(rng.choice(bits)))
    e["rel_flags"] = flags
    dup = np.nonzero(rng.random(m) < 0.2)[0]  # repeat some records elsewhere in the stream with other flags
    if len(dup):
        extra = e[dup].copy()
        extra["rel_flags"] = np.where(rng.random(len(dup)) < 0.5, np.uint64(0), np.uint64(1) << np.uint64(13))
        e = np.concatenate([e, extra])
        e = e[rng.permutation(len(e))]
    fids, fvals, fst = hbo.faithful_run(e)
    how = int(rng.integers(0, 3))
    what = dict(case=case, kind="records", records=int(len(e)), pool=n, how=("batches", "at once", "at once + node list")[how], extreme_ids=extreme)
    flags_ctx = int(rng.choice([0, 0, _lib.HB_FLAG_HOST_INGEST, _lib.HB_FLAG_HOST_PLAN]))
    # hb_run: the tail pipeline (default) or one pass at a time (HB_X_NO_TAIL_PIPELINE), results in snapshots (HB_X_SNAPSHOT_EVERY_PASS) or at the end
    tune_ctx = (0, int(rng.choice([0, 0, _lib.HB_X_SNAPSHOT_EVERY_PASS, _lib.HB_X_NO_TAIL_PIPELINE, _lib.HB_X_SNAPSHOT_EVERY_PASS | _lib.HB_X_SHORT_FINAL_LIST | _lib.HB_X_ONE_SNAPSHOT, _lib.HB_X_SNAPSHOT_EVERY_PASS | _lib.HB_X_NO_TAIL_PIPELINE])) | int(rng.choice([0, 0, _lib.HB_X_TAIL_KERNEL, _lib.HB_X_TAIL_KERNEL_ANY])), int(rng.choice([0, 0, 101])), 0, 0, 0,
                int(rng.choice([0, 0, 1])))
    what["tune"] = tune_ctx
    chunk_ctx = int(rng.choice([8, 64]))
    flags_ctx |= draw_order(rng, order, what)
    lonely = np.zeros(0, dtype=_lib.U128)
    if order != "plain" and how == 2:
        # hosts the node list names and no record mentions: neither an in- nor an out-link.  The faithful oracle, which takes its hosts
        # from the records, is told of them by records under a skipped flag; the context is not handed those
        lonely = np.zeros(int(rng.integers(2, 6)), dtype=_lib.U128)
        lonely["lo"], lonely["hi"] = np.arange(len(lonely), dtype=np.uint64) + np.uint64(1), np.uint64(1 << 63) + np.uint64(7)
        told = np.zeros(len(lonely), dtype=_lib.EDGE)
        told["from"], told["to"], told["rel_flags"] = lonely, np.roll(lonely, 1), np.uint64(1) << np.uint64(SKIPPED_BITS[0])
        fids, fvals, fst = hbo.faithful_run(np.concatenate([e, told]))
        fst = dict(fst, m_unique=fst["m_unique"] - len(lonely))  # (the pairs of those records)
        what["lonely_hosts"] = int(len(lonely))
    with _lib.Context(flags=flags_ctx, chunk=chunk_ctx, tune=tune_ctx) as ctx:
        if how == 0:
            cuts = np.sort(rng.integers(0, len(e) + 1, int(rng.integers(0, 6))))
            for part in np.split(e, cuts):
                ctx.append_edges(part)
            ctx.finalize()
        elif how == 1:
            ctx.load_edges(e)
        else:
            nodes = np.unique(np.concatenate([e["from"], e["to"], lonely]))
            ctx.load_edges(e, nodes)
        if order != "plain":
            check_plan_live(ctx, flags_ctx, chunk_ctx, tune_ctx, what)
        st = ctx.run()
        ids, vals = ctx.results()
    assert (st["n"], st["m_unique"], st["m_eff"], st["passes"]) == (fst["n"], fst["m_unique"], fst["m_eff"], fst["passes"]), ("counts", what, st, fst)
    assert np.array_equal(ids, fids) and np.array_equal(vals.view(np.uint64), fvals.view(np.uint64)), ("final list", what)
    what.update(m=int(fst["m_eff"]), passes=int(fst["passes"]))
    return what


def tail_case(rng, case):
    """HB_FLAG_REFERENCE_TAIL: the reference's changed-node machinery as written (bloom filter, exact-counting switch, sqrt(n) tail over
    page-level records replayed through the query's per-segment LinksScorer) on random tailed graphs (a core feeding a chain with side
    branches, so that 0 < |changed| <= sqrt(n) happens), with a random share of the host links present at page level, duplicates of
    documents under conflicting flags, foreign page ids, and random segment cuts; ids, values, pass count and the NUMBER OF TAIL PASSES
    against the faithful oracle given the same records."""
    core = int(rng.integers(20, 400))
    host = graphs.tailed_graph(core=core, core_edges=int(rng.integers(core, min(2000, core * (core - 1) // 3))), chain=int(rng.integers(5, 160)),
                               seed=int(rng.integers(1, 1 << 30)), branch=int(rng.integers(0, 5)))
    e = EdgeListGraph.from_tuples(host).host_edges()
    keep = rng.random(len(host)) < rng.choice([0.0, 0.3, 0.7, 1.0])
    pages = [host[i] for i in np.nonzero(keep)[0].tolist()]
    for i in np.nonzero(rng.random(len(host)) < 0.1)[0].tolist():  # duplicates of a document, some flagged, placed somewhere else
        f, t, _ = host[i]
        pages.insert(int(rng.integers(0, len(pages) + 1)), (f, t, int(rng.choice([0, graphs.NOFOLLOW, graphs.TAG]))))
    for k in range(int(rng.integers(0, 6))):  # documents whose endpoints are not hosts of the graph
        pages.append((0xDEAD0000 + k, host[int(rng.integers(0, len(host)))][1], 0))
    recs = EdgeListGraph.from_tuples(pages).host_edges() if pages else np.zeros(0, dtype=_lib.EDGE)
    cuts = sorted(set(int(x) for x in rng.integers(0, len(recs) + 1, int(rng.integers(0, 4)))) | {0, len(recs)})
    segs = [b - a for a, b in zip(cuts, cuts[1:])] or [0]
    fids, fvals, fst = hbo.faithful_run(e, recs, segs)
    what = dict(case=case, kind="tail", hosts=int(fst["n"]), host_edges=int(len(e)), page_records=int(len(recs)), segments=segs)
    with _lib.Context(flags=_lib.HB_FLAG_REFERENCE_TAIL | int(rng.choice([0, _lib.HB_FLAG_HOST_PLAN]))) as ctx:
        ctx.load_edges(e)
        at = 0
        for length in segs:
            for part in np.array_split(recs[at:at + length], int(rng.integers(1, 4))):
                ctx.append_tail_edges(part)
            ctx.tail_segment_end()
            at += length
        st = ctx.run()
        ids, vals = ctx.results()
        modes = [ps["mode"] for ps in ctx.pass_stats()]
    assert st["passes"] == fst["passes"] and modes.count(3) == fst["passes_exact"], ("pass / tail-pass count", what, modes, fst)
    assert np.array_equal(ids, fids) and np.array_equal(vals.view(np.uint64), fvals.view(np.uint64)), ("final list", what)
    what.update(m=int(len(e)), passes=int(fst["passes"]), tail_passes=int(fst["passes_exact"]))
    return what


def ranks_case(rng, max_nodes, case, extreme=False):
    """The multi-rank decompositions with R = 2..5 LOGICAL ranks on one device (the collective emulated by hb_debug_exchange): edge
    partition (all-reduce(max)), its changed-only form, destination partition (all-gather of the owned slices), its changed-only form;
    random graphs and layout knobs; after every pass all ranks must hold the oracle's registers, at the end the oracle's final list."""
    from stract_amd import dist
    kind, edges = graphs.random_graph(rng) if rng.random() < 0.5 else big_graph(rng, max(200, max_nodes // 3))
    if not edges:
        return None
    if extreme:
        edges = relabel_extreme(rng, edges)
    ids, row_ptr, src = graphs.dense_from_tuples(edges)
    world = int(rng.integers(2, 6))
    mode = str(rng.choice(["edge", "edge_changed", "dest", "dest_changed"]))
    flags = _lib.HB_FLAG_NO_RCCL | (_lib.HB_FLAG_DEST_PARTITION if mode.startswith("dest") else 0) | (_lib.HB_FLAG_CHANGED_ONLY if mode.endswith("_changed") else 0)
    chunk = int(rng.choice([8, 16, 64]))
    tune = (0, 0, int(rng.choice([0, 101])), int(rng.integers(4, 9)), int(rng.integers(1, 9)))
    what = dict(case=case, kind="ranks:" + kind, n=int(len(ids)), m=int(len(src)), world=world, mode=mode, chunk=chunk, tune=tune, extreme_ids=extreme)
    o = hbo.Dense(ids["lo"].copy(), row_ptr, src)
    split = dist.partition_dense_by_dest if mode.startswith("dest") else dist.partition_dense
    ctxs = []
    try:
        for r in range(world):
            c = _lib.Context(rank=r, world_size=world, flags=flags, chunk=chunk, tune=tune)
            ctxs.append(c)
            rp, sr = split(row_ptr, src, r, world)
            c.load_dense(ids, rp, sr)
            c.begin()
        has, t = True, 0
        while has:
            for c in ctxs:
                c.step_local()
            _lib.Context.exchange(ctxs, 0)
            out = [c.step_finish() for c in ctxs]
            ohas, _ = o.step(hbo.FRONTIER)
            assert len(set(out)) == 1 and out[0] == ohas, ("has_changes after pass %d" % t, what)
            has = out[0]
            want = o.registers()
            for r, c in enumerate(ctxs):
                assert np.array_equal(c.registers(), want), ("registers of rank %d after pass %d" % (r, t), what)
            t += 1
        _lib.Context.exchange(ctxs, 1)
        vals, keep, k = o.finish()
        for r, c in enumerate(ctxs):
            c.finish()
            gids, gvals = c.results()
            assert len(gvals) == k and np.array_equal(gids, ids[keep]) and np.array_equal(gvals.view(np.uint64), vals[keep].view(np.uint64)), ("final list of rank %d" % r, what)
    finally:
        for c in ctxs:
            c.close()
    what["passes"] = t
    return what


OPERATOR_MODES = ["distances", "betweenness", "similarity", "nearest_seed", "score_hosts", "backlinks", "forwardlinks", "similar_hosts", "sampled"]


def operator_case(rng, case, name, order="plain"):
    """One context of the layout recipe of tests/operator_cases.py - a graph of graphs.random_graph with self links, chunk 4 / 8 / 16 /
    64, the planner's cut and split knobs tune[3..5], two layout flags - and on it the body of operator `name`, the one the suite runs
    (tests/test_layouts.py), against the CPU restatement of that operator.  The hubs of the plan's chunk trees and sources inside them
    are among the body's queries."""
    kind, tuples = oc.draw_graph(rng)
    chunk, tune, flags = oc.draw_layout(rng)
    what = dict(case=case, kind=name + ":" + kind, chunk=chunk, tune=tune, flags=flags)
    flags |= draw_order(rng, order, what)
    with oc.load(_lib.Context, tuples, chunk, tune, flags) as ctx:
        graph = ctx.graph()
        live = check_plan_live(ctx, flags, chunk, tune, what) if order != "plain" else (False, 0, 0)
        # (on a live-first plan a live and a dead member of a hub's chunk are among the picks: a dead host is queried, walked from and scored)
        picks = oc.picks_of(oc.layout_conditions(ctx.plan(), graph[1], chunk, live[1] if live[0] else None))
        passes = oc.BODIES[name](ctx, graph, rng, what, picks)
    what.update(n=int(len(graph[0])), m=int(len(graph[2])), passes=int(passes))
    return what


def ampc_case(rng, case):
    """one sequence of tests/ampc_model.py under a drawn seed and length, every call on the library and on the model"""
    from tests import ampc_model
    seed, n_ops = int(rng.integers(1, 1 << 31)), int(rng.integers(60, 241))
    handles, log = ampc_model.Handles(), []
    try:
        world = ampc_model.run(seed, handles, n_ops, log)
    finally:
        handles.close()
    return dict(case=case, kind="ampc", sequence_seed=seed, operations=n_ops, m=int(world.counts["largest_table"]), passes=len(log))


def ampc_main(a):
    """--mode ampc: `passes_compared` counts the operations compared, `edges` adds up the largest table of every case"""
    from stract_amd import ampc
    from tests import ampc_model
    assert ampc.wave_group_length() == ampc_model.WAVE_GROUP
    rng = np.random.default_rng(a.seed)
    t0, done, keys, ops = time.time(), 0, 0, 0
    while time.time() - t0 < a.seconds:
        try:
            w = ampc_case(rng, done)
        except AssertionError as e:
            print(json.dumps({"failed": str(e.args[0] if e.args else e), "seed": a.seed, "cases_before": done}))
            sys.exit(1)
        done, keys, ops = done + 1, keys + w["m"], ops + w["passes"]
    print(json.dumps({"library": _lib.LIB_PATH, "mode": a.mode, "seed": a.seed, "seconds": round(time.time() - t0, 1), "cases": done, "largest_tables": keys, "operations_compared": ops, "failed": None}))


def context_case(rng, case):
    """one sequence of tests/context_model.py under a drawn seed, context and length, every call on the library and on the model"""
    from tests import context_model
    seed, n_ops = int(rng.integers(1, 1 << 31)), int(rng.integers(40, 161))
    variant = ("drawn", [(), ("NO_SPARSE",), ("LIVE_FIRST",)][int(rng.integers(0, 3))], int(rng.choice((0,) + oc.CHUNKS)))
    log = []
    world = context_model.run(seed, _lib.Context, n_ops, log, variant)
    return dict(case=case, kind="context", sequence_seed=seed, flags=list(variant[1]), chunk=variant[2], operations=n_ops, m=int(world.counts["loads"]), passes=len(log))


def context_main(a):
    """--mode context: `passes_compared` counts the operations compared, `edges` the graphs loaded"""
    rng = np.random.default_rng(a.seed)
    t0, done, loads, ops = time.time(), 0, 0, 0
    while time.time() - t0 < a.seconds:
        try:
            w = context_case(rng, done)
        except AssertionError as e:
            print(json.dumps({"failed": str(e.args[0] if e.args else e), "seed": a.seed, "cases_before": done}))
            sys.exit(1)
        done, loads, ops = done + 1, loads + w["m"], ops + w["passes"]
    print(json.dumps({"library": _lib.LIB_PATH, "mode": a.mode, "seed": a.seed, "seconds": round(time.time() - t0, 1), "cases": done, "graphs_loaded": loads, "operations_compared": ops, "failed": None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["passes", "records", "tail", "ranks", "mixed", "operators", "ampc", "context"] + OPERATOR_MODES, default="passes")
    ap.add_argument("--ids", choices=["plain", "extreme", "mixed"], default="plain")
    ap.add_argument("--order", choices=["plain", "live", "mixed"], default="mixed")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-nodes", type=int, default=6000)
    a = ap.parse_args()
    if a.mode == "ampc":
        return ampc_main(a)
    if a.mode == "context":
        return context_main(a)
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    done, edges, passes = 0, 0, 0
    case = 0
    while time.time() - t0 < a.seconds:
        extreme = a.ids == "extreme" or (a.ids == "mixed" and case % 2 == 1)
        try:
            if a.mode in OPERATOR_MODES:
                w = operator_case(rng, case, a.mode, a.order)
            elif a.mode == "operators":
                w = operator_case(rng, case, OPERATOR_MODES[case % len(OPERATOR_MODES)], a.order)
            elif a.mode == "ranks" or (a.mode == "mixed" and case % 6 == 4):
                w = ranks_case(rng, a.max_nodes, case, extreme)
            elif a.mode == "tail" or (a.mode == "mixed" and case % 6 == 5):
                w = tail_case(rng, case)
            elif a.mode == "records" or (a.mode == "mixed" and case % 3 == 2):
                w = records_case(rng, a.max_nodes, case, extreme, a.order)
            else:
                w = one_case(rng, a.max_nodes, case, extreme, a.order)
        except AssertionError as e:
            print(json.dumps({"failed": str(e.args[0] if e.args else e), "seed": a.seed, "cases_before": done}))
            sys.exit(1)
        case += 1
        if w:
            done += 1
            edges += w["m"]
            passes += w["passes"]
    print(json.dumps({"library": _lib.LIB_PATH, "mode": a.mode, "ids": a.ids, "order": a.order, "seed": a.seed, "seconds": round(time.time() - t0, 1), "cases": done, "edges": edges, "passes_compared": passes, "failed": None}))


if __name__ == "__main__":
    main()
