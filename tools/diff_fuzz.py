#!/usr/bin/env python3
"""Differential fuzzing of the pass driver against the oracle: random small graphs of several shapes x random layout / mode knobs,
compared after EVERY pass (registers, Kahan words, cached sizes, changed count, pass count) and at the end (final list).
Runs against whatever library HB_LIB_PATH names: the gfx950 library on a GPU box, or - on a machine without a GPU - the
interpreted test build of the device sources (tests/simt, with HB_ALLOW_SIMT_INTERPRETER=1; add the AddressSanitizer preload
for the `make asan` build).  A failure prints the seed and case that reproduce it and makes the exit code non-zero.

--ids extreme relabels a random 10 to 50 % of each case's nodes (passes, ranks, records) with ids whose hash sets a chosen register to a chosen
value, weighted towards 40..58 and 65 (tests/graphs.py crafted_id_low): the estimator's sequential fold, saturated sizes and the six-bit
wire codes above 47, which ids 1..n never reach; mixed alternates between plain and extreme.

usage: tools/diff_fuzz.py [--mode passes|records|tail|ranks|mixed|distances|betweenness|similarity|nearest_seed|score_hosts] [--ids plain|extreme|mixed] [--seconds S] [--seed N] [--max-nodes N]"""
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

FLAG_POOL = ["NO_REORDER", "NO_XCD_MAP", "UNFUSED", "NO_SPARSE", "NO_FRONTIER", "PASS_STATS", "HOST_PLAN", "NO_INIT_PASS"]


def big_graph(rng, max_nodes):
    """Shapes the test-suite generator does not reach: hubs above 4096 in-edges (three-level chunk trees at small chunks), many
    isolated / source-only nodes, a heavy-tailed in-degree, long chains hanging off a dense core."""
    n = int(rng.integers(2, max_nodes))
    kind = ("heavy_tail", "mega_hub", "core_and_chains")[int(rng.integers(0, 3))]
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


def one_case(rng, max_nodes, case, extreme=False):
    if rng.random() < 0.5:
        kind, edges = graphs.random_graph(rng)
    else:
        kind, edges = big_graph(rng, max_nodes)
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
    o = hbo.Dense(ids["lo"].copy(), row_ptr, src)
    with _lib.Context(flags=flags, chunk=chunk, tune=tune) as ctx:
        ctx.load_dense(ids, row_ptr, src)
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
            assert ctx.pass_stats()[t]["changed"] == ost["changed"], ("changed count of pass %d" % t, what)
            t += 1
        ctx.finish()
        vals, keep, k = o.finish()
        gids, gvals = ctx.results()
        assert len(gvals) == k and np.array_equal(gids, ids[keep]) and np.array_equal(gvals.view(np.uint64), vals[keep].view(np.uint64)), ("final list", what)
    what["passes"] = t
    return what


SKIPPED_BITS = [8, 10, 11, 13, 14, 15, 16, 17, 18, 19, 21, 22]  # HB_SKIPPED_REL_MASK = 0x6FED00
HARMLESS_BITS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 20]


def records_case(rng, max_nodes, case, extreme=False):
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
    with _lib.Context(flags=flags_ctx, chunk=int(rng.choice([8, 64])), tune=tune_ctx) as ctx:
        if how == 0:
            cuts = np.sort(rng.integers(0, len(e) + 1, int(rng.integers(0, 6))))
            for part in np.split(e, cuts):
                ctx.append_edges(part)
            ctx.finalize()
        elif how == 1:
            ctx.load_edges(e)
        else:
            nodes = np.unique(np.concatenate([e["from"], e["to"]]))
            ctx.load_edges(e, nodes)
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


def distances_case(rng, max_nodes, case):
    """hb_distances: random graph x random source set x direction x max_dist x forced step, against the host restatement
    (tests/distance_ref.py: the literal dijkstra_multi with the u8 rule)."""
    from stract_amd.harmonic import EdgeListGraph
    from tests import distance_ref as dref
    kind, tuples = graphs.random_graph(rng)
    if not tuples:
        return None
    chunk = int(rng.choice([0, 0, 4, 8, 64]))
    flags = _lib.HB_FLAG_ALL_RELS | int(rng.choice([0, 0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP, _lib.HB_FLAG_NO_SPARSE]))
    with _lib.Context(flags=flags, chunk=chunk) as ctx:
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        ids, row_ptr, src = ctx.graph()
        n = len(ids)
        what = dict(case=case, kind="distances:" + kind, n=n, m=int(len(src)), chunk=chunk, flags=flags, passes=0)
        for _ in range(4):
            srcs = sorted(set(int(x) for x in rng.integers(0, n, int(rng.integers(1, 5)))))
            rev = bool(rng.integers(0, 2))
            md = [None, 0, 1, 7, 15, 200][int(rng.integers(0, 6))]
            mode = [None, "top_down", "bottom_up"][int(rng.integers(0, 3))]
            want = dref.dijkstra(n, row_ptr, src, srcs, reversed=rev, max_dist=md)
            gids, gdist, st = ctx.distances(ids[np.asarray(srcs, dtype=np.int64)], reversed=rev, max_dist=md, mode=mode)
            keep = want != dref.UNREACHED
            run = dict(what, sources=srcs, reversed=rev, max_dist=md, mode=mode)
            assert np.array_equal(gids, ids[keep]) and np.array_equal(gdist, want[keep]), ("distance list", run)
            assert np.array_equal(ctx.distance_all(), want) and st["reached"] == int(keep.sum()) == sum(st["frontier"]), ("distance array / counters", run)
            what["passes"] += st["levels"]
    return what


def betweenness_case(rng, max_nodes, case):
    """hb_betweenness: random graph x random source set x forced mode, against the host restatement (tests/betweenness_ref.py: the
    literal betweenness.rs:50-122) under the comparison rule of tests/test_betweenness.py."""
    from stract_amd.harmonic import EdgeListGraph
    from tests import betweenness_ref as bref
    kind, tuples = graphs.random_graph(rng)
    if not tuples:
        return None
    chunk = int(rng.choice([0, 0, 4, 8, 64]))
    flags = _lib.HB_FLAG_ALL_RELS | int(rng.choice([0, 0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP, _lib.HB_FLAG_NO_SPARSE]))
    with _lib.Context(flags=flags, chunk=chunk) as ctx:
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        ids, row_ptr, src = ctx.graph()
        n = len(ids)
        what = dict(case=case, kind="betweenness:" + kind, n=n, m=int(len(src)), chunk=chunk, flags=flags, passes=0)
        for _ in range(3):
            srcs = sorted(set(int(x) for x in rng.integers(0, n, int(rng.integers(1, 20)))))
            mode = [None, "dense", "sparse"][int(rng.integers(0, 3))]
            raw = bool(rng.integers(0, 2))
            run = dict(what, sources=srcs, mode=mode, raw=raw)
            res = bref.literal(n, row_ptr, src, srcs)
            if res.max_dist > 254 or max(max(s) for s in res.sigma) >= 2 ** 64 - 1:
                continue  # (HB_ERR_LIMIT cases: tests/test_betweenness.py)
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
            what["passes"] += st["levels_forward"] + st["levels_backward"]
    return what


def similarity_case(rng, max_nodes, case):
    """hb_inbound_similarity: random graph x random entry lists (duplicates, unknown ids, an entry equal to a scored node - every known
    entry is one) x a limit (0 = whole in-lists, and small values that cut) x a key set (few distinct keys: ties are common) x the three
    mode settings, against the host restatement (tests/inbound_similarity_ref.py over the BitVecs of tests/limited_similarity_ref.py),
    bit for bit."""
    from stract_amd.harmonic import EdgeListGraph, ids_from_ints
    from tests import inbound_similarity_ref as sref
    from tests import limited_similarity_ref as lref
    kind, tuples = graphs.random_graph(rng)
    if not tuples:
        return None
    nodes = sorted({x for e in tuples for x in e[:2]})
    tuples = sorted(set(tuples) | {(v, v) for v in nodes if rng.integers(0, 8) == 0})  # some self links: listed rows at every limit
    chunk = int(rng.choice([0, 0, 4, 8, 64]))
    flags = _lib.HB_FLAG_ALL_RELS | int(rng.choice([0, 0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP, _lib.HB_FLAG_NO_SPARSE]))
    with _lib.Context(flags=flags, chunk=chunk) as ctx:
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        graph = ctx.graph()
        ids = graph[0]
        ints = sref.id_ints(ids)
        n = len(ints)
        what = dict(case=case, kind="similarity:" + kind, n=n, m=int(len(graph[2])), chunk=chunk, flags=flags, passes=0)

        def entries(k):
            e = [ints[int(x)] for x in rng.integers(0, n, k)]
            if k > 2:
                e[int(rng.integers(0, k))] = (1 << 100) + int(rng.integers(0, 3))  # no node of the graph
                e[int(rng.integers(0, k))] = e[0]  # a duplicate
            return e

        for _ in range(2):
            liked, disliked = entries(int(rng.integers(0, 40))), entries(int(rng.integers(0, 20)))
            if not liked and not disliked:
                continue
            normalized = bool(rng.integers(0, 2))
            self_score = [None, 0.25, 3.0][int(rng.integers(0, 3))]
            limit = int(rng.choice([0, 0, 1, 2, 3, 8, 1024]))
            keys = [(v, int(rng.integers(0, 4))) for v in ints if rng.integers(0, 2)] if rng.integers(0, 2) else []
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
                what["passes"] += sum(st["levels_mode"])
            asked = liked[:3] + [1 << 100, 5]
            assert ctx.similarity_lookup(ids_from_ints(asked)).tobytes() == \
                sref.lookup(bv, liked, disliked, normalized, 1.0 if self_score is None else self_score, asked).tobytes(), ("lookup", what)
            k = int(rng.integers(1, n + 3))
            tids, tvals = ctx.similarity_top(k)
            order = sref.top_order(ids, want, k)
            assert sref.id_ints(tids) == [v for _, v in order] and tvals.tolist() == [x for x, _ in order], ("top", what, k)
    return what


def score_hosts_case(rng, max_nodes, case):
    """hb_score_hosts: random graph (self links added) x a key set (few distinct keys) x a limit x 1 to 5 requests that share hosts,
    with unknown ids and duplicates on every side x the piece size and the debug flags of the list selects, against the route it
    replaces on the same context - hb_inbound_similarity + hb_similarity_lookup per request - and against the literal restatement
    (tests/score_hosts_ref.py): every score bit for bit, every counter."""
    from stract_amd.harmonic import EdgeListGraph, ids_from_ints
    from tests import inbound_similarity_ref as sref
    from tests import score_hosts_ref as ref
    kind, tuples = graphs.random_graph(rng)
    if not tuples:
        return None
    nodes = sorted({x for e in tuples for x in e[:2]})
    tuples = sorted(set(tuples) | {(v, v) for v in nodes if rng.integers(0, 8) == 0})
    chunk = int(rng.choice([0, 0, 4, 8, 64]))
    flags = _lib.HB_FLAG_ALL_RELS | int(rng.choice([0, 0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP, _lib.HB_FLAG_NO_SPARSE]))
    with _lib.Context(flags=flags, chunk=chunk) as ctx:
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        graph = ctx.graph()
        ints = sref.id_ints(graph[0])
        n = len(ints)
        what = dict(case=case, kind="score_hosts:" + kind, n=n, m=int(len(graph[2])), chunk=chunk, flags=flags, passes=0)
        pool = [ints[int(x)] for x in rng.integers(0, n, 12)] + [(1 << 100) + 1, (1 << 100) + 2]  # what the requests share

        def entries(k):
            return [pool[int(rng.integers(0, len(pool)))] if rng.integers(0, 3) == 0 else ints[int(rng.integers(0, n))] for _ in range(k)]

        for _ in range(2):
            limit = int(rng.choice([1, 2, 3, 8, 512, 1024]))
            keys = [(v, int(rng.integers(0, 4))) for v in ints if rng.integers(0, 2)] if rng.integers(0, 2) else []
            if keys:
                ctx.links_set_keys(ids_from_ints([v for v, _ in keys]), np.array([k for _, k in keys], dtype=np.uint64))
            else:
                ctx.links_set_keys()
            requests = [dict(liked=entries(int(rng.integers(0, 40))), disliked=entries(int(rng.integers(0, 20))), nodes=entries(int(rng.integers(0, 30))),
                             normalized=bool(rng.integers(0, 2)), self_score=[None, 0.25, 3.0][int(rng.integers(0, 3))]) for _ in range(int(rng.integers(1, 6)))]
            want, wst = ref.literal(ref.tables(*graph, keys, limit), requests)
            sflags = int(rng.choice([0, _lib.HB_LINKS_SPREAD_ORDS, _lib.HB_LINKS_NO_SHORTCUT]))
            small = bool(rng.integers(0, 2))
            run = dict(what, limit=limit, keys=keys, requests=requests, sflags=sflags, small_pieces=small)
            st = ctx.score_hosts([dict(r, liked=ids_from_ints(r["liked"]), disliked=ids_from_ints(r["disliked"]), nodes=ids_from_ints(r["nodes"])) for r in requests],
                                 limit=limit, flags=sflags, small_pieces=small, slots_per_batch=int(rng.choice([0, 3])))
            got = ctx.score_copy()
            assert [g.tobytes() for g in got] == [w.tobytes() for w in want], ("scores against the restatement", run)
            assert {k: st[k] for k in wst} == wst, ("stats", run, st)
            for r, g in zip(requests, got):
                if r["liked"] or r["disliked"]:
                    ctx.inbound_similarity(ids_from_ints(r["liked"]), ids_from_ints(r["disliked"]), normalized=r["normalized"], self_score=r["self_score"], limit=limit)
                    assert ctx.similarity_lookup(ids_from_ints(r["nodes"])).tobytes() == g.tobytes(), ("scores against the lookup route", run)
            what["passes"] += st["pieces"]
    return what


def nearest_seed_case(rng, max_nodes, case):
    """hb_nearest_seed: random graph (self links added) x random original / key lists (duplicates, unknown ids, 0.0, few distinct keys so
    that ties are common, u64::MAX) x rounds x discount, against the host restatement (tests/nearest_seed_ref.py): the seed of every
    node, every value bit for bit, every counter, the top order."""
    from stract_amd.harmonic import EdgeListGraph, ids_from_ints
    from tests import inbound_similarity_ref as sref
    from tests import nearest_seed_ref as nref
    kind, tuples = graphs.random_graph(rng)
    if not tuples:
        return None
    nodes_in = sorted({x for e in tuples for x in e[:2]})
    tuples = list(tuples) + [(v, v) for v in nodes_in if rng.random() < 0.1]
    chunk = int(rng.choice([0, 0, 4, 8, 64]))
    flags = _lib.HB_FLAG_ALL_RELS | int(rng.choice([0, 0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP, _lib.HB_FLAG_NO_SPARSE]))
    with _lib.Context(flags=flags, chunk=chunk) as ctx:
        ctx.load_edges(EdgeListGraph.from_tuples(tuples).host_edges())
        graph = ctx.graph()
        ints = sref.id_ints(graph[0])
        n = len(ints)
        what = dict(case=case, kind="nearest_seed:" + kind, n=n, m=int(len(graph[2])), chunk=chunk, flags=flags, passes=0)
        for _ in range(3):
            share = [0.02, 0.1, 0.5][int(rng.integers(0, 3))]
            orig = [(ints[int(x)], [0.0, float(rng.random()), float(rng.integers(0, 4)) / 4.0][int(rng.integers(0, 3))])
                    for x in rng.integers(0, n, max(1, int(n * share)))]
            orig += [((1 << 100) + 1, 0.5), orig[0]]
            spread = int(rng.choice([1, 3, 1 << 62]))
            keys = [(v, int(rng.integers(0, spread)) if rng.random() < 0.9 else nref.U64_MAX) for v in ints if rng.random() < 0.8]
            keys += [((1 << 100) + 2, 0)] + keys[:2]
            discount = [0.5, 0.3, 0.0, 1.0][int(rng.integers(0, 4))]
            rounds = int(rng.choice([0, 1, 2, 5, 255]))
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
            k = int(rng.integers(1, n + 3))
            tids, tvals = ctx.nearest_seed_top(k)
            order = nref.top_order(vals, k)
            assert sref.id_ints(tids) == [v for v, _ in order] and tvals.tolist() == [x for _, x in order], ("top", run, k)
            what["passes"] += st["rounds_run"]
    return what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["passes", "records", "tail", "ranks", "mixed", "distances", "betweenness", "similarity", "nearest_seed", "score_hosts"], default="passes")
    ap.add_argument("--ids", choices=["plain", "extreme", "mixed"], default="plain")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-nodes", type=int, default=6000)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    t0 = time.time()
    done, edges, passes = 0, 0, 0
    case = 0
    while time.time() - t0 < a.seconds:
        extreme = a.ids == "extreme" or (a.ids == "mixed" and case % 2 == 1)
        try:
            if a.mode == "distances":
                w = distances_case(rng, a.max_nodes, case)
            elif a.mode == "betweenness":
                w = betweenness_case(rng, a.max_nodes, case)
            elif a.mode == "similarity":
                w = similarity_case(rng, a.max_nodes, case)
            elif a.mode == "nearest_seed":
                w = nearest_seed_case(rng, a.max_nodes, case)
            elif a.mode == "score_hosts":
                w = score_hosts_case(rng, a.max_nodes, case)
            elif a.mode == "ranks" or (a.mode == "mixed" and case % 6 == 4):
                w = ranks_case(rng, a.max_nodes, case, extreme)
            elif a.mode == "tail" or (a.mode == "mixed" and case % 6 == 5):
                w = tail_case(rng, case)
            elif a.mode == "records" or (a.mode == "mixed" and case % 3 == 2):
                w = records_case(rng, a.max_nodes, case, extreme)
            else:
                w = one_case(rng, a.max_nodes, case, extreme)
        except AssertionError as e:
            print(json.dumps({"failed": str(e.args[0] if e.args else e), "seed": a.seed, "cases_before": done}))
            sys.exit(1)
        case += 1
        if w:
            done += 1
            edges += w["m"]
            passes += w["passes"]
    print(json.dumps({"library": _lib.LIB_PATH, "mode": a.mode, "ids": a.ids, "seed": a.seed, "seconds": round(time.time() - t0, 1), "cases": done, "edges": edges, "passes_compared": passes, "failed": None}))


if __name__ == "__main__":
    main()
