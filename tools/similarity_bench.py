#!/usr/bin/env python3
"""tools/similarity_bench.py - hb_inbound_similarity (every host against liked hosts) at the BASELINE sizes.

    python tools/similarity_bench.py --configs C3 --out profiles/similarity_bench_C3.json
    python tools/similarity_bench.py --configs C3 --limit 0,512 --out profiles/similarity_bench_C3_limit512.json

Per graph: 1, 16 and 64 liked hosts, once the hosts of highest in-degree and once seeded random hosts with an in-link.  Reported per
measurement: median wall ms of `--runs` calls after a warm-up call, and from the median call's statistics the GPU ms per phase (per-graph
state, count levels, seed + accumulate + score) and the levels and GPU ms per mode (dense, bitmap, sweep).
The yardstick, measured in the same process on the same graph: the slowest dense level of the sampled walk (hb_sampled_harmonic with 512
seeded sources) - the same gather shape, 64 bytes per edge, with OR as the join.  `dense_count_level_over_sampled_dense_level` compares a
forced-dense count level (HB_SIM_DENSE_ONLY, one batch) with it.
--limit takes a list of hb_similarity_options.limit values (0 = whole in-lists; the reference's Scorer uses 512): every value runs on the
same graph with the same anchors, in the order given.  A limited value reports, once, what the first limited call paid for the cut lists
(`per_limit_state`: ms_lists, listed rows, list entries, bytes) and per measurement the list-count kernel's share of the count time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stract_amd import _lib, synth  # noqa: E402

MODES = ("dense", "bitmap", "sweep")


def _timed(fn, runs):
    fn()  # warm-up: first launches load code objects, the first call builds the per-graph state
    rows = []
    for _ in range(runs):
        t = time.perf_counter()
        st = fn()
        rows.append(((time.perf_counter() - t) * 1e3, st))
    rows.sort(key=lambda r: r[0])
    return rows[len(rows) // 2]  # the median call and its statistics


def bench_config(name, runs, seed, counts, limits):
    g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m), runs=[])
    indeg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
    has_out = np.flatnonzero(np.bincount(np.asarray(g.src), minlength=g.n) > 0)
    by_indeg = np.argsort(-indeg, kind="stable")
    rng = np.random.default_rng(seed)
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        # the yardstick: the sampled walk's dense level on this graph, in this process
        picks = np.sort(rng.choice(has_out, min(512, len(has_out)), replace=False))
        ms, st = _timed(lambda: ctx.sampled_harmonic(sources=g.ids[picks], max_dist=15), runs)
        dense = [t for t, m in zip(st["level_ms"], st["level_modes"]) if m == 1]  # (bit 0 = only dense launches at that level)
        yard = max(dense) if dense else None
        out["sampled_walk"] = dict(ms=ms, level_ms=st["level_ms"], level_modes=st["level_modes"], dense_level_ms_max=yard)
        first = ctx.inbound_similarity(g.ids[by_indeg[:1]])  # the call that builds the per-graph state
        out["per_graph_state"] = dict(ms_bloom=first["ms_bloom"], device_bytes=first["device_bytes"])
        picks = [(pick, k, by_indeg[:k] if pick == "highest_in_degree" else rng.choice(np.flatnonzero(indeg > 0), k, replace=False))
                 for pick in ("highest_in_degree", "random") for k in counts]  # drawn once: every limit sees the same anchors
        out["per_limit_state"] = []
        for limit in limits:
            if limit:  # the call that builds the cut lists (no key set: NodeID order)
                first = ctx.inbound_similarity(g.ids[by_indeg[:1]], limit=limit)
                out["per_limit_state"].append(dict(limit=limit, ms_lists=first["ms_lists"], listed_rows=int(first["listed_rows"]),
                                                   list_entries=int(first["list_entries"]), device_bytes=first["device_bytes"]))
            for pick, k, sel in picks:
                liked = g.ids[sel]
                for mode in (None, "dense"):
                    ms, st = _timed(lambda: ctx.inbound_similarity(liked, mode=mode, limit=limit), runs)
                    levels = max(sum(st["levels_mode"]), 1)
                    rec = dict(limit=limit, pick=pick, liked=k, forced=mode or "auto", batches=int(st["batches"]), ms=ms, ms_count=st["ms_count"],
                               ms_score=st["ms_score"], ms_bloom=st["ms_bloom"], ms_lists=st["ms_lists"], ms_list_count=st["ms_list_count"],
                               ms_count_per_level=st["ms_count"] / levels, levels_mode=dict(zip(MODES, st["levels_mode"])),
                               ms_mode=dict(zip(MODES, st["ms_mode"])), rows_nonzero=int(st["rows_nonzero"]), listed_rows=int(st["listed_rows"]),
                               list_entries=int(st["list_entries"]), edges_gathered_per_m=st["edges_gathered"] / max(g.m, 1) / max(st["batches"], 1))
                    if mode == "dense" and yard:
                        rec["dense_count_level_over_sampled_dense_level"] = st["ms_mode"][0] / max(st["levels_mode"][0], 1) / yard
                    out["runs"].append(rec)
                    print(json.dumps(dict(config=name, **rec)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--liked", default="1,16,64")
    ap.add_argument("--limit", default="0", help="hb_similarity_options.limit values, comma-separated (0 = whole in-lists; e.g. 0,512)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("similarity_bench: no GPU (timings are taken on the device only)")
    counts = [int(x) for x in args.liked.split(",")]
    limits = [int(x) for x in args.limit.split(",")]
    res = dict(tool="tools/similarity_bench.py", runs=args.runs, seed=args.seed, limits=limits,
               results=[bench_config(c, args.runs, args.seed, counts, limits) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
