#!/usr/bin/env python3
"""tools/nearest_seed_bench.py - hb_nearest_seed (the seed of every node, then one fill round) at the BASELINE sizes.

    python tools/nearest_seed_bench.py --configs C3 --out profiles/nearest_seed_bench_C3.json

Per graph: 64-bit hash keys for every node, original values on a seeded tenth of the nodes, rounds = 1.  Reported: median wall ms of
`--runs` calls after a warm-up call, and from the median call's statistics the GPU ms of the seed level (candidates, chunk rows, node
rows: one pull over the plan that gathers 16 bytes per edge) and of the values (round 0, one fill round, the result in NodeID order).
The yardsticks, measured in the same process on the same graph: the slowest dense HyperBall pass of hb_run (the same pull, 64 bytes
per edge) and the per-graph state of hb_inbound_similarity (in-degrees, position bytes and sim_bloom_kernel: the same pull, 1 byte per
edge).  `seed_level_over_dense_pass` is the ratio of the first to the second."""
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


def _timed(fn, runs):
    fn()  # warm-up: first launches load code objects, the first call allocates the operator's buffers
    rows = []
    for _ in range(runs):
        t = time.perf_counter()
        st = fn()
        rows.append(((time.perf_counter() - t) * 1e3, st))
    rows.sort(key=lambda r: r[0])
    return rows[len(rows) // 2]  # the median call and its statistics


def _hash_keys(lo):
    z = lo * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def bench_config(name, runs, seed):
    g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m))
    rng = np.random.default_rng(seed)
    ids = np.ascontiguousarray(g.ids)
    keys = _hash_keys(np.asarray(ids["lo"], dtype=np.uint64))
    picks = np.sort(rng.choice(g.n, max(g.n // 10, 1), replace=False))
    orig_ids, orig_vals = ids[picks], rng.random(len(picks))
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        # the yardsticks: the dense passes of hb_run and the similarity operator's per-graph state, on this graph, in this process
        ctx.run()
        ctx.run()
        dense = [p["ms_gpu"] for p in ctx.pass_stats() if p["mode"] == 0]
        yard = max(dense) if dense else None
        out["hyperball"] = dict(passes=len(ctx.pass_stats()), dense_pass_ms=dense, dense_pass_ms_max=yard)
        first = ctx.inbound_similarity(ids[picks[:1]])
        out["similarity_per_graph_state"] = dict(ms_bloom=first["ms_bloom"])
        ms, st = _timed(lambda: ctx.nearest_seed(orig_ids, orig_vals, ids, keys, discount_factor=0.5, rounds=1), runs)
        rec = dict(ms=ms, ms_seed=st["ms_seed"], ms_fill=st["ms_fill"], with_original=int(st["with_original"]), filled=int(st["filled"][0]),
                   no_seed=int(st["no_seed"]), seed_without_value=int(st["seed_without_value"]), device_bytes=int(st["device_bytes"]))
        if yard:
            rec["seed_level_over_dense_pass"] = st["ms_seed"] / yard
        if first["ms_bloom"]:
            rec["seed_level_over_similarity_state"] = st["ms_seed"] / first["ms_bloom"]
        ms_img, st_img = _timed(lambda: ctx.nearest_seed(None, None, ids, keys, discount_factor=0.5, rounds=1, from_image=True), runs)
        rec["from_image"] = dict(ms=ms_img, ms_seed=st_img["ms_seed"], ms_fill=st_img["ms_fill"], with_original=int(st_img["with_original"]))
        t = time.perf_counter()
        ctx.nearest_seed_top(1_000_000)
        rec["top_1e6_ms"] = (time.perf_counter() - t) * 1e3
        out["nearest_seed"] = rec
        print(json.dumps(dict(config=name, **rec)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("nearest_seed_bench: no GPU (timings are taken on the device only)")
    res = dict(tool="tools/nearest_seed_bench.py", runs=args.runs, seed=args.seed,
               results=[bench_config(c, args.runs, args.seed) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
