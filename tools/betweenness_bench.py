#!/usr/bin/env python3
"""tools/betweenness_bench.py - hb_betweenness (batched Brandes) at the BASELINE sizes.

    python tools/betweenness_bench.py --configs C3 --out profiles/betweenness_bench_C3.json

Per graph: 8, 64 and 512 seeded sources (nodes with an out-edge), HB_BC_RAW.  Reported per source count: median wall ms of `--runs`
calls after a warm-up call, and from the median call's statistics the forward / backward GPU time per batch of eight sources, the
levels and GPU time per mode (dense, bitmap, sweep) and the slowest dense forward level.
The yardstick, measured in the same process on the same graph: the slowest dense level of the sampled walk (hb_sampled_harmonic with 512
seeded sources) - the same gather shape with OR as the join; a betweenness level also stores a 64-byte F row per changed row.
`extrapolated_100000_sources_s` = the per-batch time of the largest measured source count x 12 500 batches: an extrapolation, not a
measurement."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stract_amd import _lib, synth  # noqa: E402


def _timed(fn, runs):
    fn()  # warm-up: first launches load code objects, first calls allocate
    rows = []
    for _ in range(runs):
        t = time.perf_counter()
        st = fn()
        rows.append(((time.perf_counter() - t) * 1e3, st))
    rows.sort(key=lambda r: r[0])
    return rows[len(rows) // 2]  # the median call and its statistics


def bench_config(name, runs, seed, counts, device_gen=False):
    dg = synth.make_config_on_device(name) if device_gen else None
    if dg:
        G, scale, label = dg
        ids, row_ptr, src = G.host_arrays()
        g = types.SimpleNamespace(ids=ids, row_ptr=row_ptr, src=src, n=int(G.n), m=int(G.m))
        G.close()
    else:
        g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m), runs=[])
    has_out = np.flatnonzero(np.bincount(np.asarray(g.src), minlength=g.n) > 0)
    rng = np.random.default_rng(seed)
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        # the yardstick: the sampled walk's dense level on this graph, in this process
        picks = np.sort(rng.choice(has_out, min(512, len(has_out)), replace=False))
        ms, st = _timed(lambda: ctx.sampled_harmonic(sources=g.ids[picks], max_dist=15), runs)
        dense = [t for t, m in zip(st["level_ms"], st["level_modes"]) if m == 1]  # (bit 0 = only dense launches at that level)
        out["sampled_walk"] = dict(ms=ms, level_ms=st["level_ms"], level_modes=st["level_modes"], dense_level_ms_max=max(dense) if dense else None)
        for k in counts:
            sources = g.ids[np.sort(rng.choice(has_out, min(k, len(has_out)), replace=False))]
            ms, st = _timed(lambda: ctx._betweenness(sources, True, None), runs)
            b = max(st["batches"], 1)
            rec = dict(sources=int(st["sources"]), batches=int(st["batches"]), ms=ms, ms_per_batch=ms / b, ms_forward_per_batch=st["ms_forward"] / b,
                       ms_backward_per_batch=st["ms_backward"] / b, max_dist=st["max_dist"], levels_forward=st["levels_forward"],
                       levels_backward=st["levels_backward"], levels_mode=dict(zip(("dense", "bitmap", "sweep"), st["levels_mode"])),
                       ms_mode=dict(zip(("dense", "bitmap", "sweep"), st["ms_mode"])),
                       ms_per_level_mode={m: (t / n if n else None) for m, t, n in zip(("dense", "bitmap", "sweep"), st["ms_mode"], st["levels_mode"])},
                       dense_level_ms_max=st["ms_dense_max"], edges_gathered_per_m=st["edges_gathered"] / max(g.m, 1) / b, device_bytes=st["device_bytes"])
            if out["sampled_walk"]["dense_level_ms_max"] and st["ms_dense_max"]:
                rec["dense_level_over_sampled_dense_level"] = st["ms_dense_max"] / out["sampled_walk"]["dense_level_ms_max"]
            out["runs"].append(rec)
            print(json.dumps(dict(config=name, **rec)), flush=True)
        if out["runs"]:
            out["extrapolated_100000_sources_s"] = out["runs"][-1]["ms_per_batch"] * 12500 / 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--sources", default="8,64,512")
    ap.add_argument("--device-gen", action="store_true", help="generate the graphs on the GPU (plain R-MAT configs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("betweenness_bench: no GPU (timings are taken on the device only)")
    counts = [int(x) for x in args.sources.split(",")]
    res = dict(tool="tools/betweenness_bench.py", runs=args.runs, seed=args.seed,
               results=[bench_config(c, args.runs, args.seed, counts, args.device_gen) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
