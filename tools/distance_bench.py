#!/usr/bin/env python3
"""tools/distance_bench.py - hb_distances (exact BFS, forward and reversed) at the BASELINE sizes, against the only route the library
offered before it: hb_sampled_harmonic with that one source and max_dist = 15.

    python tools/distance_bench.py --configs C3,C4 --out profiles/distance_bench_C3_C4.json
    python tools/distance_bench.py --configs C3 --sweep 4,14,64:8,24,128      (alpha values : beta values of the switch rule)

Per graph: the highest-out-degree node, the highest-in-degree node and six seeded random nodes, one call each, forward and
reversed.  Reported per (source, direction): median ms of `--runs` calls after a warm-up call (wall clock around the call, which ends
in a device synchronise; and the GPU time of the level loop from the library's events), the per-level step kinds and frontier sizes,
edges_inspected / m, and traversed edges per second (the edges out of / into the reached nodes over the median time).
The yardstick: the workaround's median ms on the same graph and source, and the ratio workaround / (forward call with max_dist = 15).
The baseline leg uses only calls every version of the library has, so the script also runs on a tree without hb_distances
(--baseline-only is then implied).  hb_sampled_harmonic itself is unchanged by the distance feature, so one process measures both."""
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


def _median_ms(fn, runs):
    fn()  # warm-up: first launches load code objects, first calls allocate
    wall, extra = [], None
    for _ in range(runs):
        t = time.perf_counter()
        extra = fn()
        wall.append((time.perf_counter() - t) * 1e3)
    return statistics.median(wall), extra


def _sources(g, seed):
    src = np.asarray(g.src)
    outdeg = np.bincount(src, minlength=g.n)
    indeg = np.diff(np.asarray(g.row_ptr).astype(np.int64))
    rng = np.random.default_rng(seed)
    picks = [("max_out_degree", int(np.argmax(outdeg))), ("max_in_degree", int(np.argmax(indeg)))]
    picks += [("random_%d" % i, int(s)) for i, s in enumerate(rng.integers(0, g.n, 6))]
    return picks, outdeg, indeg


def bench_config(name, runs, seed, have_distances, baseline, sweep, device_gen=False):
    dg = synth.make_config_on_device(name) if device_gen else None
    if dg:  # the same graph generated on the GPU (minutes faster at C4), brought to the host once and freed there before the load
        G, scale, label = dg
        ids, row_ptr, src = G.host_arrays()
        g = types.SimpleNamespace(ids=ids, row_ptr=row_ptr, src=src, n=int(G.n), m=int(G.m))
        G.close()
    else:
        g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m), sources=[])
    picks, outdeg, indeg = _sources(g, seed)
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        t = time.perf_counter()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        out["load_s"] = time.perf_counter() - t
        for kind, sid in picks:
            one = g.ids[[sid]]
            rec = dict(kind=kind, sid=sid, out_degree=int(outdeg[sid]), in_degree=int(indeg[sid]))
            if baseline:
                ms, st = _median_ms(lambda: ctx.sampled_harmonic(sources=one, max_dist=15), runs)
                rec["workaround_ms"] = ms
                rec["workaround_level_changed"] = st["level_changed"]
            if have_distances:
                for tag, kw in (("forward_max15", dict(max_dist=15)), ("forward", {}), ("reversed", dict(reversed=True))):
                    ms, st = _median_ms(lambda: ctx._distances(one, kw.get("reversed", False), kw.get("max_dist"), None, 0), runs)
                    all_d = ctx.distance_all()
                    reached = all_d != _lib.HB_DIST_UNREACHED
                    traversed = int((indeg if kw.get("reversed") else outdeg)[reached].sum())
                    rec[tag] = dict(ms=ms, ms_levels=st["ms_levels"], levels=st["levels"], reached=st["reached"], step=st["step"], frontier=st["frontier"],
                                    inspected_per_m=st["edges_inspected"] / max(g.m, 1), traversed_edges=traversed,
                                    gteps=traversed / (ms * 1e-3) / 1e9 if ms > 0 else None)
                if baseline:
                    rec["ratio_workaround_over_forward_max15"] = rec["workaround_ms"] / rec["forward_max15"]["ms"]
            out["sources"].append(rec)
            print(json.dumps(dict(config=name, **{k: v for k, v in rec.items() if not isinstance(v, dict)})), flush=True)
        if have_distances and sweep:
            # the switch constants: every (alpha, beta) on the two hub sources and two random ones, forward and reversed
            out["sweep"] = []
            for alpha, beta in sweep:
                os.environ["HB_DIST_ALPHA"], os.environ["HB_DIST_BETA"] = str(alpha), str(beta)
                row = dict(alpha=alpha, beta=beta, ms={})
                for kind, sid in picks[:4]:
                    for rev in (False, True):
                        ms, st = _median_ms(lambda: ctx._distances(g.ids[[sid]], rev, None, None, 0), runs)
                        row["ms"]["%s/%s" % (kind, "reversed" if rev else "forward")] = ms
                row["sum_ms"] = sum(row["ms"].values())
                out["sweep"].append(row)
                print(json.dumps(dict(config=name, sweep=row)), flush=True)
            os.environ.pop("HB_DIST_ALPHA", None)
            os.environ.pop("HB_DIST_BETA", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C4")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--sweep", default="", help="alphas:betas, e.g. 4,14,64:8,24,128")
    ap.add_argument("--device-gen", action="store_true", help="generate the graphs on the GPU (plain R-MAT configs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("distance_bench: no GPU (timings are taken on the device only)")
    have = hasattr(_lib.Context, "distances") and not args.baseline_only
    sweep = []
    if args.sweep:
        a, b = args.sweep.split(":")
        sweep = [(int(x), int(y)) for x in a.split(",") for y in b.split(",")]
    res = dict(tool="tools/distance_bench.py", runs=args.runs, seed=args.seed, has_hb_distances=have,
               results=[bench_config(c, args.runs, args.seed, have, not args.no_baseline, sweep, args.device_gen) for c in args.configs.split(",")])
    if have and not args.no_baseline:
        ratios = [s["ratio_workaround_over_forward_max15"] for r in res["results"] for s in r["sources"]]
        res["min_ratio"] = min(ratios)
        res["all_faster"] = all(x > 1.0 for x in ratios)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
