#!/usr/bin/env python3
"""tools/score_hosts_bench.py - hb_score_hosts (the result hosts of a search against its liked / disliked hosts) at the BASELINE sizes,
against the route it replaces.

    python tools/score_hosts_bench.py --configs C3 --out profiles/score_hosts_bench_C3.json

Per graph: keys from the ranks of hb_run, limit 512.  A search has 300 result hosts, half of them the hosts of highest in-degree and
half seeded random hosts, and 1, 16 or 64 liked hosts or 32 liked plus 32 disliked ones - once hosts of high in-degree (the ones after
the 150 result hubs), once random hosts.  Per shape: a warm-up call whose scores are compared bit for bit with the comparator's, then
the median wall ms of `--runs` calls and the median call's per-stage GPU times and counters.
The comparator, in the same process and session: hb_inbound_similarity(limit = 512) with its cut lists already built, followed by
hb_similarity_lookup of the 300 hosts - timed the same way BEFORE and AFTER the new operator's runs; both medians are reported and their
difference is the spread a speed-up has to exceed.
`batch`: 16 searches of 16 liked hosts each in one call against the same 16 searches in 16 calls - the list selects of the shared
result hubs are what one call saves."""
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

LIMIT = 512
STAGES = ("ms_lists", "ms_bitvec", "ms_pairs", "ms_finish")
COUNTERS = ("distinct", "pairs", "pairs_self", "pairs_empty", "pairs_gated", "pairs_intersected", "pieces", "device_bytes")


def _timed(fn, runs):
    rows = []
    for _ in range(runs):
        t = time.perf_counter()
        st = fn()
        rows.append(((time.perf_counter() - t) * 1e3, st))
    rows.sort(key=lambda r: r[0])
    return rows[len(rows) // 2], [r[0] for r in rows]


def bench_config(name, runs, seed):
    g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m), limit=LIMIT, shapes=[])
    indeg = np.diff(np.asarray(g.row_ptr, dtype=np.int64))
    by_indeg = np.argsort(-indeg, kind="stable")
    rng = np.random.default_rng(seed)
    nodes = g.ids[np.concatenate([by_indeg[:150], rng.choice(g.n, 150, replace=False)])]
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        ctx.links_set_keys(from_ranks=True)
        first = ctx.inbound_similarity(g.ids[by_indeg[:1]], limit=LIMIT)  # builds the comparator's per-graph state and cut lists
        out["comparator_state"] = dict(ms_bloom=first["ms_bloom"], ms_lists=first["ms_lists"], listed_rows=int(first["listed_rows"]),
                                       device_bytes=first["device_bytes"])

        def old_route(liked, disliked):
            st = ctx.inbound_similarity(liked, disliked, limit=LIMIT)
            return st, ctx.similarity_lookup(nodes)

        def new_route(requests):
            st = ctx.score_hosts(requests, limit=LIMIT)
            return st, ctx.score_copy()

        def anchors(pick, k):
            return g.ids[by_indeg[150:150 + k]] if pick == "hub" else g.ids[rng.choice(g.n, k, replace=False)]

        for pick in ("hub", "random"):
            for shape, (nl, nd) in (("1 liked", (1, 0)), ("16 liked", (16, 0)), ("64 liked", (64, 0)), ("32 liked + 32 disliked", (32, 32))):
                a = anchors(pick, nl + nd)
                liked, disliked = a[:nl], a[nl:]
                req = [dict(liked=liked, disliked=disliked, nodes=nodes)]
                want = old_route(liked, disliked)[1]  # warm-up of both routes, and the contract
                got = new_route(req)[1][0]
                if got.tobytes() != want.tobytes():
                    sys.exit("score_hosts_bench: %s %s: the scores differ from hb_inbound_similarity + hb_similarity_lookup" % (pick, shape))
                (old_a, (old_st, _)), _ = _timed(lambda: old_route(liked, disliked), runs)
                (new_ms, (st, _)), new_all = _timed(lambda: new_route(req), runs)
                (old_b, _), _ = _timed(lambda: old_route(liked, disliked), runs)
                rec = dict(anchors=pick, shape=shape, nodes=300, new_ms=new_ms, new_ms_min=min(new_all), new_ms_max=max(new_all),
                           old_ms_before=old_a, old_ms_after=old_b, old_spread_ms=abs(old_a - old_b), old_batches=int(old_st["batches"]),
                           speedup=min(old_a, old_b) / new_ms, faster_by_more_than_the_spread=bool(min(old_a, old_b) - new_ms > abs(old_a - old_b)))
                rec.update({k: st[k] for k in STAGES})
                rec.update({k: int(st[k]) for k in COUNTERS})
                rec["pair_kernel_pairs_per_s"] = st["pairs"] / st["ms_pairs"] * 1e3 if st["ms_pairs"] else None
                out["shapes"].append(rec)
                print(json.dumps(dict(config=name, **rec)), flush=True)
        # 16 searches in one call against 16 calls
        searches = []
        for r in range(16):
            sel = np.concatenate([by_indeg[:150], rng.choice(g.n, 150, replace=False)])
            searches.append(dict(liked=np.concatenate([anchors("hub", 8), anchors("random", 8)]), nodes=g.ids[sel]))
        one = new_route(searches)[1]
        each = [new_route([s])[1][0] for s in searches]
        if [x.tobytes() for x in one] != [x.tobytes() for x in each]:
            sys.exit("score_hosts_bench: 16 requests in one call differ from 16 calls")
        (batch_ms, (st, _)), _ = _timed(lambda: new_route(searches), runs)
        (single_ms, _), _ = _timed(lambda: [new_route([s]) for s in searches][-1], runs)
        (batch_ms2, _), _ = _timed(lambda: new_route(searches), runs)
        out["batch"] = dict(requests=16, one_call_ms=batch_ms, one_call_ms_again=batch_ms2, sixteen_calls_ms=single_ms, ratio=single_ms / batch_ms,
                            distinct=int(st["distinct"]), pairs=int(st["pairs"]), **{k: st[k] for k in STAGES})
        print(json.dumps(dict(config=name, batch=out["batch"])), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after a warm-up call; at least 5")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("score_hosts_bench: no GPU (timings are taken on the device only)")
    runs = max(args.runs, 5)
    res = dict(tool="tools/score_hosts_bench.py", runs=runs, seed=args.seed, results=[bench_config(c, runs, args.seed) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
