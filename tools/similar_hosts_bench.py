#!/usr/bin/env python3
"""tools/similar_hosts_bench.py - hb_similar_hosts (scored_nodes of SimilarHostsFinder) at the BASELINE sizes.

    python tools/similar_hosts_bench.py --configs C3 --out profiles/similar_hosts_bench_C3.json

Per graph: hb_run, keys from its ranks (HB_LINKS_KEYS_FROM_RANKS), then batches of 1, 8 and 64 liked hosts, taken from the highest
in-degrees and at random (seeded), limit 100.  Reported per batch: median wall ms of `--runs` calls after a warm-up call
(hb_similar_hosts + hb_similar_copy), the wall time of the median call's stages, its counters, and the wall time of the numpy form of the
restatement (tests/similar_hosts_ref.py numpy_form; its CSR by source is built once, untimed) on the same graph and keys in the same
process.  The warm-up compares candidates, counts, list and score bits entry for entry."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from stract_amd import _lib, synth  # noqa: E402
from tests import links_ref as lref  # noqa: E402
from tests import similar_hosts_ref as sref  # noqa: E402
from links_bench import U64_MAX, _median  # noqa: E402


def bench_config(name, runs, seed, limit):
    g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m), limit=limit)
    rng = np.random.default_rng(seed)
    ids = np.ascontiguousarray(g.ids)
    t = time.perf_counter()
    state = sref.numpy_state(ids, g.row_ptr, g.src)
    out["host_state_s"] = time.perf_counter() - t
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.run()
        rids, _ = ctx.results()
        key = np.full(g.n, U64_MAX, dtype=np.uint64)
        key[sref.sids_of_subset(ids, rids)] = ctx.ranks()
        ctx.links_set_keys(from_ranks=True)
        indeg = np.diff(state["rp"])
        by_indeg = np.argsort(-indeg, kind="stable")
        out["batches"] = []
        for which in ("hubs", "random"):
            for count in (1, 8, 64):
                sids = by_indeg[:count] if which == "hubs" else rng.choice(g.n, count, replace=False)
                liked_ids = ids[sids]
                liked = [sref._node(ids, int(s)) for s in sids]

                def device():
                    s = ctx.similar_hosts(liked_ids, limit)
                    return s, ctx.similar_copy(), ctx.similar_candidates()
                ms, (st, top, cand) = _median(device, runs)
                t = time.perf_counter()
                want = sref.numpy_form(state, key, liked, limit)
                ms_host = (time.perf_counter() - t) * 1e3
                same = (list(zip(lref.id_ints(cand[0]), cand[1].tolist())) == want["candidates"] and lref.id_ints(top[0]) == [v for v, _ in want["top"]]
                        and top[1].view(np.uint64).tolist() == np.array([s for _, s in want["top"]], dtype=np.float64).view(np.uint64).tolist())
                rec = dict(batch=which, liked=count, ms=ms, host_ms=ms_host, host_over_device=ms_host / ms, equal_to_numpy_form=bool(same),
                           **{k: (float(v) if isinstance(v, float) else int(v)) for k, v in st.items() if k != "struct_size"})
                out["batches"].append(rec)
                print(json.dumps(dict(config=name, **rec)), flush=True)
                if not same:
                    sys.exit("similar_hosts_bench: the device result differs from the numpy form's")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("similar_hosts_bench: no GPU (timings are taken on the device only)")
    res = dict(tool="tools/similar_hosts_bench.py", runs=args.runs, seed=args.seed,
               results=[bench_config(c, args.runs, args.seed, args.limit) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
