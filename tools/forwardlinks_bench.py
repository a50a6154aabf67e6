#!/usr/bin/env python3
"""tools/forwardlinks_bench.py - hb_forwardlinks (limited, rank-ordered host forward links) at the BASELINE sizes.

    python tools/forwardlinks_bench.py --configs C3 --out profiles/forwardlinks_bench_C3.json

Per graph: hb_run, keys from its ranks (HB_LINKS_KEYS_FROM_RANKS), then four batches of 1024 queries - the 1024 hosts of highest
out-degree and 1024 seeded random hosts, each with limit 128 and 512.  Reported per batch: median wall ms of `--runs` calls after a
warm-up call (hb_forwardlinks + hb_links_copy of ids and keys), the GPU ms of the median call's three stages, and the entries gathered
per second; the first call after the load, which builds the table of tops, is timed on its own.  The yardstick is the host route of
tools/links_bench.py on the same graph and keys, in the same process, reading the out-lists of the queried hosts from a CSR by source:
that CSR is built once, untimed and for the queried hosts only (one pass over the edges), as a host that serves forward links would
keep it.  The warm-up call's lists are compared with the host route's, entry for entry."""
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
from links_bench import U64_MAX, _host_order, _host_route, _median, _sids_of_subset  # noqa: E402


def _out_lists(rp, src, n, qsids):
    """(out_ptr, dst) of a CSR by source that holds the out-lists of qsids only (every other list is empty)"""
    wanted = np.zeros(n, dtype=bool)
    wanted[qsids] = True
    at = np.flatnonzero(wanted[src])
    frm = np.asarray(src[at], dtype=np.int64)
    to = (np.searchsorted(rp, at, side="right") - 1).astype(np.uint32)
    order = np.lexsort((to, frm))
    out_ptr = np.concatenate(([0], np.cumsum(np.bincount(frm, minlength=n)))).astype(np.int64)
    return out_ptr, to[order]


def bench_config(name, runs, seed):
    g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m))
    rng = np.random.default_rng(seed)
    ids = np.ascontiguousarray(g.ids)
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        rp, src = np.asarray(g.row_ptr, dtype=np.int64), np.asarray(g.src)
        ctx.run()
        rids, _ = ctx.results()
        key = np.full(g.n, U64_MAX, dtype=np.uint64)
        key[_sids_of_subset(ids, rids)] = ctx.ranks()
        st = ctx.links_set_keys(from_ranks=True)
        out["set_keys_from_ranks_ms"] = st["ms_total"]
        ord_of, inv = _host_order(key)
        outdeg = np.bincount(src, minlength=g.n)
        batches = {"hubs": np.argsort(-outdeg, kind="stable")[:1024], "random": rng.choice(g.n, min(1024, g.n), replace=False)}
        t = time.perf_counter()
        first = ctx.forwardlinks(ids[batches["random"][:1]], 128)
        out["first_call_after_load"] = dict(ms=(time.perf_counter() - t) * 1e3, ms_expand=first["ms_expand"], device_bytes=int(first["device_bytes"]),
                                            virtual_rows=int(ctx.stats()["virtual_rows"]))
        out["batches"] = []
        for which, qsids in batches.items():
            qids = ids[qsids]
            out_ptr, dst = _out_lists(rp, src, g.n, qsids)
            for limit in (128, 512):
                def device():
                    s = ctx.forwardlinks(qids, limit)
                    return s, ctx.links_copy()
                ms, (st, res) = _median(device, runs)
                ms_host, want = _median(lambda: _host_route(out_ptr, dst, ord_of, inv, key, qsids, limit), runs)
                same = (np.array_equal(res[0], want[0]) and res[1].tobytes() == np.ascontiguousarray(ids[want[1]]).tobytes()
                        and np.array_equal(res[2], want[2]) and np.array_equal(res[3], want[3]))
                rec = dict(batch=which, queries=len(qsids), limit=limit, ms=ms, ms_expand=st["ms_expand"], ms_select=st["ms_select"], ms_emit=st["ms_emit"],
                           entries_gathered=int(st["edges_gathered"]), entries_gathered_per_s=st["edges_gathered"] / (ms * 1e-3),
                           entries_written=int(st["entries"]), segments=int(st["rows_walked"]), selected=int(st["selected"]),
                           batches=int(st["batches"]), device_bytes=int(st["device_bytes"]), host_ms=ms_host,
                           host_entries_gathered_per_s=st["edges_gathered"] / (ms_host * 1e-3), host_over_device=ms_host / ms, equal_to_host_route=bool(same))
                out["batches"].append(rec)
                print(json.dumps(dict(config=name, **rec)), flush=True)
                if not same:
                    sys.exit("forwardlinks_bench: the device lists differ from the host route's")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("forwardlinks_bench: no GPU (timings are taken on the device only)")
    res = dict(tool="tools/forwardlinks_bench.py", runs=args.runs, seed=args.seed,
               results=[bench_config(c, args.runs, args.seed) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
