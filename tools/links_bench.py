#!/usr/bin/env python3
"""tools/links_bench.py - hb_links_set_keys / hb_backlinks (limited, rank-ordered host backlinks) at the BASELINE sizes.

    python tools/links_bench.py --configs C3 --out profiles/links_bench_C3.json

Per graph: hb_run, keys from its ranks (HB_LINKS_KEYS_FROM_RANKS), then four batches of 1024 queries - the 1024 hosts of highest
in-degree and 1024 seeded random hosts, each with limit 128 and 512.  Reported per batch: median wall ms of `--runs` calls after a
warm-up call (hb_backlinks + hb_links_copy of ids and keys), the GPU ms of the median call's three stages, and the source entries
gathered per second.  hb_links_set_keys is timed separately.  The yardstick is the host route on the same graph and keys, in the same
process: the dense order by one np.lexsort over (key, sid) - the host's counterpart of hb_links_set_keys - and per query an
np.argpartition + sort of the order values of the in-list read from the CSR (hb_debug_copy_graph where the library keeps it, else the
arrays the graph was loaded from: the same CSR).  The warm-up call's lists are compared with the host route's, entry for entry."""
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

U64_MAX = np.uint64((1 << 64) - 1)


def _median(fn, runs):
    fn()  # warm-up: first launches load code objects, the first call allocates the operator's buffers
    rows = []
    for _ in range(runs):
        t = time.perf_counter()
        st = fn()
        rows.append(((time.perf_counter() - t) * 1e3, st))
    rows.sort(key=lambda r: r[0])
    return rows[len(rows) // 2]  # the median call and what it returned


def _sids_of_subset(all_ids, ids):
    """sid of every id of `ids`, an ascending subset of all_ids"""
    n, k = len(all_ids), len(ids)
    hi = np.concatenate((all_ids["hi"], ids["hi"]))
    lo = np.concatenate((all_ids["lo"], ids["lo"]))
    tag = np.concatenate((np.zeros(n, dtype=np.int8), np.ones(k, dtype=np.int8)))
    order = np.lexsort((tag, lo, hi))
    sub = tag[order] == 1
    return (np.cumsum(~sub) - 1)[sub].astype(np.int64)


def _host_order(key):
    """ord[sid] = position of the node in the sort by (key, sid)"""
    order = np.lexsort((np.arange(len(key)), key))
    ord_of = np.empty(len(key), dtype=np.uint32)
    ord_of[order] = np.arange(len(key), dtype=np.uint32)
    return ord_of, order.astype(np.uint32)


def _host_route(rp, src, ord_of, inv, key, qsids, limit):
    """the lists of qsids as (offsets, sids, keys, degrees)"""
    lists, degrees = [], np.zeros(len(qsids), dtype=np.uint64)
    for i, v in enumerate(qsids.tolist()):
        frm = src[rp[v]:rp[v + 1]]
        o = ord_of[frm[frm != v]]
        degrees[i] = len(o)
        if len(o) > limit:
            o = o[np.argpartition(o, limit - 1)[:limit]]
        lists.append(np.sort(o))
    offsets = np.zeros(len(qsids) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in lists])
    sids = inv[np.concatenate(lists)] if lists else np.zeros(0, dtype=np.uint32)
    return offsets, sids, key[sids], degrees


def bench_config(name, runs, seed):
    g, scale, label = synth.make_config(name)
    out = dict(config=name, label=label, n=int(g.n), m=int(g.m))
    rng = np.random.default_rng(seed)
    ids = np.ascontiguousarray(g.ids)
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        try:
            _, rp, src = ctx.graph()
            out["host_csr"] = "hb_debug_copy_graph"
        except _lib.HyperballError:
            rp, src = g.row_ptr, g.src
            out["host_csr"] = "the arrays the graph was loaded from (the library keeps no host copy at this size)"
        rp, src = np.asarray(rp, dtype=np.int64), np.asarray(src)
        ctx.run()
        rids, _ = ctx.results()
        key = np.full(g.n, U64_MAX, dtype=np.uint64)
        key[_sids_of_subset(ids, rids)] = ctx.ranks()
        ms, st = _median(lambda: ctx.links_set_keys(from_ranks=True), runs)
        out["set_keys_from_ranks"] = dict(ms=ms, ms_order=st["ms_order"], listed=int(st["listed"]), device_bytes=int(st["device_bytes"]))
        ms_list, st = _median(lambda: ctx.links_set_keys(ids, key), runs)
        out["set_keys_from_a_list_of_n"] = dict(ms=ms_list, ms_order=st["ms_order"])
        t = time.perf_counter()
        ord_of, inv = _host_order(key)
        out["host_order_lexsort_ms"] = (time.perf_counter() - t) * 1e3
        indeg = np.diff(rp)
        batches = {"hubs": np.argsort(-indeg, kind="stable")[:1024], "random": rng.choice(g.n, min(1024, g.n), replace=False)}
        out["batches"] = []
        for which, qsids in batches.items():
            qids = ids[qsids]
            for limit in (128, 512):
                def device():
                    s = ctx.backlinks(qids, limit)
                    return s, ctx.links_copy()
                ms, (st, res) = _median(device, runs)
                ms_host, want = _median(lambda: _host_route(rp, src, ord_of, inv, key, qsids, limit), runs)
                same = (np.array_equal(res[0], want[0]) and res[1].tobytes() == np.ascontiguousarray(ids[want[1]]).tobytes()
                        and np.array_equal(res[2], want[2]) and np.array_equal(res[3], want[3]))
                rec = dict(batch=which, queries=len(qsids), limit=limit, ms=ms, ms_expand=st["ms_expand"], ms_select=st["ms_select"], ms_emit=st["ms_emit"],
                           entries_gathered=int(st["edges_gathered"]), entries_gathered_per_s=st["edges_gathered"] / (ms * 1e-3),
                           entries_written=int(st["entries"]), rows_walked=int(st["rows_walked"]), selected=int(st["selected"]),
                           batches=int(st["batches"]), device_bytes=int(st["device_bytes"]), host_ms=ms_host,
                           host_entries_gathered_per_s=st["edges_gathered"] / (ms_host * 1e-3), host_over_device=ms_host / ms, equal_to_host_route=bool(same))
                out["batches"].append(rec)
                print(json.dumps(dict(config=name, **rec)), flush=True)
                if not same:
                    sys.exit("links_bench: the device lists differ from the host route's")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--runs", type=int, default=5, help="timed calls per measurement (median), after one warm-up call")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if _lib.device_count() == 0:
        sys.exit("links_bench: no GPU (timings are taken on the device only)")
    res = dict(tool="tools/links_bench.py", runs=args.runs, seed=args.seed,
               results=[bench_config(c, args.runs, args.seed) for c in args.configs.split(",")])
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "results"}))


if __name__ == "__main__":
    main()
