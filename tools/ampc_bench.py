#!/usr/bin/env python3
"""Throughput of the AMPC counter shard (include/hb_ampc.h) with its DEVICE key index (round 5; VERDICT r4 #8: "report upserts/s
at 10 M keys"): batch_set of K distinct keys (every pair inserts), batch_upsert of random pairs over those keys (every pair finds
its slot, the pairs of one key applied in batch order), batch_get; from pageable numpy buffers (what the ctypes mirror hands
over) and from page-locked ones (hb_pinned_alloc: what a worker that owns its receive buffers would use).  Semantics:
crates/core/src/ampc/dht/upsert.rs:66-89, dht/store.rs:159-190; driver: entrypoint/ampc/harmonic_centrality/mapper.rs:52-118.
--values adds the scalar value tables in the same process (the counter table's rate above is their comparator): per kind / operator (or
the one of --kind / --op) the set, get and upsert rates on uniformly drawn keys and the time of a HOT-KEY batch - one key takes half of
every batch, the shape a shortest-path round sends to a hub - over the time of a uniform one.  --centralities adds
hbu_update_centralities on four tables of that many keys against the host route it replaces: two batch_gets of counters,
HyperLogLog::size() on the host (the CPU oracle's, called per counter from Python: its time is reported on its own), the Kahan sums,
one batch_set.  --edges adds the two edge steps, hbu_update_counters and hbu_update_distances, between two tables of that many keys
against the host route built from the calls that were there before them - batch_get + batch_upsert for the counters, batch_get_values +
batch_upsert_values(U64_MIN) on the per-destination minima for the distances; the host's own add / minimum is NOT timed, so the
comparator is its link-and-device part alone - on uniformly drawn destinations and on batches half of which go to one destination,
both sides alternating, median / minimum / maximum of --reps batches each.  --rounds adds the resident worker: a graph of
--round-edges R-MAT edges (stract_amd/synth.py, stream order) and a bloom filter next to tables of that many keys, one
hbu_round_counters, hbu_round_distances and hbu_round_centralities per repetition at three filter densities (filled, about 10 % and
about 0.1 % of the nodes inserted) against the route of the calls that were there before - hbu_update_counters / hbu_update_distances /
hbu_update_centralities fed from page-locked host ids in batches of `pairs per batch`; only the time inside those calls counts for the
comparator, the host's own filtering and filter update are timed once per density and reported beside it.  --only-rounds skips the
counter-table section.  --approx adds the approximated-harmonic job: hbu_fold_harmonic against the route of the calls that were there before
it, in the same process (batch_get_values of every key of the distance table, the terms in numpy - not timed -, batch_upsert_values(KAHAN_ADD),
page-locked buffers, only the time inside the calls) into a centrality table of that many keys from distance tables of 100 %, 10 % and 0.1 %
of them, every key present and half of them absent; hbu_export of a table of every kind; and whole sources of run_approx_harmonic_job's loop
on the --rounds R-MAT worker graph with max_distance = 5, with the fold's share of a source.  --only-approx skips the counter-table section.
--lanes adds, on the same worker graph with max_distance = 5, 64 sampled sources through the per-source route (run_shortest_path_job +
fold_harmonic each) and through one 64-lane walk (run_shortest_paths_job + fold_harmonic_lanes), alternating in this process, a warm-up and
--reps timed repetitions with the folds included and the two results compared bit for bit; and the round call alone,
hbu_round_lane_distances against hbu_round_distances, on the state each job holds after each of its rounds.  --only-lanes skips the
counter-table section.  --finish adds the finish of a job: finish_centralities, top_centralities(1 000 000) and store_centralities (into a
memory file system) against today's route in the same process - items(), the division and np.lexsort in numpy, hb_store_harmonic on the host
arrays -, alternating, a warm-up in which the two routes' outputs are compared and --reps timed repetitions, on the centrality table one
64-lane walk of --lanes leaves and on a synthetic KahanSum table of `keys` keys.  --only-finish skips the counter-table section.
--out FILE also writes the JSON line there.
usage: tools/ampc_bench.py [keys, default 10000000] [pairs per batch, default 1000000] [--values] [--kind K] [--op OP] [--centralities]
                           [--edges] [--rounds] [--round-edges N, default 100000000] [--round-scale S] [--only-rounds] [--approx] [--only-approx]
                           [--sources N, default 5] [--lanes] [--only-lanes] [--finish] [--only-finish] [--reps N, default 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stract_amd import _lib, ampc  # noqa: E402


KINDS = {"u64": ampc.KIND_U64, "f32": ampc.KIND_F32, "f64": ampc.KIND_F64, "kahan": ampc.KIND_KAHAN}
OP_NAMES = {"u64_add": ampc.OP_U64_ADD, "u64_min": ampc.OP_U64_MIN, "f32_add": ampc.OP_F32_ADD, "f64_add": ampc.OP_F64_ADD, "kahan_add": ampc.OP_KAHAN_ADD}


def random_values(rng, kind, n):
    if kind == ampc.KIND_U64:
        return rng.integers(0, 1 << 40, n, dtype=np.uint64)
    if kind == ampc.KIND_KAHAN:
        v = np.zeros(n, dtype=ampc.KAHAN)
        v["sum"] = rng.random(n) * 1e6
        return v
    return (rng.random(n) * 1e6).astype(ampc.DTYPES[kind])


def timed(fn):
    t0 = time.perf_counter()
    fn()  # (every call of the table ends in a stream synchronise)
    return time.perf_counter() - t0


def values_mode(rng, keys, K, B, kind, op):
    """set / get / upsert rates of one scalar kind and operator from page-locked buffers, uniform and hot-key batches alternating"""
    dtype = ampc.DTYPES[kind]
    kb, vb = _lib.PinnedRecords(B, dtype=_lib.U128), _lib.PinnedRecords(B, dtype=dtype)
    kbuf, vbuf = kb.array, vb.array
    vbuf[:] = random_values(rng, kind, B)
    acts, found, gout = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=dtype)
    rounds = max(K // B, 1)
    with ampc.ValueTable(kind, capacity_hint=K) as tab:
        lib, h = tab.lib, tab.h
        t_set = t_up = t_hot = t_get = 0.0
        for b in range(0, K, B):
            n = min(B, K - b)
            kbuf[:n] = keys[b:b + n]
            t_set += timed(lambda: tab._check(lib.hbu_batch_set_values(h, _lib._ptr(kbuf), _lib._ptr(vbuf), n)))
        assert len(tab) == K
        for shape in ["warm_uniform", "warm_hot"] + ["uniform", "hot"] * rounds:  # alternating: both see the same machine
            idx = rng.integers(0, K, B)
            if shape.endswith("hot"):
                idx[rng.random(B) < 0.5] = 12345 % K  # one key takes half of the batch, spread over it
            kbuf[:] = keys[idx]
            t = timed(lambda: tab._check(lib.hbu_batch_upsert_values(h, op, _lib._ptr(kbuf), _lib._ptr(vbuf), B, _lib._ptr(acts))))
            if shape == "uniform":
                t_up += t
            elif shape == "hot":
                t_hot += t
        for r in range(rounds):
            kbuf[:] = keys[rng.integers(0, K, B)]
            t_get += timed(lambda: tab._check(lib.hbu_batch_get_values(h, _lib._ptr(kbuf), B, _lib._ptr(gout), _lib._ptr(found))))
        assert found.all() and len(tab) == K
    kb.close()
    vb.close()
    pair_bytes = 16 + dtype.itemsize + 1
    return {"bytes_per_pair": pair_bytes, "batch_set_inserting_Mpairs_per_s": round(K / t_set / 1e6, 2),
            "batch_upsert_Mpairs_per_s": round(rounds * B / t_up / 1e6, 2), "batch_upsert_hot_key_Mpairs_per_s": round(rounds * B / t_hot / 1e6, 2),
            "hot_over_uniform_batch_time": round(t_hot / t_up, 3), "upsert_link_GBs": round(rounds * B * pair_bytes / t_up / 1e9, 2),
            "batch_get_Mkeys_per_s": round(rounds * B / t_get / 1e6, 2)}


def centralities_mode(rng, keys, K, B, host_batches=2):
    """hbu_update_centralities over four tables of K keys in batches of B nodes, and the host route for the first host_batches of them"""
    from oracle import hbo
    regs = rng.integers(0, 30, (B, 64), dtype=np.uint8)
    more = rng.integers(0, 32, (B, 64), dtype=np.uint8)
    acts = np.zeros(B, dtype=np.uint8)
    res = {}
    with ampc.CounterTable(capacity_hint=K) as prev_c, ampc.ValueTable(ampc.KIND_KAHAN, capacity_hint=K) as prev_v:
        for b in range(0, K, B):
            n = min(B, K - b)
            prev_c.batch_set(keys[b:b + n], regs[:n])
            prev_v.batch_set(keys[b:b + n], random_values(rng, ampc.KIND_KAHAN, n))
        t_clone = timed(lambda: res.setdefault("t", (prev_c.clone(), prev_v.clone())))
        next_c, next_v = res.pop("t")
        res["clone_counters_and_centrality_s"] = round(t_clone, 4)
        res["clone_GBs"] = round(K * (64 + 16 + 2 * 2 * 20) / t_clone / 1e9, 1)  # values + the index (2 x 20 B per key at load factor 1/2)
        for b in range(0, K, B):                      # a round's update_counters: about half of the counters grow
            n = min(B, K - b)
            next_c.batch_upsert(keys[b:b + n], more[:n])
        with next_c, next_v:
            ampc.update_centralities(prev_c, next_c, prev_v, next_v, keys[:B], 0)  # warm-up (the estimator tables go up here)
            t_dev, written = 0.0, 0
            for b in range(0, K, B):
                nodes = keys[b:b + B]
                t0 = time.perf_counter()
                written += ampc.update_centralities(prev_c, next_c, prev_v, next_v, nodes, 1)
                t_dev += time.perf_counter() - t0
            res["update_centralities_Mnodes_per_s"] = round(K / t_dev / 1e6, 2)
            res["written_share"] = round(written / K, 3)
            t_link = t_size = t_kahan = 0.0
            done = 0
            for b in range(0, min(K, host_batches * B), B):
                nodes = keys[b:b + B]
                t0 = time.perf_counter()
                old_c, _ = prev_c.batch_get(nodes)
                new_c, _ = next_c.batch_get(nodes)
                old_v, _ = prev_v.batch_get(nodes)
                t1 = time.perf_counter()
                d = hbo.hll_sizes(new_c).astype(np.int64) - hbo.hll_sizes(old_c).astype(np.int64)
                t2 = time.perf_counter()
                sel = d > 0
                rhs = d[sel].astype(np.float64) / 2.0
                y = rhs - old_v["err"][sel]
                t = old_v["sum"][sel] + y
                val = np.zeros(int(sel.sum()), dtype=ampc.KAHAN)
                val["sum"], val["err"] = t, (t - old_v["sum"][sel]) - y
                t3 = time.perf_counter()
                next_v.batch_set(nodes[sel], val)
                t4 = time.perf_counter()
                t_link += (t1 - t0) + (t4 - t3)
                t_size += t2 - t1
                t_kahan += t3 - t2
                done += len(nodes)
            res["host_route_Mnodes_per_s"] = round(done / (t_link + t_size + t_kahan) / 1e6, 3)
            res["host_route_link_only_Mnodes_per_s"] = round(done / t_link / 1e6, 2)  # the gets and the set alone: 64 + 64 + 16 B down, 32 B up per node
            res["host_route_seconds_per_Mnodes"] = {"gets_and_set": round(t_link / done * 1e6, 3), "sizes_on_host": round(t_size / done * 1e6, 3),
                                                    "kahan_on_host": round(t_kahan / done * 1e6, 3)}
    return res


def spread(times):
    t = sorted(times)
    return {"median_s": round(t[len(t) // 2] if len(t) % 2 else (t[len(t) // 2 - 1] + t[len(t) // 2]) / 2, 6), "min_s": round(t[0], 6), "max_s": round(t[-1], 6)}


def edges_mode(rng, keys, K, B, reps):
    """hbu_update_counters / hbu_update_distances against the host route (see the module's docstring); every buffer that crosses the link
    is page-locked on both sides"""
    fb, tb, ub = (_lib.PinnedRecords(B, dtype=_lib.U128) for _ in range(3))
    cb = _lib.PinnedRecords(B * 64, dtype=np.uint8)
    vb = _lib.PinnedRecords(B, dtype=np.uint64)
    ab, db = _lib.PinnedRecords(B, dtype=np.uint8), _lib.PinnedRecords(B, dtype=np.uint8)
    fbuf, tbuf, ubuf, cbuf, vbuf, acts, found = fb.array, tb.array, ub.array, cb.array, vb.array, ab.array, db.array
    written = np.zeros(1, dtype=np.uint64)
    shapes = ["warm_uniform", "warm_hot"] + ["uniform", "hot"] * reps  # alternating: both shapes and both sides see the same machine

    def draw(shape):
        fi, ti = rng.integers(0, K, B), rng.integers(0, K, B)
        if shape.endswith("hot"):
            ti[rng.random(B) < 0.5] = 12345 % K  # one destination takes half of the batch, spread over it
        return fi, ti

    def summary(times, link_dev, link_host):
        out = {}
        for shape in ("uniform", "hot"):
            dev, host = spread(times[shape, "device"]), spread(times[shape, "host"])
            gap = max(dev["max_s"] - dev["min_s"], host["max_s"] - host["min_s"])
            out[shape] = {"device_call": dev, "host_route": host, "host_over_device_median": round(host["median_s"] / dev["median_s"], 3),
                          "median_gain_s": round(host["median_s"] - dev["median_s"], 6), "larger_spread_s": round(gap, 6),
                          "device_Medges_per_s": round(B / dev["median_s"] / 1e6, 2), "host_route_Medges_per_s": round(B / host["median_s"] / 1e6, 2)}
        out["hot_over_uniform_batch_time"] = {side: round(out["hot"][name]["median_s"] / out["uniform"][name]["median_s"], 3)
                                              for side, name in (("device", "device_call"), ("host", "host_route"))}
        out["link_bytes_per_edge"] = {"device": link_dev, "host_route": link_host}
        return out

    res = {"edges_per_batch": B, "repetitions": reps}
    # ---- the counter job: 32 B up + 1 B down per edge against 16 up + 64 down, 80 up + 1 down
    regs = rng.integers(0, 30, (B, 64), dtype=np.uint8)
    with ampc.CounterTable(capacity_hint=K) as prev:
        for b in range(0, K, B):
            n = min(B, K - b)
            prev.batch_set(keys[b:b + n], regs[:n])
        with prev.clone() as next_d, prev.clone() as next_h:
            lib = prev.lib
            times = {(s, side): [] for s in ("uniform", "hot") for side in ("device", "host")}
            for shape in shapes:
                fi, ti = draw(shape)
                fbuf[:], tbuf[:] = keys[fi], keys[ti]
                t_dev = timed(lambda: next_d._check(lib.hbu_update_counters(prev.h, next_d.h, _lib._ptr(fbuf), _lib._ptr(tbuf), B, _lib._ptr(acts))))
                t_host = timed(lambda: prev._check(lib.hbu_batch_get(prev.h, _lib._ptr(fbuf), B, _lib._ptr(cbuf), _lib._ptr(found))))
                # (here the worker adds edge.from to every counter: host work, not timed)
                t_host += timed(lambda: next_h._check(lib.hbu_batch_upsert(next_h.h, _lib._ptr(tbuf), _lib._ptr(cbuf), B, _lib._ptr(acts))))
                if not shape.startswith("warm"):
                    times[shape, "device"].append(t_dev)
                    times[shape, "host"].append(t_host)
            assert len(next_d) == K and len(next_h) == K
            res["update_counters"] = summary(times, 33, 161)
    # ---- the distance job: 32 B up per edge + 17 B down per destination against 16 + 8 per distinct source, 24 + 1 per destination
    with ampc.ValueTable(ampc.KIND_U64, capacity_hint=K) as prev:
        for b in range(0, K, B):
            n = min(B, K - b)
            prev.batch_set(keys[b:b + n], rng.integers(0, 1 << 20, n, dtype=np.uint64))
        with prev.clone() as next_d, prev.clone() as next_h:
            lib = prev.lib
            times = {(s, side): [] for s in ("uniform", "hot") for side in ("device", "host")}
            sources = dests = 0
            for shape in shapes:
                fi, ti = draw(shape)
                fbuf[:], tbuf[:] = keys[fi], keys[ti]
                t_dev = timed(lambda: next_d._check(lib.hbu_update_distances(prev.h, next_d.h, _lib._ptr(fbuf), _lib._ptr(tbuf), B, _lib._ptr(ubuf), _lib._ptr(acts),
                                                                             written.ctypes.data_as(lib.hbu_update_distances.argtypes[7]))))
                us, inv = np.unique(fi, return_inverse=True)  # the worker asks for every source once
                ubuf[:len(us)] = keys[us]
                ns = len(us)
                t_host = timed(lambda: prev._check(lib.hbu_batch_get_values(prev.h, _lib._ptr(ubuf), ns, _lib._ptr(vbuf), _lib._ptr(found))))
                cand = vbuf[:ns][inv] + np.uint64(1)          # host work, not timed: the candidates and their minimum per destination
                ud, dinv = np.unique(ti, return_inverse=True)
                best = np.full(len(ud), np.iinfo(np.uint64).max, dtype=np.uint64)
                np.minimum.at(best, dinv, cand)
                nd = len(ud)
                assert nd == int(written[0])
                ubuf[:nd], vbuf[:nd] = keys[ud], best
                t_host += timed(lambda: next_h._check(lib.hbu_batch_upsert_values(next_h.h, ampc.OP_U64_MIN, _lib._ptr(ubuf), _lib._ptr(vbuf), nd, _lib._ptr(acts))))
                if not shape.startswith("warm"):
                    times[shape, "device"].append(t_dev)
                    times[shape, "host"].append(t_host)
                    sources, dests = sources + ns, dests + nd
            res["update_distances"] = summary(times, round(32 + 17 * dests / (2 * reps * B), 1), round((24 * sources + 25 * dests) / (2 * reps * B), 1))
            res["update_distances"]["distinct_sources_per_edge"] = round(sources / (2 * reps * B), 3)
            res["update_distances"]["distinct_destinations_per_edge"] = round(dests / (2 * reps * B), 3)
            check = keys[rng.integers(0, K, min(B, 100000))]   # both routes leave the same table
            assert np.array_equal(next_d.batch_get(check)[0], next_h.batch_get(check)[0])
    for x in (fb, tb, ub, cb, vb, ab, db):
        x.close()
    return res


def rounds_mode(rng, K, B, reps, total_edges, scale):
    """the resident worker's round calls against the host-fed route of the parent's calls (see the module's docstring)"""
    from stract_amd import synth
    t0 = time.perf_counter()
    g = synth.RmatGraph(scale, total_edges)
    E = g.stream_len(0)
    from_ids, to_ids = np.zeros(E, dtype=_lib.U128), np.zeros(E, dtype=_lib.U128)
    at = 0
    for slab in g.stream():
        from_ids[at:at + len(slab)], to_ids[at:at + len(slab)] = slab["from"], slab["to"]
        at += len(slab)
    nodes = np.array(g.ids)
    n = len(nodes)
    g.close()
    keys = nodes
    if n < K:  # the shard holds K keys: the graph's nodes and others
        extra = np.zeros(K - n, dtype=_lib.U128)
        extra["lo"], extra["hi"] = rng.integers(0, 1 << 63, K - n, dtype=np.uint64), np.uint64(1 << 62)
        keys = np.concatenate([nodes, extra])
    print("graph: %d nodes, %d edges, %.1f s" % (n, E, time.perf_counter() - t0), file=sys.stderr, flush=True)
    num_bits = ampc.bloom_num_bits(n, 0.05)
    prime = np.uint64(11400714819323198549)

    def slots(ids):
        return (ids["lo"] * prime) % np.uint64(num_bits)

    fb, tb, ub = (_lib.PinnedRecords(B, dtype=_lib.U128) for _ in range(3))
    ab = _lib.PinnedRecords(B, dtype=np.uint8)
    fbuf, tbuf, ubuf, acts = fb.array, tb.array, ub.array, ab.array
    written = np.zeros(1, dtype=np.uint64)
    res = {"nodes": n, "edges": E, "keys": len(keys), "bloom_num_bits": num_bits, "host_batch": B, "repetitions": reps, "densities": {}}
    regs = rng.integers(0, 30, (B, 64), dtype=np.uint8)
    more = rng.integers(0, 32, (B, 64), dtype=np.uint8)
    with ampc.WorkerGraph(nodes, from_ids, to_ids) as graph, ampc.ChangedFilter.bloom(num_bits) as changed, ampc.ChangedFilter.bloom(num_bits) as new, \
            ampc.CounterTable(capacity_hint=len(keys)) as prev_c, ampc.ValueTable(ampc.KIND_U64, capacity_hint=len(keys)) as prev_d, \
            ampc.ValueTable(ampc.KIND_KAHAN, capacity_hint=len(keys)) as prev_v:
        for b in range(0, len(keys), B):
            m = min(B, len(keys) - b)
            prev_c.batch_set(keys[b:b + m], regs[:m])
            prev_d.batch_set(keys[b:b + m], rng.integers(0, 1 << 20, m, dtype=np.uint64))
        with prev_c.clone() as grown:  # the counters a centrality step compares with: about half of them grew
            for b in range(0, len(keys), B):
                m = min(B, len(keys) - b)
                grown.batch_upsert(keys[b:b + m], more[:m])
            lib = prev_c.lib
            for label, share in (("all_changed", None), ("about_10_percent", 0.1), ("about_0.1_percent", 0.001)):
                changed.clear()
                if share is None:
                    changed.fill()
                else:
                    changed.insert(nodes[rng.random(n) < share])
                bits = np.unpackbits(changed.export_bits().view(np.uint8), bitorder="little")
                t0 = time.perf_counter()
                edge_mask = bits[slots(from_ids)].astype(bool)
                t_filter_edges = time.perf_counter() - t0
                t0 = time.perf_counter()
                node_mask = bits[slots(nodes)].astype(bool)
                t_filter_nodes = time.perf_counter() - t0
                sel_from, sel_to, sel_nodes = from_ids[edge_mask], to_ids[edge_mask], nodes[node_mask]
                S = len(sel_from)
                t = {k: [] for k in ("counters_device", "counters_host", "distances_device", "distances_host", "centralities_device", "centralities_host")}
                t_update = 0.0
                for r in range(reps + 1):  # the first repetition warms both sides up
                    with prev_c.clone() as next_d, prev_c.clone() as next_h:
                        new.clear()
                        t_dev = timed(lambda: res.__setitem__("_c", ampc.round_counters(prev_c, next_d, graph, changed, new)))
                        t_host, merged_to = 0.0, []
                        for b in range(0, S, B):
                            m = min(B, S - b)
                            fbuf[:m], tbuf[:m] = sel_from[b:b + m], sel_to[b:b + m]
                            t_host += timed(lambda: next_h._check(lib.hbu_update_counters(prev_c.h, next_h.h, _lib._ptr(fbuf), _lib._ptr(tbuf), m, _lib._ptr(acts))))
                            merged_to.append(tbuf[:m][acts[:m] == ampc.MERGED])
                        t0 = time.perf_counter()
                        host_new = np.zeros(num_bits, dtype=np.uint8)
                        if merged_to:
                            host_new[slots(np.concatenate(merged_to))] = 1
                        t_update = time.perf_counter() - t0
                        assert res["_c"][0] == S and new.count() == int(host_new.sum())
                    with prev_d.clone() as next_d, prev_d.clone() as next_h:
                        new.clear()
                        t_dev2 = timed(lambda: res.__setitem__("_d", ampc.round_distances(prev_d, next_d, graph, changed, new)))
                        t_host2, dests = 0.0, 0
                        for b in range(0, S, B):
                            m = min(B, S - b)
                            fbuf[:m], tbuf[:m] = sel_from[b:b + m], sel_to[b:b + m]
                            t_host2 += timed(lambda: next_h._check(lib.hbu_update_distances(prev_d.h, next_h.h, _lib._ptr(fbuf), _lib._ptr(tbuf), m, _lib._ptr(ubuf), _lib._ptr(acts),
                                                                                            written.ctypes.data_as(lib.hbu_update_distances.argtypes[7]))))
                            dests += int(written[0])
                        assert res["_d"][0] == S
                    with prev_v.clone() as next_d, prev_v.clone() as next_h:
                        t_dev3 = timed(lambda: res.__setitem__("_v", ampc.round_centralities(prev_c, grown, prev_v, next_d, graph, changed, 1)))
                        t_host3 = 0.0
                        for b in range(0, len(sel_nodes), B):
                            m = min(B, len(sel_nodes) - b)
                            fbuf[:m] = sel_nodes[b:b + m]
                            t_host3 += timed(lambda: next_h._check(lib.hbu_update_centralities(prev_c.h, grown.h, prev_v.h, next_h.h, _lib._ptr(fbuf), m, 1,
                                                                                               written.ctypes.data_as(lib.hbu_update_centralities.argtypes[7]))))
                        assert res["_v"][0] == len(sel_nodes) and len(next_d) == len(next_h)
                    if r:
                        for k, v in (("counters_device", t_dev), ("counters_host", t_host), ("distances_device", t_dev2), ("distances_host", t_host2),
                                     ("centralities_device", t_dev3), ("centralities_host", t_host3)):
                            t[k].append(v)
                d = {"selected_edges": S, "selected_edge_share": round(S / max(E, 1), 5), "selected_nodes": len(sel_nodes),
                     "host_filtering_s": {"edges": round(t_filter_edges, 4), "nodes": round(t_filter_nodes, 4), "filter_update": round(t_update, 4)},
                     "counts": {"round_counters": list(res.pop("_c")), "round_distances": list(res.pop("_d")), "round_centralities": list(res.pop("_v"))}}
                for job in ("counters", "distances", "centralities"):
                    dev, host = spread(t[job + "_device"]), spread(t[job + "_host"])
                    d["round_" + job] = {"device_call": dev, "host_fed_library_time": host, "median_gain_s": round(host["median_s"] - dev["median_s"], 6),
                                         "larger_spread_s": round(max(dev["max_s"] - dev["min_s"], host["max_s"] - host["min_s"]), 6),
                                         "device_walks_Medges_per_s": round((E if job != "centralities" else n) / dev["median_s"] / 1e6, 1)}
                # device: one 4-byte count per chunk of the default 2^22 edges and 32 bytes of counts per call; host: ids up, actions (and keys) back
                d["link_bytes_per_selected_edge"] = {"device": round((4 * -(-E // (1 << 22)) + 32) / max(S, 1), 6), "host_route_counters": 33,
                                                     "host_route_distances": round(32 + 17 * dests / max(S, 1), 1)}
                res["densities"][label] = d
                print(label, d, file=sys.stderr, flush=True)
    for x in (fb, tb, ub, ab):
        x.close()
    return res


def rmat_worker(scale, total_edges):
    """the R-MAT worker graph of --rounds: (nodes, from_ids, to_ids), edges in stream order"""
    from stract_amd import synth
    g = synth.RmatGraph(scale, total_edges)
    E = g.stream_len(0)
    from_ids, to_ids = np.zeros(E, dtype=_lib.U128), np.zeros(E, dtype=_lib.U128)
    at = 0
    for slab in g.stream():
        from_ids[at:at + len(slab)], to_ids[at:at + len(slab)] = slab["from"], slab["to"]
        at += len(slab)
    nodes = np.array(g.ids)
    g.close()
    return nodes, from_ids, to_ids


def approx_mode(rng, keys, K, reps, total_edges, scale, n_sources):
    """hbu_fold_harmonic against the composed route, hbu_export, and whole sources of the approximated-harmonic loop (see the module's docstring)"""
    res = {"repetitions": reps, "fold": {}, "export": {}}
    norm = 1.0 / 2657.0
    kb, db, pb, ab, fb = (_lib.PinnedRecords(K, dtype=_lib.U128), _lib.PinnedRecords(K, dtype=np.uint64), _lib.PinnedRecords(K, dtype=ampc.KAHAN),
                          _lib.PinnedRecords(K, dtype=np.uint8), _lib.PinnedRecords(K, dtype=np.uint8))
    kbuf, dbuf, pbuf, acts, found = kb.array, db.array, pb.array, ab.array, fb.array
    fresh = np.zeros(K, dtype=_lib.U128)  # keys the centrality table does not hold
    fresh["lo"], fresh["hi"] = np.arange(K, dtype=np.uint64) * np.uint64(0xD6E8FEB86659FD93) + np.uint64(7), np.uint64((1 << 63) + 5)
    folded, inserted = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    with ampc.ValueTable(ampc.KIND_KAHAN, capacity_hint=K) as base:
        lib = base.lib
        u64p = lib.hbu_fold_harmonic.argtypes[4]
        for b in range(0, K, 1_000_000):
            base.batch_set(keys[b:b + 1_000_000], random_values(rng, ampc.KIND_KAHAN, len(keys[b:b + 1_000_000])))
        for share in (1.0, 0.1, 0.001):
            n = max(int(K * share), 1)
            for label, absent in (("all_present", 0), ("half_absent", n // 2)):
                ids = np.concatenate([keys[rng.permutation(K)[:n - absent]], fresh[:absent]])
                rng.shuffle(ids)
                kbuf[:n] = ids
                with ampc.ValueTable(ampc.KIND_U64, capacity_hint=n) as dist:
                    dist.batch_set(ids, rng.integers(1, 8, n, dtype=np.uint64))
                    t_dev, t_host, t_get, t_up = [], [], [], []
                    for r in range(reps + 1):  # the first repetition warms both sides up; both start from a fresh copy every time
                        with base.clone() as cent_d, base.clone() as cent_h:
                            td = timed(lambda: cent_d._check(lib.hbu_fold_harmonic(dist.h, cent_d.h, norm, 0, folded.ctypes.data_as(u64p), inserted.ctypes.data_as(u64p))))
                            assert (int(folded[0]), int(inserted[0])) == (n, absent)
                            tg = timed(lambda: dist._check(lib.hbu_batch_get_values(dist.h, _lib._ptr(kbuf), n, _lib._ptr(dbuf), _lib._ptr(found))))
                            pbuf["sum"][:n] = (1.0 / dbuf[:n].astype(np.float64)) * norm  # host work, not timed
                            pbuf["err"][:n] = 0.0
                            tu = timed(lambda: cent_h._check(lib.hbu_batch_upsert_values(cent_h.h, ampc.OP_KAHAN_ADD, _lib._ptr(kbuf), _lib._ptr(pbuf), n, _lib._ptr(acts))))
                            if r == reps:  # both routes leave the same table
                                check = ids[rng.integers(0, n, min(n, 100000))]
                                a, b2 = cent_d.batch_get(check)[0], cent_h.batch_get(check)[0]
                                assert np.array_equal(a.view(np.uint64), b2.view(np.uint64)) and len(cent_d) == len(cent_h) == K + absent
                        if r:
                            t_dev.append(td)
                            t_host.append(tg + tu)
                            t_get.append(tg)
                            t_up.append(tu)
                dev, host = spread(t_dev), spread(t_host)
                gap = max(dev["max_s"] - dev["min_s"], host["max_s"] - host["min_s"])
                cell = {"entries": n, "absent": absent, "fold_harmonic": dev, "composed_route": host, "composed_batch_get": spread(t_get),
                        "composed_batch_upsert": spread(t_up), "median_gain_s": round(host["median_s"] - dev["median_s"], 6), "larger_spread_s": round(gap, 6),
                        "beats_by_more_than_the_spread": bool(host["median_s"] - dev["median_s"] > gap),
                        "fold_Mentries_per_s": round(n / dev["median_s"] / 1e6, 1), "composed_Mentries_per_s": round(n / host["median_s"] / 1e6, 1),
                        "link_bytes_per_entry": {"fold_harmonic": 0, "composed_route": 16 + 9 + 32 + 1}}
                res["fold"]["%g_percent_%s" % (share * 100, label)] = cell
                print("fold", share, label, cell, file=sys.stderr, flush=True)
    for x in (db, pb, ab, fb):
        x.close()
    # ---- hbu_export of K keys, every kind, into page-locked memory
    written = np.zeros(1, dtype=np.uint64)
    for name, kind in [("hll64", ampc.KIND_HLL64)] + sorted(KINDS.items()):
        vbytes = 64 if kind == ampc.KIND_HLL64 else ampc.DTYPES[kind].itemsize
        vb = _lib.PinnedRecords(K * vbytes, dtype=np.uint8)
        with (ampc.CounterTable(capacity_hint=K) if kind == ampc.KIND_HLL64 else ampc.ValueTable(kind, capacity_hint=K)) as tab:
            for b in range(0, K, 1_000_000):
                m = len(keys[b:b + 1_000_000])
                tab.batch_set(keys[b:b + m], rng.integers(0, 40, (m, 64), dtype=np.uint8) if kind == ampc.KIND_HLL64 else random_values(rng, kind, m))
            times = [timed(lambda: tab._check(tab.lib.hbu_export(tab.h, _lib._ptr(kbuf), _lib._ptr(vb.array), K, written.ctypes.data_as(tab.lib.hbu_export.argtypes[4]))))
                     for _ in range(reps + 1)][1:]
            assert int(written[0]) == K
        sp = spread(times)
        res["export"][name] = dict(sp, value_bytes=vbytes, Mkeys_per_s=round(K / sp["median_s"] / 1e6, 1), GBs=round(K * (16 + vbytes) / sp["median_s"] / 1e9, 2))
        print("export", name, res["export"][name], file=sys.stderr, flush=True)
        vb.close()
    kb.close()
    # ---- whole sources: the shortest-path job with max_distance = 5, then the fold
    t0 = time.perf_counter()
    nodes, from_ids, to_ids = rmat_worker(scale, total_edges)
    print("graph: %d nodes, %d edges, %.1f s" % (len(nodes), len(from_ids), time.perf_counter() - t0), file=sys.stderr, flush=True)
    out_deg_sources = np.unique(from_ids[rng.integers(0, len(from_ids), 4 * n_sources + 4)])  # sources with out-links, as random_page_nodes_with_outgoing picks
    sources = [(int(k["hi"]) << 64) | int(k["lo"]) for k in out_deg_sources[:n_sources + 1]]
    per = []
    with ampc.WorkerGraph(nodes, from_ids, to_ids) as graph, ampc.ValueTable(ampc.KIND_KAHAN) as cent:
        t0 = time.perf_counter()
        sketch = graph.node_sketch()
        t_sketch = time.perf_counter() - t0
        t_sketch = min(t_sketch, timed(graph.node_sketch))
        for i, source in enumerate(sources):  # the first source warms up
            t0 = time.perf_counter()
            dist = ampc.run_shortest_path_job([graph], source, 5)
            t1 = time.perf_counter()
            f, ins = ampc.fold_harmonic(dist, cent, norm)
            t2 = time.perf_counter()
            dist.close()
            if i:
                per.append({"walk_s": round(t1 - t0, 6), "fold_s": round(t2 - t1, 6), "reached": f, "inserted": ins})
        t_items = timed(cent.items)
        total_keys = len(cent)
    whole = [p["walk_s"] + p["fold_s"] for p in per]
    share = [p["fold_s"] / (p["walk_s"] + p["fold_s"]) for p in per]
    res["whole_source"] = {"nodes": len(nodes), "edges": len(from_ids), "max_distance": 5, "sources": per, "source": spread(whole),
                           "fold": spread([p["fold_s"] for p in per]), "fold_share_median": round(sorted(share)[len(share) // 2], 5),
                           "fold_share_max": round(max(share), 5), "node_sketch_s": round(t_sketch, 6), "node_sketch_registers_set": int(np.count_nonzero(sketch)),
                           "items_s": round(t_items, 6), "centrality_keys": total_keys}
    print("whole_source", res["whole_source"], file=sys.stderr, flush=True)
    return res


def lanes_mode(rng, reps, total_edges, scale, n_sources=64):
    """64 sampled sources of the approximated-harmonic loop (max_distance = 5, the fold included) through the per-source route
    (run_shortest_path_job + fold_harmonic per source) and through one 64-lane walk (run_shortest_paths_job + fold_harmonic_lanes), in this
    process, alternating, one warm-up and `reps` timed repetitions each; and the round call alone, hbu_round_lane_distances against
    hbu_round_distances, on the tables and filters the two jobs hold after each of their rounds."""
    norm, max_distance = 1.0 / 2657.0, 5
    t0 = time.perf_counter()
    nodes, from_ids, to_ids = rmat_worker(scale, total_edges)
    print("graph: %d nodes, %d edges, %.1f s" % (len(nodes), len(from_ids), time.perf_counter() - t0), file=sys.stderr, flush=True)
    picked = np.unique(from_ids[rng.integers(0, len(from_ids), 4 * n_sources + 4)])  # sources with out-links, as random_page_nodes_with_outgoing picks
    rng.shuffle(picked)
    sources = [(int(k["hi"]) << 64) | int(k["lo"]) for k in picked[:n_sources]]
    res = {"nodes": len(nodes), "edges": len(from_ids), "max_distance": max_distance, "sources": len(sources), "repetitions": reps}

    def result_of(cent):
        keys, values = cent.items()
        order = np.lexsort((keys["lo"], keys["hi"]))
        return keys[order], values[order]

    with ampc.WorkerGraph(nodes, from_ids, to_ids) as graph:
        def per_source(keep):
            with ampc.ValueTable(ampc.KIND_KAHAN) as cent:
                t0 = time.perf_counter()
                for s_ in sources:
                    dist = ampc.run_shortest_path_job([graph], s_, max_distance)
                    ampc.fold_harmonic(dist, cent, norm)
                    dist.close()
                t = time.perf_counter() - t0
                return t, (result_of(cent) if keep else None)

        def one_walk(keep):
            with ampc.ValueTable(ampc.KIND_KAHAN) as cent:
                t0 = time.perf_counter()
                lanes = ampc.run_shortest_paths_job([graph], sources, max_distance)
                t1 = time.perf_counter()
                folded, inserted = ampc.fold_harmonic_lanes(lanes, cent, norm, len(sources))
                t2 = time.perf_counter()
                lanes.close()
                return t2 - t0, t2 - t1, (folded, inserted), (result_of(cent) if keep else None)

        t_old, t_new, t_fold = [], [], []
        for r in range(reps + 1):  # the first repetition warms both routes up and compares their results
            to, old = per_source(r == 0)
            tn, tf, counts, new = one_walk(r == 0)
            if r == 0:
                same = (np.array_equal(old[0], new[0]) and np.array_equal(old[1]["sum"].view(np.uint64), new[1]["sum"].view(np.uint64))
                        and np.array_equal(old[1]["err"].view(np.uint64), new[1]["err"].view(np.uint64)))
                res.update(results_equal_bit_for_bit=bool(same), centrality_keys=len(old[0]), lanes_folded=counts[0], keys_inserted=counts[1])
                assert same, "the two routes differ"
            else:
                t_old.append(to)
                t_new.append(tn)
                t_fold.append(tf)
            print("repetition", r, round(to, 4), round(tn, 4), file=sys.stderr, flush=True)
        old, new = spread(t_old), spread(t_new)
        gap = max(old["max_s"] - old["min_s"], new["max_s"] - new["min_s"])
        res["job_of_64_sources"] = {"per_source_route": old, "one_64_lane_walk": new, "fold_harmonic_lanes": spread(t_fold),
                                    "median_gain_s": round(old["median_s"] - new["median_s"], 6), "larger_spread_s": round(gap, 6),
                                    "beats_by_more_than_the_spread": bool(old["median_s"] - new["median_s"] > gap),
                                    "ratio_of_medians": round(old["median_s"] / new["median_s"], 2)}
        print("job", res["job_of_64_sources"], file=sys.stderr, flush=True)

        # ---- the round call alone: the call the next round makes, repeated on a fresh clone of its `next`
        def time_round(call, state):
            times, counts = [], None
            for r in range(reps + 1):
                with state["next"].clone() as scratch:
                    t0 = time.perf_counter()
                    counts = call(state["next"], scratch, graph, state["filters"][0], None)
                    t = time.perf_counter() - t0
                if r:
                    times.append(t)
            return dict(spread(times), selected=counts[0], filter="exact" if state["filters"][0].kind == ampc.FILTER_EXACT else "bloom")

        single, batch = {}, {}
        ampc.run_shortest_path_job([graph], sources[0], max_distance, on_round=lambda st: single.__setitem__(st["round"] + 1, time_round(ampc.round_distances, st))).close()
        ampc.run_shortest_paths_job([graph], sources, max_distance, on_round=lambda st: batch.__setitem__(st["round"] + 1, time_round(ampc.round_lane_distances, st))).close()
        res["round_call"] = {}
        for rnd in sorted(set(single) & set(batch)):
            a, b = single[rnd], batch[rnd]
            res["round_call"]["round_%d" % rnd] = {"hbu_round_distances_one_source": a, "hbu_round_lane_distances_64_sources": b,
                                                   "lane_call_in_single_calls": round(b["median_s"] / a["median_s"], 2)}
        print("round_call", res["round_call"], file=sys.stderr, flush=True)
    return res


def finish_mode(rng, keys, K, reps, total_edges, scale, n_sources=64):
    """The finish of a job (finish_centralities, top_centralities(1 000 000), store_centralities into a memory file system) against today's
    route in this process - items(), the division in numpy, np.lexsort for the id order, the ranks and the top list, hb_store_harmonic on
    the host arrays -, alternating, one warm-up (in which the outputs of the two routes are compared) and `reps` timed repetitions each; on
    the centrality table one 64-lane walk of --lanes leaves (divisor 1.0, the approximated job's) and on a synthetic KahanSum table of K
    keys (divisor K - 1, the harmonic job's)."""
    import hashlib
    import shutil
    import tempfile
    top_k = 1_000_000
    res = {"repetitions": reps, "top_k": top_k, "tables": {}}
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    scratch = tempfile.mkdtemp(prefix="ampc_finish_", dir=base)
    res["store_directory_is_memory_backed"] = base is not None

    def total_key(vals):
        b = vals.view(np.uint64)
        return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))

    def host_values(tab, divisor):
        k, v = tab.items()
        with np.errstate(all="ignore"):
            return k, v["sum"] / np.float64(divisor)

    def host_finish(tab, divisor):
        k, q = host_values(tab, divisor)
        order = np.lexsort((k["lo"], k["hi"]))
        ids, vals = k[order], q[order]
        by_rank = np.argsort(~total_key(vals), kind="stable")  # (ids ascend: a stable sort leaves ties in id order)
        ranks = np.empty(len(ids), dtype=np.uint64)
        ranks[by_rank] = np.arange(len(ids), dtype=np.uint64)
        return ids, vals, ranks

    def host_top(tab, divisor, k_top):
        k, q = host_values(tab, divisor)
        first = np.lexsort((k["lo"], k["hi"], ~total_key(q)))[:k_top]
        return k[first], q[first]

    def files_of(out):
        found = {}
        for db in sorted(os.listdir(out)):
            for f in sorted(os.listdir(os.path.join(out, db))):
                h = hashlib.sha256()
                with open(os.path.join(out, db, f), "rb") as fh:
                    for block in iter(lambda: fh.read(1 << 24), b""):
                        h.update(block)
                if f != "meta.json":  # (meta.json names the segment: a fresh uuid per store)
                    found[(db, os.path.splitext(f)[1])] = h.hexdigest()
        return found

    def canon(vals):
        b = vals.view(np.uint64).copy()
        b[np.isnan(vals)] = 0x7FF8000000000000
        return b

    def measure(name, tab, divisor):
        n = len(tab)
        t = {x: [] for x in ("finish_dev", "finish_host", "top_dev", "top_host", "store_dev", "store_host", "store_host_writer")}
        same = {}
        for r in range(reps + 1):  # the first repetition warms both routes up and compares their outputs
            t0 = time.perf_counter()
            d = ampc.finish_centralities(tab, divisor)
            t1 = time.perf_counter()
            h = host_finish(tab, divisor)
            t2 = time.perf_counter()
            dt = ampc.top_centralities(tab, top_k, divisor)
            t3 = time.perf_counter()
            ht = host_top(tab, divisor, top_k)
            t4 = time.perf_counter()
            a, b = os.path.join(scratch, "dev"), os.path.join(scratch, "host")
            ampc.store_centralities(tab, a, divisor)
            t5 = time.perf_counter()
            hs = host_finish(tab, divisor)
            t6 = time.perf_counter()
            _lib.store_harmonic(b, *hs)
            t7 = time.perf_counter()
            if r == 0:
                same = {"ids": bool(np.array_equal(d[0], h[0])), "values": bool(np.array_equal(canon(d[1]), canon(h[1]))), "ranks": bool(np.array_equal(d[2], h[2])),
                        "top_ids": bool(np.array_equal(dt[0], ht[0])), "top_values": bool(np.array_equal(canon(dt[1]), canon(ht[1]))),
                        "store_files": files_of(a) == files_of(b), "nan_values": int(np.isnan(d[1]).sum()), "infinite_values": int(np.isinf(d[1]).sum())}
                stored_bytes = sum(os.path.getsize(os.path.join(a, db, f)) for db in os.listdir(a) for f in os.listdir(os.path.join(a, db)))
            else:
                for key, dt_ in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t7 - t5, t7 - t6)):
                    t[key].append(dt_)
            shutil.rmtree(a)
            shutil.rmtree(b)
            print(name, "repetition", r, [round(x, 4) for x in (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t7 - t5)], file=sys.stderr, flush=True)
        cell = {"keys": n, "divisor": divisor, "outputs_equal_in_the_warm_up": same, "store_bytes": stored_bytes}
        for what in ("finish", "top", "store"):
            dev, host = spread(t[what + "_dev"]), spread(t[what + "_host"])
            gap = max(dev["max_s"] - dev["min_s"], host["max_s"] - host["min_s"])
            cell[what] = {"device_route": dev, "host_route": host, "median_gain_s": round(host["median_s"] - dev["median_s"], 6), "larger_spread_s": round(gap, 6),
                          "beats_by_more_than_the_spread": bool(host["median_s"] - dev["median_s"] > gap), "ratio_of_medians": round(host["median_s"] / dev["median_s"], 2)}
        cell["store"]["host_route_hb_store_harmonic_alone"] = spread(t["store_host_writer"])
        cell["link_bytes_per_key"] = {"finish": {"device_route": 32, "host_route": 32}, "top": {"device_route": round(24 * min(top_k, n) / max(n, 1), 2), "host_route": 32},
                                      "store": {"device_route": 40, "host_route": 32}}
        res["tables"][name] = cell
        print(name, cell, file=sys.stderr, flush=True)

    try:
        t0 = time.perf_counter()
        nodes, from_ids, to_ids = rmat_worker(scale, total_edges)
        print("graph: %d nodes, %d edges, %.1f s" % (len(nodes), len(from_ids), time.perf_counter() - t0), file=sys.stderr, flush=True)
        picked = np.unique(from_ids[rng.integers(0, len(from_ids), 4 * n_sources + 4)])
        rng.shuffle(picked)
        sources = [(int(k["hi"]) << 64) | int(k["lo"]) for k in picked[:n_sources]]
        with ampc.ValueTable(ampc.KIND_KAHAN) as cent:
            with ampc.WorkerGraph(nodes, from_ids, to_ids) as graph:
                lanes = ampc.run_shortest_paths_job([graph], sources, 5)
                ampc.fold_harmonic_lanes(lanes, cent, 1.0 / 2657.0, len(sources))
                lanes.close()
            del nodes, from_ids, to_ids
            measure("lanes_job_centralities", cent, 1.0)
        with ampc.ValueTable(ampc.KIND_KAHAN, capacity_hint=K) as tab:
            for b in range(0, K, 1_000_000):
                v = np.zeros(len(keys[b:b + 1_000_000]), dtype=ampc.KAHAN)
                v["sum"] = np.floor(rng.random(len(v)) * 1e6)  # a million levels: ties of about K / 1e6 keys each
                v["err"] = rng.random(len(v)) * 1e-9
                tab.batch_set(keys[b:b + 1_000_000], v)
            measure("synthetic_kahan", tab, float(K - 1))
    finally:
        shutil.rmtree(scratch, ignore_errors=True)
    res["all_outputs_equal"] = all(v for c in res["tables"].values() for k, v in c["outputs_equal_in_the_warm_up"].items() if isinstance(v, bool))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("keys", nargs="?", type=int, default=10_000_000)
    ap.add_argument("batch", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--values", action="store_true", help="also the scalar value tables (every kind / operator unless --kind / --op)")
    ap.add_argument("--kind", choices=sorted(KINDS))
    ap.add_argument("--op", choices=sorted(OP_NAMES))
    ap.add_argument("--centralities", action="store_true", help="also hbu_update_centralities against the host route")
    ap.add_argument("--edges", action="store_true", help="also hbu_update_counters / hbu_update_distances against the host route")
    ap.add_argument("--rounds", action="store_true", help="also the resident worker's round calls against the host-fed route")
    ap.add_argument("--round-edges", type=int, default=100_000_000, help="R-MAT edges of the worker graph of --rounds")
    ap.add_argument("--round-scale", type=int, default=0, help="R-MAT scale of that graph (0: the largest with 2^scale <= keys)")
    ap.add_argument("--only-rounds", action="store_true", help="skip the counter-table section (with --rounds)")
    ap.add_argument("--approx", action="store_true", help="also the approximated-harmonic job: the fold against the composed route, export, whole sources")
    ap.add_argument("--only-approx", action="store_true", help="skip the counter-table section (with --approx)")
    ap.add_argument("--lanes", action="store_true", help="also 64 sources through the per-source route and through one 64-lane walk, and the round call alone")
    ap.add_argument("--only-lanes", action="store_true", help="skip the counter-table section (with --lanes)")
    ap.add_argument("--finish", action="store_true", help="also the finish of a job (values, ranks, top nodes, store) against items() + numpy + hb_store_harmonic")
    ap.add_argument("--only-finish", action="store_true", help="skip the counter-table section (with --finish)")
    ap.add_argument("--sources", type=int, default=5, help="timed sources of --approx (one more warms up)")
    ap.add_argument("--reps", type=int, default=5, help="timed batches per shape and side of --edges / repetitions of --rounds (at least 5)")
    ap.add_argument("--out")
    args = ap.parse_args()
    K, B = args.keys, args.batch
    rng = np.random.default_rng(1)
    keys = np.zeros(K, dtype=_lib.U128)
    keys["lo"] = rng.permutation(K).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    keys["hi"] = rng.integers(0, 1 << 63, K, dtype=np.uint64)
    out = {"keys": K, "pairs_per_batch": B, "bytes_per_pair": 80}
    for label, pinned in (() if (args.only_rounds and args.rounds) or (args.only_approx and args.approx) or (args.only_lanes and args.lanes) or (args.only_finish and args.finish) else (("pageable", False), ("pinned", True))):
        kb = _lib.PinnedRecords(B, dtype=_lib.U128) if pinned else None
        vb = _lib.PinnedRecords(B * 64, dtype=np.uint8) if pinned else None
        kbuf = kb.array if pinned else np.zeros(B, dtype=_lib.U128)
        vbuf = (vb.array if pinned else np.zeros(B * 64, dtype=np.uint8)).reshape(B, 64)
        vbuf[:] = rng.integers(0, 40, (B, 64), dtype=np.uint8)
        res = {}
        with ampc.CounterTable(capacity_hint=K) as tab:
            lib, h = tab.lib, tab.h
            acts = np.zeros(B, dtype=np.uint8)
            found = np.zeros(B, dtype=np.uint8)
            getbuf = _lib.PinnedRecords(B * 64, dtype=np.uint8) if pinned else None
            gout = getbuf.array if pinned else np.zeros(B * 64, dtype=np.uint8)
            t_set = t_up = t_get = 0.0
            for b in range(0, K, B):                      # setup_counters: every pair inserts a new key
                n = min(B, K - b)
                kbuf[:n] = keys[b:b + n]
                t0 = time.perf_counter()
                tab._check(lib.hbu_batch_set(h, _lib._ptr(kbuf), _lib._ptr(vbuf), n))
                t_set += time.perf_counter() - t0
            assert len(tab) == K
            rounds = max(K // B, 1)
            for r in range(rounds):                       # update_counters: random destinations, ~1/8 of the batch on 1000 hub keys
                idx = rng.integers(0, K, B)
                hub = rng.random(B) < 0.125
                idx[hub] = rng.integers(0, 1000, int(hub.sum()))
                kbuf[:] = keys[idx]
                t0 = time.perf_counter()
                tab._check(lib.hbu_batch_upsert(h, _lib._ptr(kbuf), _lib._ptr(vbuf), B, _lib._ptr(acts)))
                t_up += time.perf_counter() - t0
            for r in range(rounds):                       # get_old_counters
                kbuf[:] = keys[rng.integers(0, K, B)]
                t0 = time.perf_counter()
                tab._check(lib.hbu_batch_get(h, _lib._ptr(kbuf), B, _lib._ptr(gout), _lib._ptr(found)))
                t_get += time.perf_counter() - t0
            assert found.all() and len(tab) == K
            res = {"batch_set_inserting_Mpairs_per_s": round(K / t_set / 1e6, 2), "batch_upsert_Mpairs_per_s": round(rounds * B / t_up / 1e6, 2),
                   "batch_get_Mkeys_per_s": round(rounds * B / t_get / 1e6, 2),
                   "upsert_link_GBs": round(rounds * B * 81 / t_up / 1e9, 2), "actions_merged_share_last_batch": round(float((acts == ampc.MERGED).mean()), 3)}
            if getbuf:
                getbuf.close()
        for x in (kb, vb):
            if x:
                x.close()
        out[label] = res
        print(label, res, file=sys.stderr, flush=True)
    if args.values or args.kind or args.op:
        out["values_pinned"] = {}
        for name, op in OP_NAMES.items():
            kind = name.split("_")[0]
            if (args.kind and kind != args.kind) or (args.op and name != args.op):
                continue
            out["values_pinned"][name] = values_mode(rng, keys, K, B, KINDS[kind], op)
            print(name, out["values_pinned"][name], file=sys.stderr, flush=True)
    if args.centralities:
        out["update_centralities"] = centralities_mode(rng, keys, K, B)
    if args.edges:
        out["edges"] = edges_mode(rng, keys, K, B, max(args.reps, 5))
        print("edges", out["edges"], file=sys.stderr, flush=True)
    if args.rounds:
        scale = args.round_scale or max(int(K).bit_length() - 1, 1)
        out["rounds"] = rounds_mode(rng, K, B, max(args.reps, 5), args.round_edges, scale)
    if args.approx:
        scale = args.round_scale or max(int(K).bit_length() - 1, 1)
        out["approx"] = approx_mode(rng, keys, K, max(args.reps, 5), args.round_edges, scale, max(args.sources, 1))
    if args.lanes:
        scale = args.round_scale or max(int(K).bit_length() - 1, 1)
        out["lanes"] = lanes_mode(rng, max(args.reps, 5), args.round_edges, scale)
    if args.finish:
        scale = args.round_scale or max(int(K).bit_length() - 1, 1)
        out["finish"] = finish_mode(rng, keys, K, max(args.reps, 5), args.round_edges, scale)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.finish and not out["finish"]["all_outputs_equal"]:
        sys.exit("--finish: the two routes differ (see outputs_equal_in_the_warm_up)")


if __name__ == "__main__":
    main()
