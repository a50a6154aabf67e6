#!/usr/bin/env python3
"""tools/packed_wire_bench.py - the three kernels of HB_FLAG_PACKED_WIRE at a BASELINE size, on one GPU.

    python tools/packed_wire_bench.py --config C3 --out profiles/packed_wire_bench.json

The graph is loaded, three passes run, nothing is downloaded.  hb_debug_wire6 without rows then packs the context's own resident
counters (all n_pad rows; every piece is that buffer), takes the maximum over the pieces in packed form and unpacks it, each launch
between two events on the context's stream: pieces = 2 and 8, one warm-up call and the median of `--runs` calls.  Per kernel: ms, the
bytes it moves (computed from the shapes: pack reads 64 and writes 48 bytes per row and piece, the maximum reads 48 bytes per row and
piece and writes 48 per row, unpack reads 48 and writes 64 per row) and TB/s.  The yardstick is measured in the same process: a plain
device-to-device copy of n_pad x 64 bytes (reads and writes counted, like the kernels'), same warm-up and median - the kernels are to be
judged against that copy.  Last, the bytes a rank receives (hb_stats.wire_bytes) in a logical two-rank run on a small graph, edge
partition and its changed-only form, with and without the flag.  Wire TIME is not measured anywhere here: one card has no wire."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stract_amd import _lib, dist, synth  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def copy_yardstick(nbytes, runs):
    """ms of a device-to-device hipMemcpyAsync of nbytes between two events, through the HIP runtime the library itself runs on"""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what, rc))

    a, b, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    ok(hip.hipMalloc(ctypes.byref(a), ctypes.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipMalloc(ctypes.byref(b), ctypes.c_size_t(nbytes)), "hipMalloc")
    ok(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
    try:
        ok(hip.hipMemset(a, 0, ctypes.c_size_t(nbytes)), "hipMemset")
        ms = []
        for k in range(runs + 1):  # (the first copy is the warm-up)
            ok(hip.hipEventRecord(e0, None), "hipEventRecord")
            ok(hip.hipMemcpyAsync(b, a, ctypes.c_size_t(nbytes), 3, None), "hipMemcpyAsync")  # 3 = hipMemcpyDeviceToDevice
            ok(hip.hipEventRecord(e1, None), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            t = ctypes.c_float(0)
            ok(hip.hipEventElapsedTime(ctypes.byref(t), e0, e1), "hipEventElapsedTime")
            if k:
                ms.append(t.value)
    finally:
        hip.hipFree(a)
        hip.hipFree(b)
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
    return _median(ms)


def kernel_rates(ctx, n_pad, pieces, runs):
    ctx.wire6(None, pieces, count=n_pad)  # warm-up: code objects, the scratch buffers' first touch
    laps = [ctx.wire6(None, pieces, count=n_pad)[2] for _ in range(runs)]
    moved = dict(pack=pieces * n_pad * (64 + 48), max=n_pad * 48 * (pieces + 1), unpack=n_pad * (48 + 64))
    out = {}
    for k, name in enumerate(("pack", "max", "unpack")):
        ms = _median([lap[k] for lap in laps])
        out[name] = dict(ms=ms, bytes=moved[name], TBps=moved[name] / (ms * 1e-3) / 1e12 if ms > 0 else None, ms_all=[lap[k] for lap in laps])
    return out


def logical_wire_bytes(scale, m, world=2):
    """hb_stats.wire_bytes of rank 0 of `world` logical ranks on one device (hb_debug_exchange), per mode, flag off / on"""
    g = synth.RmatGraph(scale, m)
    out = dict(graph="R-MAT scale %d, %d edges" % (scale, g.m), n=int(g.n), world=world)
    for mode in ("edge", "edge_changed"):
        for packed in (False, True):
            flags = _lib.HB_FLAG_NO_RCCL | (_lib.HB_FLAG_CHANGED_ONLY if mode == "edge_changed" else 0) | (_lib.HB_FLAG_PACKED_WIRE if packed else 0)
            ctxs = []
            try:
                for r in range(world):
                    c = _lib.Context(rank=r, world_size=world, flags=flags)
                    rp, src = dist.partition_dense(g.row_ptr, g.src, r, world)
                    c.load_dense(g.ids, rp, src)
                    c.begin()
                    ctxs.append(c)
                has, T = True, 0
                while has:
                    for c in ctxs:
                        c.step_local()
                    _lib.Context.exchange(ctxs, 0)
                    has = [c.step_finish() for c in ctxs][0]
                    T += 1
                _lib.Context.exchange(ctxs, 1)
                for c in ctxs:
                    c.finish()  # (the statistics of a run are complete once it is finished)
                wb = int(ctxs[0].stats()["wire_bytes"])
            finally:
                for c in ctxs:
                    c.close()
            out["%s_%s" % (mode, "packed" if packed else "64B")] = wb
            out["passes"] = T
    n_pad = (g.n + 63) // 64 * 64
    # the logical ranks' exchange books nothing for whole 64-byte rows (it moves none over a wire); a linked context books this:
    out["edge_64B_by_formula"] = out["passes"] * 2 * (world - 1) * n_pad * 64 // world
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pieces", default="2,8")
    ap.add_argument("--wire-graph", default="16:1000000", help="scale:edges of the logical two-rank runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_wire_bench.json"))
    args = ap.parse_args()
    g, scale, label = synth.make_config(args.config)
    out = dict(config=args.config, label=label, n=int(g.n), m=int(g.m), runs=args.runs)
    with _lib.Context() as ctx:
        out["device"] = ctx.device_name()
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        ctx.begin()
        for _ in range(3):
            ctx.step()
        n_pad = (g.n + 63) // 64 * 64  # (the node rows of a one-rank plan: n rounded up to a 64-row tile)
        out["n_pad"] = n_pad
        copy_ms = copy_yardstick(n_pad * 64, args.runs)
        out["d2d_copy"] = dict(ms=copy_ms, bytes=2 * n_pad * 64, TBps=2 * n_pad * 64 / (copy_ms * 1e-3) / 1e12)
        out["kernels"] = {}
        for pieces in [int(x) for x in args.pieces.split(",")]:
            rec = kernel_rates(ctx, n_pad, pieces, args.runs)
            for name in rec:
                rec[name]["rate_over_copy"] = rec[name]["TBps"] / out["d2d_copy"]["TBps"] if rec[name]["TBps"] else None
            out["kernels"]["pieces_%d" % pieces] = rec
    del g
    ws, wm = (int(x) for x in args.wire_graph.split(":"))
    out["wire_bytes_logical_ranks"] = logical_wire_bytes(ws, wm)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
