"""HB_FLAG_PACKED_WIRE: every exchange that moves whole counters moves them as 48-byte rows, 6 bits per
register.  The three kernels against a numpy restatement of the bit stream; the three packed exchanges between logical ranks on one
device (hb_debug_exchange) against the oracle after every pass, with the bytes a rank receives booked exactly; the flag off is the
parent; the refusals; the one-rank communicator; N processes through hb_set_collectives + hb_set_all_to_all.  All tests need a
gfx950 device (tests/test_packed_wire_simt.py runs them on the SIMT interpreter)."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib, dist, synth
from tests import graphs

pytestmark = pytest.mark.gpu
PACKED = _lib.HB_FLAG_PACKED_WIRE
LEGAL = np.array([0] + list(range(1, 59)) + [65], dtype=np.uint8)  # what a register of this library can hold


# ---- the bit stream, restated ---------------------------------------------------------------------------------------------------
def pack6(rows):
    """(count, 64) registers -> (count, 48) bytes: a plain little-endian bit stream of 64 six-bit codes, code = r (r <= 58) or 63 (65)."""
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 64)
    codes = np.where(rows == 65, 63, rows).astype(np.uint8)
    bits = np.unpackbits(codes[:, :, None], axis=2, bitorder="little")[:, :, :6]
    return np.packbits(bits.reshape(len(rows), 384), axis=1, bitorder="little")


def unpack6(packed):
    bits = np.unpackbits(np.asarray(packed, dtype=np.uint8).reshape(-1, 48), axis=1, bitorder="little").reshape(-1, 64, 6)
    codes = np.packbits(np.concatenate([bits, np.zeros(bits.shape[:2] + (2,), np.uint8)], axis=2), axis=2, bitorder="little")[:, :, 0]
    return np.where(codes == 63, 65, codes).astype(np.uint8)


def _legal_rows(rng, count):
    """random_registers, with the values a counter cannot hold (59..64) replaced by legal ones"""
    rows = graphs.random_registers(rng, count)
    bad = (rows > 58) & (rows != 65)
    rows[bad] = LEGAL[rng.integers(0, len(LEGAL), int(bad.sum()))]
    return rows


_MASTER = {}


def _master_rows():
    """one row per (legal value, position): that value at that position, the other 63 positions random - 3840 rows, built once"""
    if "rows" not in _MASTER:
        rng = np.random.default_rng(40)
        rows = _legal_rows(rng, len(LEGAL) * 64)
        for k, v in enumerate(LEGAL):
            for pos in range(64):
                rows[k * 64 + pos, pos] = v
        rows.setflags(write=False)
        _MASTER["rows"] = rows
    return _MASTER["rows"]


def test_restatement_is_a_plain_bit_stream():
    row = np.zeros((1, 64), np.uint8)
    row[0, 0], row[0, 1], row[0, 63] = 1, 65, 58
    p = pack6(row)[0]
    assert p[0] == (1 | (63 << 6)) & 0xFF and p[1] == 63 >> 2 and p[47] == 58 << 2
    assert np.array_equal(unpack6(pack6(_master_rows())), _master_rows())


# ---- test 1: the code -----------------------------------------------------------------------------------------------------------
def test_every_value_in_every_position(gpu_ctx_factory):
    """pieces = 1 over all 3840 rows: the packed rows are the restatement's, and unpacking gives the rows back; pieces = 4 over the same
    rows cut in four: the packed maximum is the restatement's pack of the byte-wise maximum."""
    rows = _master_rows()
    with gpu_ctx_factory() as ctx:
        packed, out, ms = ctx.wire6(rows, 1)
        assert np.array_equal(out, rows)
        assert np.array_equal(packed, pack6(rows))
        packed, out, ms = ctx.wire6(rows, 4)
        want = rows.reshape(4, -1, 64).max(axis=0)
        assert np.array_equal(out, want) and np.array_equal(packed, pack6(want))
        assert len(ms) == 3 and all(m >= 0 for m in ms)


@pytest.mark.parametrize("pieces", [1, 2, 3, 4])
def test_wave_and_quad_tails(gpu_ctx_factory, pieces):
    """count = 1, 15, 16, 17, 64, 65: a quad, a wave less one row, a whole wave, one row more, a workgroup, one row more"""
    rows = _master_rows()
    at = 0
    with gpu_ctx_factory() as ctx:
        for count in (1, 15, 16, 17, 64, 65):
            take = rows[np.arange(at, at + pieces * count) % len(rows)]
            at += 977 * pieces  # (another window of the master rows for every case)
            packed, out, _ = ctx.wire6(take, pieces)
            want = take.reshape(pieces, count, 64).max(axis=0)
            assert packed.shape == (count, 48) and out.shape == (count, 64)
            assert np.array_equal(out, want), (pieces, count)
            assert np.array_equal(packed, pack6(want)), (pieces, count)
            if pieces == 1:
                assert np.array_equal(out, take)


def test_register_ten_of_a_quarter_straddles_the_word(gpu_ctx_factory):
    """bits 60..65 of a quarter's 96: the low four bits of code 10 end the second 32-bit word, its high two begin the third"""
    rows = np.zeros((4, 64), np.uint8)
    for q in range(4):
        rows[q, 16 * q + 10] = 45  # 0b101101
    rows[3, 16 * 3 + 10] = 65      # code 63: all six bits
    with gpu_ctx_factory() as ctx:
        packed, out, _ = ctx.wire6(rows, 1)
        assert np.array_equal(out, rows)
        for q in range(4):
            want = np.zeros(48, np.uint8)
            code = 63 if q == 3 else 45
            want[12 * q + 7] = (code & 15) << 4
            want[12 * q + 8] = code >> 4
            assert np.array_equal(packed[q], want), q
        # and the maximum across the straddle: 45 against 58 in another piece, 65 against 58
        other = np.zeros((4, 64), np.uint8)
        other[:, 10] = 58
        other[3, 16 * 3 + 10] = 58
        packed, out, _ = ctx.wire6(np.concatenate([rows, other]), 2)
        assert np.array_equal(out, np.maximum(rows, other)) and np.array_equal(packed, pack6(np.maximum(rows, other)))
        assert out[0, 10] == 58 and out[3, 58] == 65


# ---- test 2: logical ranks on one device ----------------------------------------------------------------------------------------
def _graph(name):
    """(ids, row_ptr, src, registers after every pass by the oracle, T, vals, keep) - computed once per graph and never changed"""
    if name not in _MASTER:
        if name == "extreme":
            ids, row_ptr, src = graphs.extreme_register_graph()
        else:
            n, m = {"lcg300": (300, 2400), "lcg40": (40, 200)}[name]
            ids, row_ptr, src = graphs.dense_from_tuples(graphs.lcg_graph(n=n, m=m, seed=7))
        o = hbo.Dense(np.ascontiguousarray(ids["lo"]), row_ptr, src)
        per_pass, has = [], True
        while has:
            has, _ = o.step()
            per_pass.append(o.registers())
        vals, keep, k = o.finish()
        _MASTER[name] = (ids, row_ptr, src, per_pass, len(per_pass), vals, keep)
    return _MASTER[name]


def _flags(mode, packed):
    flags = _lib.HB_FLAG_NO_RCCL | (_lib.HB_FLAG_DEST_PARTITION if mode.startswith("dest") else 0)
    flags |= _lib.HB_FLAG_CHANGED_ONLY if mode.endswith("_changed") else 0
    return flags | (PACKED if packed else 0)


def _run_logical(factory, name, world, mode, packed):
    """the loop of test_logical_ranks_on_one_device: after every pass every rank holds the oracle's registers; the final list is the
    oracle's bit for bit.  Returns (wire_bytes per rank, pass statistics of rank 0, n_pad)."""
    ids, row_ptr, src, per_pass, T, vals, keep = _graph(name)
    split = dist.partition_dense_by_dest if mode.startswith("dest") else dist.partition_dense
    ctxs = []
    try:
        for r in range(world):
            c = factory(rank=r, world_size=world, flags=_flags(mode, packed), chunk=16, tune=(0, 0, 0, 7, 4))
            rp, sr = split(row_ptr, src, r, world)
            c.load_dense(ids, rp, sr)
            c.begin()
            ctxs.append(c)
        has, t = True, 0
        while has:
            for c in ctxs:
                c.step_local()
            _lib.Context.exchange(ctxs, 0)
            out = [c.step_finish() for c in ctxs]
            assert len(set(out)) == 1
            has = out[0]
            assert t < T
            for r, c in enumerate(ctxs):
                assert np.array_equal(c.registers(), per_pass[t]), (name, world, mode, "pass", t, "rank", r)
            t += 1
        assert t == T
        _lib.Context.exchange(ctxs, 1)
        for c in ctxs:
            c.finish()
            gids, gvals = c.results()
            assert c.stats()["passes"] == T
            assert np.array_equal(gids, ids[keep])
            assert np.array_equal(gvals.view(np.uint64), vals[keep].view(np.uint64))
        ps = [(int(p["changed"]), int(p["mode"]), int(p["active_edges"])) for p in ctxs[0].pass_stats()]
        return [int(c.stats()["wire_bytes"]) for c in ctxs], ps, int(ctxs[0].plan()["n_pad"])
    finally:
        for c in ctxs:
            c.close()


def _edge_slice(n_pad, world):
    return ((n_pad + world - 1) // world + 63) // 64 * 64


@pytest.mark.parametrize("world,mode", [(2, "dest"), (3, "dest"), (4, "dest"), (2, "edge"), (3, "edge"), (4, "edge"), (2, "edge_changed"),
                                        (4, "edge_changed"), (2, "dest_changed")])
def test_packed_exchanges_between_logical_ranks(gpu_ctx_factory, world, mode):
    """(a) registers up to 58 and 65; (b) 300 nodes: n_pad = 320, edge slices 128/128/64 for three ranks and an empty last slice for
    four; 40 nodes: n_pad = 64, rank 1 of 2 owns nothing on the edge partition."""
    assert int(max(r.max() for r in _graph("extreme")[3])) == 65 and int(_graph("extreme")[3][-1].max()) == 65
    for name in ("extreme", "lcg300", "lcg40"):
        T = _graph(name)[4]
        wires, _, n_pad = _run_logical(gpu_ctx_factory, name, world, mode, True)
        if name == "lcg300" and mode == "edge":
            assert n_pad == 320 and _edge_slice(n_pad, world) == {2: 192, 3: 128, 4: 128}[world]
        if name == "lcg40" and mode == "edge":
            assert n_pad == 64 and _edge_slice(n_pad, world) == 64
        if mode == "dest":
            S = n_pad // world
            assert wires == [T * ((n_pad - min(S, n_pad)) * 48 + (n_pad - min(S, n_pad)) // 8)] * world, (name, wires)
        elif mode == "edge":
            assert wires == [T * 2 * (world - 1) * _edge_slice(n_pad, world) * 48] * world, (name, wires)
        else:
            off, _, _ = _run_logical(gpu_ctx_factory, name, world, mode, False)
            if mode == "dest_changed":  # 6-bit already: the flag changes nothing
                assert wires == off, (name, wires, off)
                continue
            for w48, w64 in zip(wires, off):
                # the bitmap part is the same in both runs: (w64 - B) * 3 == (w48 - B) * 4  =>  B = 4 w48 - 3 w64
                b = 4 * w48 - 3 * w64
                assert b == T * (world - 1) * (n_pad // 32) * 4, (name, w48, w64, b)
                # a row of the union costs a rank 2 (world - 1) / world of its bytes: 64 and 48 for two ranks, 96 and 72 for four
                per64, per48 = 2 * (world - 1) * 64 // world, 2 * (world - 1) * 48 // world
                assert w48 < w64 and (w64 - b) % per64 == 0 and (w48 - b) % per48 == 0 and (w64 - b) // per64 == (w48 - b) // per48, (name, w48, w64, b)


# ---- test 3: the flag off is the parent -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,mode", [(2, "edge"), (2, "edge_changed"), (3, "dest")])
def test_flag_off_is_unchanged(gpu_ctx_factory, world, mode):
    """same registers after every pass (both runs are compared with the oracle's), same pass statistics; and without the flag the bytes
    booked are what tests/test_gpu.py::test_logical_ranks_on_one_device asserts: none for the plain edge partition (hb_debug_exchange books
    none for whole 64-byte rows, nor for the destination partition's whole slices), below 0.8 of the full all-reduce for its
    changed-only form."""
    name = "lcg300"
    T = _graph(name)[4]
    off, ps_off, n_pad = _run_logical(gpu_ctx_factory, name, world, mode, False)
    on, ps_on, _ = _run_logical(gpu_ctx_factory, name, world, mode, True)
    assert ps_off == ps_on and len(ps_off) == T
    full = T * 2 * (world - 1) * n_pad * 64 // world
    if mode == "edge_changed":
        assert all(0 < w < 0.8 * full for w in off), (off, full)
    else:
        assert off == [0] * world, off
    assert all(w > 0 for w in on)


# ---- test 4: refusals -------------------------------------------------------------------------------------------------------------
def test_refused_with_the_reference_tail(gpu_ctx_factory):
    with pytest.raises(_lib.HyperballError) as e:
        gpu_ctx_factory(flags=PACKED | _lib.HB_FLAG_REFERENCE_TAIL)
    assert e.value.code == _lib.HB_ERR_INVALID and "HB_FLAG_PACKED_WIRE" in str(e.value) and "HB_FLAG_REFERENCE_TAIL" in str(e.value)


def test_edge_partition_with_caller_collectives_needs_all_to_all(gpu_ctx_factory):
    """collectives that do nothing (the load's all-reduce of the out-degrees then sees one rank's share): hb_begin must refuse before any
    pass runs; with an all_to_all registered it accepts"""
    ids, row_ptr, src = _graph("lcg40")[:3]
    H = dist.HostStagedCollectives
    cbs = (H._ALL_REDUCE(lambda *a: 0), H._ALL_GATHER(lambda *a: 0), H._BROADCAST(lambda *a: 0))
    a2a = _lib.ALL_TO_ALL_FN(lambda *a: 0)

    class Ops(ctypes.Structure):
        _fields_ = [("user", ctypes.c_void_p), ("all_reduce", H._ALL_REDUCE), ("all_gather", H._ALL_GATHER), ("broadcast", H._BROADCAST)]

    ops = Ops(None, *cbs)
    for with_a2a in (False, True):
        with gpu_ctx_factory(rank=0, world_size=2, flags=_lib.HB_FLAG_NO_RCCL | PACKED) as ctx:
            if with_a2a:  # before hb_set_collectives there is no `user` pointer to pass on
                with pytest.raises(_lib.HyperballError):
                    ctx.set_all_to_all(a2a)
            ctx._check(ctx.lib.hb_set_collectives(ctx.h, ctypes.byref(ops)))
            if with_a2a:
                ctx.set_all_to_all(a2a)
            rp, sr = dist.partition_dense(row_ptr, src, 0, 2)
            ctx.load_dense(ids, rp, sr)
            if with_a2a:
                ctx.begin()
                continue
            with pytest.raises(_lib.HyperballError) as e:
                ctx.begin()
            assert e.value.code == _lib.HB_ERR_INVALID and "hb_set_all_to_all" in str(e.value) and "HB_FLAG_PACKED_WIRE" in str(e.value)


def test_inert_on_a_plain_one_rank_context(gpu_ctx_factory):
    ids, row_ptr, src, per_pass, T, vals, keep = _graph("lcg300")
    got = {}
    for flags in (0, PACKED):
        with gpu_ctx_factory(flags=flags) as ctx:
            ctx.load_dense(ids, row_ptr, src)
            st = ctx.run()
            got[flags] = (ctx.results(), ctx.registers(), [(int(p["changed"]), int(p["mode"]), int(p["active_edges"])) for p in ctx.pass_stats()])
            assert st["passes"] == T and st["wire_bytes"] == 0
    (ia, va), ra, pa = got[0]
    (ib, vb), rb, pb = got[PACKED]
    assert np.array_equal(ia, ib) and np.array_equal(va.view(np.uint64), vb.view(np.uint64)) and np.array_equal(ra, rb) and pa == pb
    assert np.array_equal(ra, per_pass[-1]) and np.array_equal(va.view(np.uint64), vals[keep].view(np.uint64))


# ---- test 5: the communicator branch, one rank --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dest", [False, True])
def test_one_rank_communicator(gpu_ctx_factory, dest):
    """HB_FLAG_RCCL_SELF: the library's own collectives on a one-rank communicator - all-to-all as a device copy, the in-place all-gather
    of the packed slices; the only run of the communicator branch one GPU allows"""
    ids, row_ptr, src, per_pass, T, vals, keep = _graph("extreme")
    flags = _lib.HB_FLAG_RCCL_SELF | PACKED | (_lib.HB_FLAG_DEST_PARTITION if dest else 0)
    with gpu_ctx_factory(flags=flags, rccl_id=_lib.rccl_unique_id()) as ctx:
        ctx.load_dense(ids, row_ptr, src)
        ctx.begin()
        for t in range(T):
            has = ctx.step()
            assert np.array_equal(ctx.registers(), per_pass[t]), t
            assert has == (t + 1 < T)
        ctx.finish()
        gids, gvals = ctx.results()
        assert np.array_equal(gids, ids[keep]) and np.array_equal(gvals.view(np.uint64), vals[keep].view(np.uint64))
        assert ctx.stats()["wire_bytes"] == 0  # (one rank receives nothing)


# ---- test 6: processes on one device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world,modes", [(2, "dest,edge,edge_changed"), (3, "edge")])
def test_multi_process_packed_exchanges_on_one_device(tmp_path, world, modes):
    """N processes (torch.distributed.run, gloo) drive the library's pass driver with the flag on ONE device; the exchanges go through
    hb_set_collectives + hb_set_all_to_all (stract_amd.dist.HostStagedCollectives).  Every rank's final list is the oracle's, the
    counters are the same on all ranks, and the all-to-all carried the edge partition's counters in every pass."""
    scale, m = 10, 8_000
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "dist_packed_worker.py"), str(scale), str(m), str(tmp_path), modes]
    r = subprocess.run(cmd, cwd=root, env=dict(os.environ, OMP_NUM_THREADS="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    g = synth.RmatGraph(scale, m)
    o = hbo.Dense(g.id_low64(), g.row_ptr, g.src)
    T = o.run()
    ovals, keep, k = o.finish()
    want_bits = ovals[keep].view(np.uint64).tolist()
    n_pad = (g.n + 63) // 64 * 64
    ranks = [json.load(open(os.path.join(str(tmp_path), "rank%d.json" % i))) for i in range(world)]
    for mode in modes.split(","):
        for i, z in enumerate(ranks):
            z = z[mode]
            assert z["callback_error"] is None, (mode, i, z["callback_error"])
            assert z["passes"] == T and z["results"] == k, (mode, i, z["passes"], T)
            assert z["vals_bits"] == want_bits, (mode, i)
            assert z["same_counters_on_all_ranks"], (mode, i)
            if mode.startswith("edge"):
                # one per pass; the changed-only form has none in a pass whose union of changed rows is empty (R == 0 means no call) -
                # which the last pass of a run, the one that changes nothing, always is
                assert z["calls"]["all_to_all"] >= (T if mode == "edge" else T - 1), (mode, z["calls"])
            else:
                assert z["calls"]["all_to_all"] == 0, (mode, z["calls"])
            if mode == "edge":
                assert z["calls"]["all_to_all"] == T and z["wire_bytes"] == T * 2 * (world - 1) * _edge_slice(n_pad, world) * 48, (mode, z)
