"""The fused passes on counters with registers of 48..58 and 65 (tests/graphs.py extreme_register_graph; NodeIDs built by inverting
FastHasher's multiplication, because small, salted and R-MAT ids never raise a register above about 25).  What that reaches and no
other graph test does: the `big` branch of every copy of the epilogue (hb_estimator.hip.h hll_sum_quad / hll_fold_quad; the deferred
epilogue of hb_kernels.hip.h with its p_szfull / flag 8 hand-over to the lane that owns the row; the per-tile epilogue, hb_sweep.hip.h
and hb_tail.hip.h through hll_size_quad), f64_as_usize at 2^64 - 1 with Kahan terms of about 2^64 behind it, the value 65 and values
48..58 in the 2-byte src_jp / self_jp entries of pass 0, and codes 48..58 of the six-bit wire.

The reference of every comparison is the CPU oracle (oracle/hb_oracle.c), whose estimator is pinned at these register values against
exact rational arithmetic in tests/test_oracle.py; its per-pass state is computed once (graphs.extreme_reference) and shared.
Nothing here tries to show that the f64 fold depends on its order: no size of this graph could show it (see extreme_register_graph)."""
import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib, dist
from tests import graphs
from tests.test_gpu import VARIANTS, _check_final

pytestmark = pytest.mark.gpu

# each reaches another copy of the epilogue or of the jp path; few_blocks: one workgroup per compute unit, so that a launch with fewer
# workgroups than 64-row tiles (the interpreter's two compute units) defers four tiles per flush of the epilogue
assert VARIANTS["default_lean"] is VARIANTS["default"]  # (test_gpu.py lists the non-lean "default" only as a base of its _lean loop)
RUN = ("default", "default_lean", "old_per_tile_epilogue", "chunk4_multilevel", "frontier_always", "sparse_always_multilevel", "sparse_always_chunk128",
       "pass0_level1_generic_kernel", "pass0_level1_chunk128", "full_init_switch", "long_tail_tail_kernel_after_any_pass", "sweep_rows_round_by_round",
       "few_blocks")
FORCED_MODES = {"frontier_always": {0, 1}, "sparse_always_multilevel": {0, 2}, "sparse_always_chunk128": {0, 2}, "sweep_rows_round_by_round": {0, 2},
                "long_tail_tail_kernel_after_any_pass": {0, 4}}
SATURATED = (1 << 64) - 1


@pytest.mark.parametrize("variant", RUN)
def test_per_pass_state_on_extreme_registers(gpu_ctx_factory, variant):
    """The loop of test_per_pass_state_matches_oracle: registers, both Kahan words, sizes, state checksum and changed count after every
    pass, the final list and the ranks - on a graph where from pass 0 on more than a hundred counters have a register above 47 and no
    zero register, some sizes are 2^64 - 1 and some Kahan sums are at least 2^63."""
    ref = graphs.extreme_reference()  # (asserts the graph's conditions on the oracle alone)
    kw = VARIANTS[variant]
    with gpu_ctx_factory(**kw) as ctx:
        ctx.load_dense(ref.ids, ref.row_ptr, ref.src)
        if variant == "default":
            assert ctx.plan()["nv"] > 0  # virtual rows at the default chunk size: the hubs' partial maxima carry big registers
        ctx.begin()
        if not variant.endswith("_lean"):
            assert np.array_equal(ctx.registers(), ref.initial[0])
            assert np.array_equal(ctx.sizes(), ref.initial[1])
        by_mode = {}
        for t, want in enumerate(ref.passes):
            has = ctx.step()
            assert has == want["has"], t
            assert np.array_equal(ctx.registers(), want["regs"]), "registers differ after pass %d" % t
            s, e = ctx.kahan()
            assert np.array_equal(s.view(np.uint64), want["ks"].view(np.uint64)), "Kahan sum differs after pass %d" % t
            assert np.array_equal(e.view(np.uint64), want["ke"].view(np.uint64)), "Kahan err differs after pass %d" % t
            assert np.array_equal(ctx.sizes(), want["sizes"]), "sizes differ after pass %d" % t
            assert ctx.state_hash() == want["hash"], t
            ps = ctx.pass_stats()[t]
            assert ps["changed"] == want["st"]["changed"], t
            assert ps["active_edges"] == want["st"]["active_edges"], t
            by_mode.setdefault(ps["mode"], []).append(want["moved_big"])
        assert not has
        ctx.finish()
        _check_final(ctx, ref.ids, ref.T, ref.vals, ref.keep, ctx.stats())
        assert np.array_equal(ctx.ranks(), hbo.rank_results(ref.vals[ref.keep]))
    assert FORCED_MODES.get(variant, {0}) <= set(by_mode), (variant, sorted(by_mode))
    # every pass mode this variant ran moved at least one row that holds a register above 47 (from the oracle's registers)
    assert all(max(moved) > 0 for moved in by_mode.values()), (variant, by_mode)


def test_deferred_epilogue_hands_over_in_every_pending_slot(gpu_ctx_factory):
    """The deferred epilogue of the dense fused node rows (hb_kernels.hip.h kEpi4) keeps up to four tiles pending per wave; lane (g, q)
    then owns row g of the q-th pending tile and gets a big counter's folded size as p_szfull / flag 8.  On the graph of about 1000 rows
    every workgroup has one tile, so only q = 0 owns anything.  Here: the same sources, sinks and hubs between 66 000 filler rows, one
    workgroup per compute unit (tune[0] = 1): 1044 tiles for 256 workgroups on the MI355X, and on the plan every one of the four slots
    holds rows of every kind - a register above 47 and no zero register, nothing above 47, sum-decided, zero-count-decided - next to
    rows without sources.  Registers, Kahan words and sizes after pass 0, the checksum and changed count after every pass, the final list."""
    ids, row_ptr, src = graphs.extreme_register_graph(1, chain=6, filler=66_000)
    o = hbo.Dense(np.ascontiguousarray(ids["lo"]), row_ptr, src)
    has, st = o.step(hbo.FRONTIER)
    kind = graphs.row_kinds(o.registers(), row_ptr)
    assert (o.sizes() == SATURATED).sum() >= 1 and int((kind == graphs.BIG_FULL).sum()) >= 100
    every = {graphs.BIG_FULL, graphs.SMALL_FULL, graphs.BY_SUM, graphs.BY_ZERO_COUNT, graphs.NO_SOURCES}
    with gpu_ctx_factory(tune=(1,)) as ctx:
        ctx.load_dense(ids, row_ptr, src)
        order = ctx.plan()["order"][:len(ids)]
        for workgroups in (256, 2):  # MI355X: 256 compute units; the interpreted build: 2
            assert all(every <= slot for slot in graphs.flush_slots(order, kind, workgroups)), workgroups
        ctx.begin()
        assert ctx.step() == has
        assert np.array_equal(ctx.registers(), o.registers())
        assert np.array_equal(ctx.sizes(), o.sizes())
        for got, want in zip(ctx.kahan(), o.kahan()):
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        t = 0
        while True:
            assert ctx.state_hash() == o.state_hash(), t
            assert ctx.pass_stats()[t]["changed"] == st["changed"], t
            if not has:
                break
            has, st = o.step(hbo.FRONTIER)
            assert ctx.step() == has
            t += 1
        assert np.array_equal(ctx.sizes(), o.sizes())
        ctx.finish()
        vals, keep, k = o.finish()
        _check_final(ctx, ids, t + 1, vals, keep, ctx.stats())


def test_run_and_store_with_saturated_sizes(gpu_ctx_factory, tmp_path):
    """hb_run (the pipelined tail) twice on one context, then both stores: sizes of 2^64 - 1 give Kahan sums of about 1.8e19, which
    reach the result image, the normalisation (/ (n - 1): values of about 2e16), the ranks and the files bit for bit."""
    from tests import speedy_kv_reader as kv
    ref = graphs.extreme_reference()
    want_vals, want_ranks = ref.vals[ref.keep], hbo.rank_results(ref.vals[ref.keep])
    assert want_vals.max() > 1e16 and (ref.passes[-1]["sizes"] == SATURATED).sum() > 10
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(ref.ids, ref.row_ptr, ref.src)
        for again in range(2):
            st = ctx.run()
            _check_final(ctx, ref.ids, ref.T, ref.vals, ref.keep, st)
            assert ctx.state_hash() == ref.final_hash, again
            assert np.array_equal(ctx.sizes(), ref.passes[-1]["sizes"]), again
            assert np.array_equal(ctx.ranks(), want_ranks), again
        ids, vals = ctx.results()
        ranks = ctx.ranks()
        ctx.store_harmonic(str(tmp_path / "dev"))
    _lib.store_harmonic(str(tmp_path / "host"), ids, vals, ranks)
    ints = kv.ids_to_ints(ids)
    for where in ("dev", "host"):
        cen = kv.Db(str(tmp_path / where / "harmonic"), "f64", str(tmp_path))
        rnk = kv.Db(str(tmp_path / where / "harmonic_rank"), "u64", str(tmp_path))
        assert len(cen) == len(rnk) == ref.k
        got = dict(cen.items())
        assert [np.float64(got[i]).view(np.uint64) for i in ints] == want_vals.view(np.uint64).tolist(), where
        assert dict(rnk.items()) == dict(zip(ints, want_ranks.tolist())), where


def test_records_with_crafted_ids(gpu_ctx_factory):
    """The same graph as raw SmallEdge records, in two batches with duplicates, through hb_append_edges and the device ingest (ids whose
    low halves are inverted hashes, told apart from each other only as 128-bit values): the graph the device builds = the host
    ingest's = the fixture's, and the final list = the load_dense run's = the oracle's."""
    ref = graphs.extreme_reference()
    dst = np.repeat(np.arange(len(ref.ids)), np.diff(ref.row_ptr).astype(np.int64))
    e = np.zeros(len(ref.src), dtype=_lib.EDGE)
    e["from"], e["to"] = ref.ids[ref.src], ref.ids[dst]
    rng = np.random.default_rng(3)
    e = np.concatenate([e, e[rng.integers(0, len(e), 2000)]])[rng.permutation(len(e) + 2000)]
    cut = len(e) // 3
    host = _lib.host_ingest(e)
    assert np.array_equal(host[0], ref.ids) and np.array_equal(host[1], ref.row_ptr) and np.array_equal(host[2], ref.src) and host[3] == len(ref.src)
    graphs_seen = []
    for flags in (0, _lib.HB_FLAG_HOST_INGEST):
        with gpu_ctx_factory(flags=flags) as ctx:
            ctx.append_edges(e[:cut])
            ctx.append_edges(e[cut:])
            ctx.finalize()
            st = ctx.stats()
            graphs_seen.append((ctx.graph(), st["n"], st["m_unique"], st["m_eff"], st["m_input"]))
            if flags == 0:
                st = ctx.run()
                rec_ids, rec_vals = ctx.results()
                _check_final(ctx, ref.ids, ref.T, ref.vals, ref.keep, st)
                assert ctx.state_hash() == ref.final_hash
    (ga, *sa), (gb, *sb) = graphs_seen
    assert sa == sb == [len(ref.ids), len(ref.src), len(ref.src), len(e)]
    for x, y, z in zip(ga, gb, host):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    with gpu_ctx_factory() as ctx:
        ctx.load_dense(ref.ids, ref.row_ptr, ref.src)
        ctx.run()
        ids, vals = ctx.results()
    assert np.array_equal(ids, rec_ids) and np.array_equal(vals.view(np.uint64), rec_vals.view(np.uint64))


@pytest.mark.parametrize("mode", ["edge", "dest", "dest_changed"])
def test_logical_ranks_with_extreme_registers(gpu_ctx_factory, mode):
    """Two logical ranks on one device (test_logical_ranks_on_one_device): edge partition with all-reduce, destination partition with
    all-gather, and its changed-only form, whose wire holds a counter as 48 bytes of six-bit codes (hb_aux.hip.h pack6_quarter): here
    the codes 40, 47, 48, 51, 55, 58 and 63 (= 65) all travel, at every register index.  Registers of both ranks after every pass and
    the final list against the oracle."""
    ref = graphs.extreme_reference()
    seen = set(np.unique(ref.passes[-1]["regs"]).tolist())
    assert {48, 51, 55, 58, 65} <= seen and not (seen & set(range(59, 65)))  # the point of the six-bit case
    for j in range(64):
        assert {48, 51, 55, 58, 65} <= set(np.unique(ref.passes[0]["regs"][:, j]).tolist()), j
    world = 2
    flags = _lib.HB_FLAG_NO_RCCL | (_lib.HB_FLAG_DEST_PARTITION if mode.startswith("dest") else 0)
    flags |= _lib.HB_FLAG_CHANGED_ONLY if mode.endswith("_changed") else 0
    split = dist.partition_dense_by_dest if mode.startswith("dest") else dist.partition_dense
    ctxs = []
    try:
        for r in range(world):
            c = gpu_ctx_factory(rank=r, world_size=world, flags=flags, chunk=16, tune=(0, 0, 0, 7, 4))
            ctxs.append(c)
            rp, src = split(ref.row_ptr, ref.src, r, world)
            c.load_dense(ref.ids, rp, src)
            c.begin()
        for t, want in enumerate(ref.passes):
            for c in ctxs:
                c.step_local()
            _lib.Context.exchange(ctxs, 0)
            assert [c.step_finish() for c in ctxs] == [want["has"]] * world, t
            for r, c in enumerate(ctxs):
                assert np.array_equal(c.registers(), want["regs"]), "registers of rank %d differ after pass %d" % (r, t)
        _lib.Context.exchange(ctxs, 1)
        for c in ctxs:
            c.finish()
            _check_final(c, ref.ids, ref.T, ref.vals, ref.keep, c.stats())
            if mode == "dest_changed":
                assert c.stats()["wire_bytes"] > 0
    finally:
        for c in ctxs:
            c.close()
