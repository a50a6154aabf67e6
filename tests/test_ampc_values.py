"""The scalar value tables of the AMPC shard (include/hb_ampc.h: u64 / f32 / f64 / KahanSum tables with the five scalar upsert operators,
hbu_clone, hbu_update_centralities; kernels in stract_amd/csrc/hb_ampc_values.hip.h) against tests/ampc_ref.py, the restatement that
tests/test_ampc_ref.py pins on the reference's own answers.  Every comparison is exact: action codes and integers with ==, floats by
bit pattern.  One exception is written into canon(): every NaN compares equal to every NaN, because neither IEEE 754 nor Rust fixes
the sign and payload of a NaN an addition produces, the model's are those of the CPU the test runs on and the device's are its own."""
import collections
import json

import numpy as np
import pytest

from stract_amd import _lib, ampc, synth
from tests import ampc_ref as ref
from tests import graphs
from tests.test_ampc_ref import CASES, model_value

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
KIND_OPS = [(ampc.KIND_U64, ampc.OP_U64_ADD), (ampc.KIND_U64, ampc.OP_U64_MIN), (ampc.KIND_F32, ampc.OP_F32_ADD), (ampc.KIND_F64, ampc.OP_F64_ADD),
            (ampc.KIND_KAHAN, ampc.OP_KAHAN_ADD)]
IDS = ["u64_add", "u64_min", "f32_add", "f64_add", "kahan_add"]
KIND_NAMES = {"U64": ampc.KIND_U64, "F32": ampc.KIND_F32, "F64": ampc.KIND_F64, "KAHAN": ampc.KIND_KAHAN}
assert (ref.NO_CHANGE, ref.MERGED, ref.INSERTED) == (ampc.NO_CHANGE, ampc.MERGED, ampc.INSERTED)
assert (ref.HLL64, ref.U64_ADD, ref.U64_MIN, ref.F32_ADD, ref.F64_ADD, ref.KAHAN_ADD) == (ampc.OP_HLL64, ampc.OP_U64_ADD, ampc.OP_U64_MIN, ampc.OP_F32_ADD,
                                                                                             ampc.OP_F64_ADD, ampc.OP_KAHAN_ADD)


# ---- model values <-> device arrays ---------------------------------------------------------------------------------------------
def u128(ints):
    a = np.zeros(len(ints), dtype=_lib.U128)
    a["lo"] = np.array([k & M64 for k in ints], dtype=np.uint64)
    a["hi"] = np.array([k >> 64 for k in ints], dtype=np.uint64)
    return a


def key_int(k):
    return (int(k["hi"]) << 64) | int(k["lo"])


def dev_values(kind, values):
    """model values as the array the device takes"""
    values = list(values)
    if kind == ampc.KIND_KAHAN:
        a = np.zeros(len(values), dtype=ampc.KAHAN)
        a["sum"] = [v[0] for v in values]
        a["err"] = [v[1] for v in values]
        return a
    if kind == ampc.KIND_U64:
        return np.array(values, dtype=np.uint64).reshape(len(values))
    return np.array(values, dtype=ampc.DTYPES[kind]).reshape(len(values))


def canon(kind, arr):
    """bit patterns of a device array, every NaN as one pattern (see the module's docstring)"""
    if kind == ampc.KIND_U64:
        return arr.copy()
    if kind == ampc.KIND_F32:
        b = arr.view(np.uint32).copy()
        b[np.isnan(arr)] = 0x7FC00000
        return b
    f = arr.view(np.float64).reshape(len(arr), -1)  # F64: one column, KAHAN: (sum, err)
    b = f.view(np.uint64).copy()
    b[np.isnan(f)] = 0x7FF8000000000000
    return b


DEFAULT = {ampc.KIND_U64: 0, ampc.KIND_F32: np.float32(0.0), ampc.KIND_F64: 0.0, ampc.KIND_KAHAN: ref.KAHAN_DEFAULT}


def assert_table(tab, kind, model, space, what):
    """len and a batch_get of the whole key space: found flags, stored values, defaults for the absent keys"""
    assert len(tab) == len(model), what
    got, found = tab.batch_get(u128(space))
    assert found.tolist() == [k in model for k in space], what
    want = dev_values(kind, [model.get(k, DEFAULT[kind]) for k in space])
    assert np.array_equal(canon(kind, got), canon(kind, want)), what


def assert_counters(tab, model, space, what):
    assert len(tab) == len(model), what
    got, found = tab.batch_get(u128(space))
    assert found.tolist() == [k in model for k in space], what
    assert np.array_equal(got, np.stack([model.get(k, np.zeros(64, np.uint8)) for k in space])), what


def upsert_both(tab, kind, model, op, keys, values, what):
    acts = tab.batch_upsert(op, u128(keys), dev_values(kind, values))
    assert acts.tolist() == ref.batch_upsert(model, op, keys, values), what


# ---- values for which the order matters ---------------------------------------------------------------------------------------
def float_pool(rng, n, f32, tiny=False):
    """NaN, +-0.0, +-inf, subnormals and magnitudes 2^-30 .. 2^60 with random mantissas and signs; tiny: subnormals and zeros only
    (a key that only ever gets these shows whether subnormal sums are kept)"""
    sub = [1e-45, -1e-40, 3e-39] if f32 else [5e-324, -1e-310, 2e-308]
    out = []
    for _ in range(n):
        r = rng.random()
        if tiny:
            out.append(sub[rng.integers(0, 3)] if r < 0.8 else (0.0, -0.0)[rng.integers(0, 2)])
        elif r < 0.01:
            out.append(float("nan"))
        elif r < 0.02:
            out.append((float("inf"), float("-inf"))[rng.integers(0, 2)])
        elif r < 0.08:
            out.append((0.0, -0.0)[rng.integers(0, 2)])
        elif r < 0.12:
            out.append(sub[rng.integers(0, 3)])
        else:
            out.append(float((1.0 + rng.random()) * 2.0 ** int(rng.integers(-30, 61)) * (1, -1)[rng.integers(0, 2)]))
    return [np.float32(x) for x in out] if f32 else out


def value_pool(kind, rng, n, tiny=False):
    if kind == ampc.KIND_U64:
        special = [0, 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1]
        return [special[rng.integers(0, 6)] if rng.random() < 0.15 else int(rng.integers(0, 1 << 60)) >> int(rng.integers(0, 60)) for _ in range(n)]
    if kind == ampc.KIND_KAHAN:
        err = [0.0 if rng.random() < 0.5 else float(rng.standard_normal() * 2.0 ** int(rng.integers(-60, 8))) for _ in range(n)]
        return list(zip(float_pool(rng, n, False, tiny), err))
    return float_pool(rng, n, kind == ampc.KIND_F32, tiny)


def draw(kind, rng, keys, tiny_keys):
    """a value for every key of a batch; the keys of tiny_keys get subnormals and zeros only"""
    vals = value_pool(kind, rng, len(keys))
    tiny = value_pool(kind, rng, len(keys), tiny=True) if kind != ampc.KIND_U64 else vals
    return [t if k in tiny_keys else v for k, v, t in zip(keys, vals, tiny)]


@pytest.mark.parametrize("kind,op", KIND_OPS, ids=IDS)
def test_scalar_upserts_against_the_model(kind, op):
    """Ten steps of batches of 1 .. 3000 pairs over 400 keys; three hot keys take a fifth of every batch (long groups: the wave form),
    every fourth step is a batch_set.  Actions, len and the whole key space after every step."""
    rng = np.random.default_rng(100 + op)
    space = [int(x) for x in rng.integers(1, 1 << 62, 400)]
    space[5] = space[6] | (1 << 100)  # the same low half, another high half
    tiny_keys = set(space[:10])
    model = {}
    sizes = [1, 3000, 70, 1500] + [int(x) for x in rng.integers(1, 3001, 6)]
    with ampc.ValueTable(kind, capacity_hint=4) as tab:
        assert tab.kind == kind and len(tab) == 0
        for step, n in enumerate(sizes):
            hot = rng.integers(10, 400, 3)
            idx = np.where(rng.random(n) < 0.2, hot[rng.integers(0, 3, n)], rng.integers(0, min(400, 2 * n + 3), n))
            keys = [space[i] for i in idx]
            values = draw(kind, rng, keys, tiny_keys)
            if step % 4 == 3:
                tab.batch_set(u128(keys), dev_values(kind, values))
                ref.batch_set(model, keys, values)
            else:
                upsert_both(tab, kind, model, op, keys, values, step)
            assert_table(tab, kind, model, space, step)


@pytest.mark.parametrize("kind,op", KIND_OPS, ids=IDS)
def test_group_lengths_at_the_switch(kind, op):
    """One batch in which single keys occur exactly 1, 2, 3, 63, 64, 65, 127, 128, 129 and 4097 times and the switch length of the
    kernel (thread form up to it, wave form above) - 1, + 0, + 1 times, shuffled between each other and 300 single keys: the batch
    order of a key's pairs is not their order in memory.  Once on fresh keys (the first pair inserts), once more on the stored ones."""
    sw = ampc.wave_group_length()
    lengths = sorted({1, 2, 3, 63, 64, 65, 127, 128, 129, 4097, sw - 1, sw, sw + 1} - {0})
    rng = np.random.default_rng(7 + op)
    group_keys = [1000 + i for i in range(len(lengths))]
    occurrences = [k for k, n in zip(group_keys, lengths) for _ in range(n)] + [5000 + i for i in range(300)]
    space = group_keys + [5000 + i for i in range(300)] + [9999]
    model = {}
    with ampc.ValueTable(kind) as tab:
        for run in ("fresh", "stored"):
            keys = [occurrences[i] for i in rng.permutation(len(occurrences))]
            assert collections.Counter(keys)[group_keys[-1]] == 4097
            values = draw(kind, rng, keys, set())
            upsert_both(tab, kind, model, op, keys, values, run)
            assert_table(tab, kind, model, space, run)


def test_golden_value_cases():
    """tests/golden/ampc_value_cases.json (hand-written; tests/test_ampc_ref.py holds the model to it) replayed on the device"""
    with open(CASES) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        kind, op = KIND_NAMES[c["kind"]], getattr(ampc, "OP_" + c["op"])
        with ampc.ValueTable(kind) as tab:
            tab.batch_set(u128([k for k, _ in c["stored"]]), dev_values(kind, [model_value(c["kind"], v) for _, v in c["stored"]]))
            acts = tab.batch_upsert(op, u128([k for k, _ in c["batch"]]), dev_values(kind, [model_value(c["kind"], v) for _, v in c["batch"]]))
            assert acts.tolist() == c["actions"], c["name"]
            assert len(tab) == len(c["final"]), c["name"]
            got, found = tab.batch_get(u128([k for k, _ in c["final"]]))
            assert found.all(), c["name"]
            bits = canon(kind, got).reshape(len(got), -1)
            for row, (k, want) in zip(bits, c["final"]):
                want = want if isinstance(want, list) else [want]
                nan = {ampc.KIND_F32: 0x7FC00000}.get(kind, 0x7FF8000000000000)
                assert [int(x) for x in row] == [nan if w == "nan" else int(w, 16) for w in want], (c["name"], k)


def test_wrong_op_or_kind_is_refused_and_changes_nothing():
    """Every (kind, operator of another kind) pair, an unknown operator, the three counter calls on a scalar table, NULL with a count:
    HB_ERR_INVALID, and a batch_get of the whole key space afterwards equals the one before.  And the _values calls on a counter table
    are the three counter calls."""
    rng = np.random.default_rng(3)
    space = list(range(1, 41))
    keys = u128(space[:30])
    lib = _lib.load()
    junk = np.full(30 * 64, 0x3F, dtype=np.uint8)  # large enough for every kind
    acts = np.zeros(30, dtype=np.uint8)

    def refused(tab, rc):
        assert rc == _lib.HB_ERR_INVALID
        with pytest.raises(_lib.HyperballError):
            tab._check(rc)

    for kind in ampc.DTYPES:
        with ampc.ValueTable(kind) as tab:
            tab.batch_set(keys, dev_values(kind, value_pool(kind, rng, 30)))
            before, found_before = tab.batch_get(u128(space))

            def unchanged():
                got, found = tab.batch_get(u128(space))
                assert np.array_equal(found, found_before) and np.array_equal(canon(kind, got), canon(kind, before)) and len(tab) == 30

            for op in list(range(6)) + [6, 99]:
                if op in ampc.OPS[kind]:
                    continue
                refused(tab, lib.hbu_batch_upsert_values(tab.h, op, _lib._ptr(keys), _lib._ptr(junk), 30, _lib._ptr(acts)))
                unchanged()
            refused(tab, lib.hbu_batch_set(tab.h, _lib._ptr(keys), _lib._ptr(junk), 30))
            unchanged()
            refused(tab, lib.hbu_batch_upsert(tab.h, _lib._ptr(keys), _lib._ptr(junk), 30, _lib._ptr(acts)))
            unchanged()
            refused(tab, lib.hbu_batch_get(tab.h, _lib._ptr(keys), 30, _lib._ptr(junk), _lib._ptr(acts)))
            unchanged()
            refused(tab, lib.hbu_batch_set_values(tab.h, None, None, 5))
            refused(tab, lib.hbu_batch_upsert_values(tab.h, ampc.OPS[kind][0], _lib._ptr(keys), _lib._ptr(junk), 5, None))
            refused(tab, lib.hbu_batch_get_values(tab.h, None, 5, None, None))
            unchanged()
    with ampc.CounterTable() as tab:
        regs = graphs.random_registers(rng, 30)
        tab._check(lib.hbu_batch_set_values(tab.h, _lib._ptr(keys), _lib._ptr(regs), 30))
        before, found_before = tab.batch_get(u128(space))
        assert np.array_equal(before[:30], regs) and found_before.sum() == 30
        for op in range(1, 6):
            refused(tab, lib.hbu_batch_upsert_values(tab.h, op, _lib._ptr(keys), _lib._ptr(junk), 30, _lib._ptr(acts)))
            got, found = tab.batch_get(u128(space))
            assert np.array_equal(got, before) and np.array_equal(found, found_before)
        more = graphs.random_registers(rng, 30)
        tab._check(lib.hbu_batch_upsert_values(tab.h, ampc.OP_HLL64, _lib._ptr(keys), _lib._ptr(more), 30, _lib._ptr(acts)))
        merged = np.maximum(regs, more)
        assert acts.tolist() == [ampc.MERGED if (m != r).any() else ampc.NO_CHANGE for m, r in zip(merged, regs)]
        out, found = np.zeros((30, 64), np.uint8), np.zeros(30, np.uint8)
        tab._check(lib.hbu_batch_get_values(tab.h, _lib._ptr(keys), 30, _lib._ptr(out), _lib._ptr(found)))
        assert np.array_equal(out, merged) and found.all()
        kind, vbytes = (np.zeros(1, np.uint32) for _ in range(2))
        assert lib.hbu_kind(tab.h, kind.ctypes.data_as(lib.hbu_kind.argtypes[1]), vbytes.ctypes.data_as(lib.hbu_kind.argtypes[2])) == 0
        assert (int(kind[0]), int(vbytes[0])) == (ampc.KIND_HLL64, 64)


def test_clone_is_a_copy():
    """hbu_clone of a counter table and of a KahanSum table of 5000 keys that grew from room for 4 (the index was rebuilt several times
    on the way): equal content and len, and afterwards each follows its own model."""
    rng = np.random.default_rng(11)
    space = [int(x) for x in rng.integers(1, 1 << 62, 5000)] + [(1 << 70) + 5]
    stored = space[:5000]
    cuts = [(0, 60), (60, 1900), (1900, 5000)]
    # counters
    regs = graphs.random_registers(rng, 5000)
    model = {k: r for k, r in zip(stored, regs)}
    with ampc.CounterTable(capacity_hint=4) as tab:
        for a, b in cuts:
            tab.batch_set(u128(stored[a:b]), regs[a:b])
        with tab.clone() as twin:
            twin_model = ref.clone_table(model)
            assert_counters(twin, twin_model, space, "clone")
            for t, m, seed in ((tab, model, 1), (twin, twin_model, 2)):
                r2 = np.random.default_rng(seed)
                keys = [space[i] for i in r2.integers(0, len(space), 700)]
                vals = graphs.random_registers(r2, 700)
                assert t.batch_upsert(u128(keys), vals).tolist() == ref.batch_upsert(m, ref.HLL64, keys, list(vals))
            assert_counters(tab, model, space, "original")
            assert_counters(twin, twin_model, space, "clone after its own batch")
    # Kahan sums
    kind, op = ampc.KIND_KAHAN, ampc.OP_KAHAN_ADD
    values = value_pool(kind, rng, 5000)
    model = dict(zip(stored, values))
    with ampc.ValueTable(kind, capacity_hint=4) as tab:
        for a, b in cuts:
            tab.batch_set(u128(stored[a:b]), dev_values(kind, values[a:b]))
        with tab.clone() as twin:
            assert twin.kind == kind
            twin_model = ref.clone_table(model)
            assert_table(twin, kind, twin_model, space, "clone")
            for t, m, seed in ((tab, model, 1), (twin, twin_model, 2)):
                r2 = np.random.default_rng(seed)
                keys = [space[i] for i in r2.integers(0, len(space), 700)]
                upsert_both(t, kind, m, op, keys, value_pool(kind, r2, 700), seed)
            assert_table(tab, kind, model, space, "original")
            assert_table(twin, kind, twin_model, space, "clone after its own batch")
    with ampc.ValueTable(ampc.KIND_U64) as empty, empty.clone() as twin:
        assert len(twin) == 0 and not twin.batch_get(u128([1]))[1].any()


def size_branches(regs):
    """which exit of HyperLogLog<64>::size() (hyperloglog.rs:4484-4516) each counter takes: 0 linear counting (v zero registers,
    64 ln(64 / v) <= 40, i.e. v >= 35), 1 the bias-corrected range (e <= 320), 2 e > 320"""
    zeros = (regs == 0).sum(axis=1)
    e = 0.709 * 4096.0 / np.exp2(-regs.astype(np.float64)).sum(axis=1)
    return np.where(zeros >= 35, 0, np.where(e <= 320.0, 1, 2))


def test_update_centralities_against_the_model():
    """hbu_update_centralities on counters that take every exit of size() - linear counting, the bias-corrected range, e > 320, a register
    of 48..58 and of 65 (the counters of tests/test_extreme_registers.py's graph after its passes) - with nodes missing from the previous
    counters, from the next ones and from the centrality table, counters that did not grow (d == 0) and that shrank (saturating), nodes
    listed twice, rounds 0, 1 and 7: `written`, the whole next centrality table (sum and err bits), and the three tables it only reads."""
    rng = np.random.default_rng(21)
    ext = graphs.extreme_reference()
    big = np.concatenate([p["regs"] for p in ext.passes[:2]])
    big = big[(big > 47).any(axis=1)]
    assert ((big >= 48) & (big <= 58)).any() and (big == 65).any()
    pool = np.concatenate([graphs.random_registers(rng, 400), big[rng.permutation(len(big))[:150]]])
    branches = size_branches(pool)
    assert all((branches == b).sum() >= 20 for b in (0, 1, 2)), np.bincount(branches)
    n = len(pool)
    nodes = [int(x) | (i << 64) for i, x in enumerate(rng.integers(1, 1 << 62, n))]
    prev_c, next_c, prev_v = {}, {}, {}
    for i, k in enumerate(nodes):
        grown = np.maximum(pool[i], pool[rng.integers(0, n)])  # what an upsert makes of it
        how = i % 10
        if how != 0:
            prev_c[k] = pool[i] if how != 1 else grown        # how == 1: next is the smaller one (saturating_sub)
        if how != 2:
            next_c[k] = {1: pool[i], 3: pool[i]}.get(how, grown)  # how == 3: unchanged, d == 0
        if i % 3 != 0:
            prev_v[k] = (float(rng.integers(0, 1 << 40)) / 7.0, float(rng.standard_normal() * 1e-9))
    asked = [nodes[i] for i in rng.permutation(n)] + nodes[:50] + [12345]  # 50 nodes twice, one node nobody knows
    space = nodes + [12345]
    kind = ampc.KIND_KAHAN
    with ampc.CounterTable() as d_prev_c, ampc.CounterTable() as d_next_c, ampc.ValueTable(kind) as d_prev_v:
        d_prev_c.batch_set(u128(list(prev_c)), np.stack(list(prev_c.values())))
        d_next_c.batch_set(u128(list(next_c)), np.stack(list(next_c.values())))
        d_prev_v.batch_set(u128(list(prev_v)), dev_values(kind, prev_v.values()))
        for round_ in (0, 1, 7):
            with d_prev_v.clone() as d_next_v:  # init_from: the round's next table starts as a copy of prev
                next_v = ref.clone_table(prev_v)
                want = ref.update_centralities(prev_c, next_c, prev_v, next_v, asked, round_)
                assert 0 < want < n and len(next_v) > len(prev_v)  # some keys are new to the centrality table
                assert ampc.update_centralities(d_prev_c, d_next_c, d_prev_v, d_next_v, u128(asked), round_) == want
                assert_table(d_next_v, kind, next_v, space, round_)
                assert_table(d_prev_v, kind, prev_v, space, round_)
                assert_counters(d_prev_c, prev_c, space, round_)
                assert_counters(d_next_c, next_c, space, round_)
                assert ampc.update_centralities(d_prev_c, d_next_c, d_prev_v, d_next_v, u128([]), round_) == 0
        # refusals: kinds in the wrong places, one table as both centrality tables
        for args in ((d_prev_v, d_next_c, d_prev_v, d_prev_v), (d_prev_c, d_next_c, d_prev_c, d_prev_v), (d_prev_c, d_next_c, d_prev_v, d_prev_v)):
            with pytest.raises(_lib.HyperballError):
                ampc.update_centralities(*args, u128(asked), 0)
        assert_table(d_prev_v, kind, prev_v, space, "after the refusals")


def int_edges(ids, row_ptr, src):
    """(from, to) as ints, in the order of a CSR by destination"""
    name = [key_int(k) for k in ids]
    dst = np.repeat(np.arange(len(ids)), np.diff(row_ptr).astype(np.int64))
    return [(name[s], name[d]) for s, d in zip(src, dst)]


def harmonic_graphs():
    g = synth.RmatGraph(9, 3000)
    yield "rmat", int_edges(g.ids, g.row_ptr, g.src)
    yield "fixture", [(key_int(e["from"]), key_int(e["to"])) for e in graphs.fixture_graph().host_edges()]


@pytest.mark.parametrize("which", ["rmat", "fixture"])
def test_ampc_harmonic_rounds_on_device_tables(which):
    """The AMPC harmonic job's loop (harmonic_centrality/mapper.rs) with every table on the device: per round clone prev into next,
    then for each of two workers (edges i % 2) the old counters of edge.from for the edges whose source changed, batch_upsert into
    edge.to, the changed set from the Merged actions, update_centralities for the changed nodes, swap - until a round changes nothing.
    Both sides keep the changed set EXACTLY (the reference keeps a bloom filter, whose false positives only add work that changes nothing).
    After every round both counter tables and the centrality table equal the model's bit for bit."""
    edges = dict(harmonic_graphs())[which]
    nodes = sorted({x for e in edges for x in e})
    kind = ampc.KIND_KAHAN
    m_prev_c = {k: ref.hll_of(k) for k in nodes}  # setup_counters, mapper.rs:64-88
    m_prev_v = {}
    d_prev_c, d_prev_v = ampc.CounterTable(), ampc.ValueTable(kind)
    d_prev_c.batch_set(u128(nodes), np.stack([m_prev_c[k] for k in nodes]))
    changed, rounds = set(nodes), 0
    try:
        while changed:
            m_next_c, m_next_v = ref.clone_table(m_prev_c), ref.clone_table(m_prev_v)
            d_next_c, d_next_v = d_prev_c.clone(), d_prev_v.clone()
            new_changed = set()
            for worker in (0, 1):
                batch = [e for i, e in enumerate(edges) if i % 2 == worker and e[0] in changed]
                for b in range(0, len(batch), 1000):
                    part = batch[b:b + 1000]
                    keys, want = ref.update_counters(m_prev_c, m_next_c, part)
                    old, found = d_prev_c.batch_get(u128([f for f, _ in part]))  # get_old_counters
                    assert found.all()
                    for reg, (f, _) in zip(old, part):
                        ref.hbo.hll_add(reg, f)                                   # counter.add_u128(edge.from), on the worker
                    acts = d_next_c.batch_upsert(u128([t for _, t in part]), old)
                    assert acts.tolist() == want, rounds
                    new_changed |= {k for k, a in zip(keys, acts) if a == ampc.MERGED}
            ask = sorted(new_changed) + nodes[:3]  # (three nodes that may not have changed: d == 0 for them)
            want = ref.update_centralities(m_prev_c, m_next_c, m_prev_v, m_next_v, ask, rounds)
            assert ampc.update_centralities(d_prev_c, d_next_c, d_prev_v, d_next_v, u128(ask), rounds) == want
            assert_counters(d_prev_c, m_prev_c, nodes, rounds)
            assert_counters(d_next_c, m_next_c, nodes, rounds)
            assert_table(d_next_v, kind, m_next_v, nodes, rounds)
            d_prev_c.close()
            d_prev_v.close()
            d_prev_c, d_prev_v, m_prev_c, m_prev_v = d_next_c, d_next_v, m_next_c, m_next_v  # swap
            changed = new_changed
            rounds += 1
        assert rounds >= 3 and len(m_prev_v) > 0
    finally:
        d_prev_c.close()
        d_prev_v.close()


def test_ampc_shortest_path_rounds_on_device_tables():
    """The shortest-path job's RelaxEdges loop (shortest_path/mapper.rs:57-150) on a u64 table with U64Min: 300 nodes, 5000 edges, at
    most 2000 edges per batch, so the edges into one node arrive in several batches of a round.  The table equals the model after every
    round and plain BFS distances at the end."""
    edges = graphs.lcg_graph(300, 5000)
    source = 1
    kind = ampc.KIND_U64
    space = list(range(1, 301)) + [777]
    m_prev = {source: 0}
    d_prev = ampc.ValueTable(kind)
    d_prev.batch_set(u128([source]), dev_values(kind, [0]))
    changed, rounds = {source}, 0
    try:
        while changed:
            m_next, d_next = ref.clone_table(m_prev), d_prev.clone()
            new_changed = set()
            batch = [e for e in edges if e[0] in changed]
            for b in range(0, len(batch), 2000):
                part = batch[b:b + 2000]
                keys, want = ref.update_distances(m_prev, m_next, part)
                sources = sorted({f for f, _ in part})
                old, found = d_prev.batch_get(u128(sources))  # get_old_distances
                new = ref.new_distances({f: int(o) for f, o, ok in zip(sources, old, found) if ok}, part)
                assert list(new) == keys
                acts = d_next.batch_upsert(ampc.OP_U64_MIN, u128(keys), dev_values(kind, new.values()))
                assert acts.tolist() == want, rounds
                new_changed |= {k for k, a in zip(keys, acts) if a != ampc.NO_CHANGE}
            assert_table(d_next, kind, m_next, space, rounds)
            assert_table(d_prev, kind, m_prev, space, rounds)
            d_prev.close()
            d_prev, m_prev, changed = d_next, m_next, new_changed
            rounds += 1
        # plain breadth-first search
        out = collections.defaultdict(list)
        for f, t in edges:
            out[f].append(t)
        dist, frontier = {source: 0}, [source]
        while frontier:
            nxt = []
            for f in frontier:
                for t in out[f]:
                    if t not in dist:
                        dist[t] = dist[f] + 1
                        nxt.append(t)
            frontier = nxt
        assert m_prev == dist and rounds == max(dist.values()) + 1 and len(dist) > 250
        assert_table(d_prev, kind, dist, space, "bfs")
    finally:
        d_prev.close()


def test_batch_sizes_across_the_work_memory_pieces():
    """One u64 table and one exact ChangedFilter through batches of 1, 16, 17, 64, 65, 257, 17 and 1: 16 and 17 sixteen-byte keys straddle
    one 256-byte piece of the work memory, 64 and 65 groups one block of the group kernels, and the last two batches are smaller than the
    work memory they find.  Every call that lays the work memory out runs at every size - batch_upsert (U64_MIN, keys repeated inside the
    batch), batch_get of present and absent keys, items(), and the filter's insert, contains and export_ids - and every answer equals a
    dict / set model exactly."""
    rng = np.random.default_rng(41)
    kind, op = ampc.KIND_U64, ampc.OP_U64_MIN

    def name(i):
        return i | ((i % 3) << 100)

    model, members = {}, set()
    with ampc.ValueTable(kind, capacity_hint=4) as tab, ampc.ChangedFilter.exact() as filt:
        for step, n in enumerate([1, 16, 17, 64, 65, 257, 17, 1]):
            what = (step, n)
            fresh = [name(1000 * (step + 1) + i) for i in range(max(1, 2 * n // 3))]
            pool = fresh + list(model)[:5]
            keys = [pool[i] for i in rng.integers(0, len(pool), n)]
            if n > 1:
                keys[-1] = keys[0]  # (whatever the draw: one key twice)
            upsert_both(tab, kind, model, op, keys, value_pool(kind, rng, n), what)
            known = list(model)
            ask = [known[i % len(known)] if i % 2 == 0 else name(500_000 + 1000 * step + i) for i in range(n)]
            assert sum(k in model for k in ask) == (n + 1) // 2, what
            assert_table(tab, kind, model, ask, what)
            got_keys, got_vals = tab.items()
            assert len(got_keys) == len(model), what
            assert {key_int(k): int(v) for k, v in zip(got_keys, got_vals)} == model, what
            ids = [keys[i] if i % 3 else name(900_000 + 1000 * step + i) for i in range(n)]
            filt.insert(u128(ids))
            members |= set(ids)
            assert filt.count() == len(members), what
            assert filt.contains(u128(ask)).tolist() == [k in members for k in ask], what
            assert filt.contains(u128(ids)).all(), what
            out = filt.export_ids()
            assert len(out) == len(members) and {key_int(k) for k in out} == members, what
