"""The approximated harmonic centrality job on the AMPC shard (include/hb_ampc.h: hbu_fold_harmonic, hbu_export, hbu_graph_node_sketch;
kernels in stract_amd/csrc/hb_ampc_fold.hip.h; driver run_approx_harmonic_job in stract_amd/ampc.py) against tests/ampc_approx_ref.py and,
for the fold, against the route a coordinator had to take before: batch_get of the distances, the terms in host code, batch_upsert
(KAHAN_ADD).  Every comparison is exact, on bit patterns, except that a NaN equals a NaN: its sign and payload are not pinned (x86 and
gfx950 produce different default NaNs for inf - inf)."""
import ctypes
import math

import numpy as np
import pytest

from stract_amd import _lib, ampc
from tests import ampc_approx_ref as aref
from tests.ampc_slots import slot_hash
from tests.test_ampc_edges import distance_table
from tests.test_ampc_round import graph_of, interpreted, two_workers
from tests.test_ampc_values import assert_table, canon, dev_values, harmonic_graphs, key_int, u128

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
U64, KAHAN = ampc.KIND_U64, ampc.KIND_KAHAN
INF = math.inf
NORMS = [1.0, 1.0 / 3.0, 1.0 / 2657.0, INF]
NORM_IDS = ["one", "third", "2657th", "inf"]
EDGE_DISTANCES = [0, 1, 2, 3, 7, (1 << 53) + 1, M64]
PRIME_INV = pow(aref.LARGE_PRIME, -1, 1 << 64)


def kahan_table(model, capacity_hint=0):
    tab = ampc.ValueTable(KAHAN, capacity_hint=capacity_hint)
    if model:
        tab.batch_set(u128(list(model)), dev_values(KAHAN, model.values()))
    return tab


def composed_fold(distances, centralities, keys, norm, skip_zero=False):
    """today's route: the distances cross the link, the terms are made in host code, the pairs go back as one KAHAN_ADD upsert"""
    d, found = distances.batch_get(u128(keys))
    assert found.all()
    keep = d != 0 if skip_zero else np.ones(len(d), dtype=bool)
    pairs = np.zeros(int(keep.sum()), dtype=ampc.KAHAN)
    with np.errstate(all="ignore"):
        pairs["sum"] = (np.float64(1.0) / d[keep].astype(np.float64)) * np.float64(norm)
    acts = centralities.batch_upsert(ampc.OP_KAHAN_ADD, u128(keys)[keep], pairs)
    return len(acts), int((acts == ampc.INSERTED).sum())


def items_of(tab, kind):
    """items() as {key: canonical bit patterns}; every key once"""
    keys, values = tab.items()
    assert len(keys) == len(values) == len(tab)
    if not len(keys):
        return {}
    bits = canon(kind, values) if kind != ampc.KIND_HLL64 else values
    out = {key_int(k): tuple(np.atleast_1d(b).tolist()) for k, b in zip(keys, bits)}
    assert len(out) == len(keys), "a key twice"
    return out


def model_items(kind, model):
    keys = list(model)
    if not keys:
        return {}
    if kind == ampc.KIND_HLL64:
        return {k: tuple(model[k].tolist()) for k in keys}
    bits = canon(kind, dev_values(kind, [model[k] for k in keys]))
    return {k: tuple(np.atleast_1d(b).tolist()) for k, b in zip(keys, bits)}


def fold_checked(dist_model, d_cent, m_cent, d_composed, space, norm, skip_zero=False, what=""):
    """one fold on the device, in the model and (norm > 0) along the composed route into d_composed: counts, both tables through
    batch_get over `space` and through items(), the distance table untouched"""
    with distance_table(dist_model) as d_dist:
        got = ampc.fold_harmonic(d_dist, d_cent, norm, skip_zero)
        want = aref.fold(m_cent, dist_model, norm, skip_zero)
        assert got == want, what
        assert_table(d_cent, KAHAN, m_cent, space, what)
        assert items_of(d_cent, KAHAN) == model_items(KAHAN, m_cent), what
        assert_table(d_dist, U64, dist_model, space, what)
        if d_composed is not None:
            assert composed_fold(d_dist, d_composed, list(dist_model), norm, skip_zero) == want, what
            assert items_of(d_composed, KAHAN) == items_of(d_cent, KAHAN), what
    return got


def id_pool(rng, n):
    """ids with high halves; the first two share their low half"""
    lo = rng.integers(1, 1 << 62, n).tolist()
    hi = rng.integers(0, 1 << 30, n).tolist()
    ids = [int(a) | (int(b) << 64) for a, b in zip(lo, hi)]
    ids[1] = (ids[0] & M64) | (((ids[0] >> 64) + 1) << 64)
    assert len(set(ids)) == n
    return ids


# ---- 1. the fold ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("present", ["all_present", "all_absent", "mixed"])
@pytest.mark.parametrize("entries", [0, 1, 63, 64, 65])
def test_fold_against_the_model_and_the_composed_route(entries, present):
    """Distance tables of 0, 1, 63, 64, 65 entries (a wave and one more / less) into a centrality table of 40 keys that holds all, none or
    every other of them; two ids with one low half; two folds, so every absent key is inserted and then added to"""
    rng = np.random.default_rng(entries * 3 + len(present))
    ids = id_pool(rng, 140)
    dist = {k: int(d) for k, d in zip(ids[:entries], rng.integers(1, 8, entries))}
    held = {"all_present": ids[:40] if entries <= 40 else ids[:entries], "all_absent": ids[100:140], "mixed": ids[0:100:2]}[present]
    m_cent = {k: (float(x), float(e)) for k, x, e in zip(held, rng.random(len(held)), rng.random(len(held)) * 2.0 ** -54)}
    space = ids + [5, 6]
    with kahan_table(m_cent) as d_cent, kahan_table(m_cent) as d_comp:
        for turn, norm in enumerate([1.0 / 2657.0, 1.0 / 3.0]):
            folded, inserted = fold_checked(dist, d_cent, m_cent, d_comp, space, norm, what=(entries, present, turn))
            assert folded == entries
            if turn == 0:
                assert inserted == {"all_present": 0, "all_absent": entries, "mixed": len([k for k in dist if k not in held])}[present]
            else:
                assert inserted == 0


def test_fold_rebuilds_the_index():
    """500 keys receive 100 new ones (and 50 they hold): the index of 1024 slots passes 512 keys and is rebuilt inside the fold"""
    rng = np.random.default_rng(5)
    ids = id_pool(rng, 700)
    m_cent = {k: (float(x), 0.0) for k, x in zip(ids[:500], rng.random(500))}
    dist = {k: int(d) for k, d in zip(ids[450:600], rng.integers(1, 8, 150))}
    with kahan_table(m_cent) as d_cent, kahan_table(m_cent) as d_comp:
        assert fold_checked(dist, d_cent, m_cent, d_comp, ids, 1.0 / 2657.0) == (150, 100)
        assert len(d_cent) == 600
        assert fold_checked(dist, d_cent, m_cent, d_comp, ids, 1.0 / 2657.0) == (150, 0)


def test_fold_grows_the_value_table():
    """1000 values become 1025: past the first value capacity (1024 rows) inside the fold; the rows that move keep their bits"""
    rng = np.random.default_rng(6)
    ids = id_pool(rng, 1100)
    m_cent = {k: (float(x), float(e)) for k, x, e in zip(ids[:1000], rng.random(1000), rng.random(1000) * 2.0 ** -55)}
    dist = {k: int(d) for k, d in zip(ids[990:1025], rng.integers(1, 8, 35))}
    with kahan_table(m_cent) as d_cent, kahan_table(m_cent) as d_comp:
        assert fold_checked(dist, d_cent, m_cent, d_comp, ids, 0.5) == (35, 25)
        assert len(d_cent) == 1025


def test_fold_and_export_reach_the_first_and_the_last_slot():
    """A table of up to 512 keys has an index of 1024 slots.  Keys whose home is slot 1023 (two of them: the second wraps round to slot 0
    or beyond) and slot 0, alone in the distance table: a loop over the slots that stops one short, or starts one late, loses them"""
    last = [k for k in range(1, 40000) if slot_hash(k) & 1023 == 1023][:2]
    first = [k | (9 << 64) for k in range(1, 40000) if slot_hash(k | (9 << 64)) & 1023 == 0][:1]
    assert len(last) == 2 and len(first) == 1
    for keys in ([last[0]], last, first, last + first):
        dist = {k: i + 1 for i, k in enumerate(keys)}
        m_cent = {}
        with kahan_table({}) as d_cent, kahan_table({}) as d_comp:
            assert fold_checked(dist, d_cent, m_cent, d_comp, last + first + [1], 0.5) == (len(keys), len(keys))
            assert fold_checked(dist, d_cent, m_cent, d_comp, last + first + [1], 0.5) == (len(keys), 0)
            assert sorted(items_of(d_cent, KAHAN)) == sorted(keys)


@pytest.mark.parametrize("norm", NORMS, ids=NORM_IDS)
def test_fold_edge_distances_and_norms(norm):
    """Distances 0, 1, 2, 3, 7, 2^53 + 1 (rounds to 2^53) and 2^64 - 1 (rounds to 2^64), present and absent, under every norm; three
    folds: insert or add, add, add (the zero distance walks through inf, NaN err, NaN sum)"""
    ids = [100 + i for i in range(len(EDGE_DISTANCES))] + [(200 + i) | (3 << 64) for i in range(len(EDGE_DISTANCES))]
    dist = dict(zip(ids, EDGE_DISTANCES + EDGE_DISTANCES))
    m_cent = {k: (0.125 * (i + 1), 2.0 ** -60) for i, k in enumerate(ids[:len(EDGE_DISTANCES)])}
    with kahan_table(m_cent) as d_cent, kahan_table(m_cent) as d_comp:
        for turn in range(3):
            got = fold_checked(dist, d_cent, m_cent, d_comp, ids + [1], norm, what=(norm, turn))
            assert got == (14, 7 if turn == 0 else 0)
    if norm == 1.0:
        assert m_cent[ids[12]][0] == 3 * 2.0 ** -53 and m_cent[ids[13]][0] == 3 * 2.0 ** -64


@pytest.mark.parametrize("skip_zero", [False, True], ids=["as_the_reference", "skip_zero"])
def test_three_folds_of_a_zero_distance(skip_zero):
    """A table holding the source (distance 0) and a neighbour, folded three times into an empty table: the source is inf, then err = NaN,
    then sum = NaN; with HBU_FOLD_SKIP_ZERO it never appears and is not counted"""
    dist = {7: 0, 8 | (1 << 64): 2}
    m_cent, seen = {}, []
    with kahan_table({}) as d_cent, kahan_table({}) as d_comp:
        for turn in range(3):
            got = fold_checked(dist, d_cent, m_cent, d_comp, [7, 8, 8 | (1 << 64)], 0.5, skip_zero, what=turn)
            assert got == ((1, 1 if turn == 0 else 0) if skip_zero else (2, 2 if turn == 0 else 0))
            seen.append(items_of(d_cent, KAHAN).get(7))
    nan, inf = 0x7FF8000000000000, aref.bits(INF)
    assert seen == ([None, None, None] if skip_zero else [(inf, 0), (inf, nan), (nan, nan)])
    assert m_cent[8 | (1 << 64)][0] == 0.75


def test_fold_is_not_contracted():
    """tests/test_ampc_approx_ref.py's fixture through six folds: a fold whose `(1 / d) * norm - err` is one fused operation ends with
    err = -2^-64"""
    norm = 1.0 / (aref.CONTRACTION_NUM_SAMPLES - 1)
    node, m_cent = 42 | (7 << 64), {}
    with kahan_table({}) as d_cent, kahan_table({}) as d_comp:
        for turn, d in enumerate(aref.CONTRACTION_DISTANCES):
            fold_checked({node: d}, d_cent, m_cent, d_comp, [node, 42], norm, what=turn)
        (_, values) = d_cent.items()
    assert float(values["err"][0]) == -(2.0 ** -65) and float(values["sum"][0]) == 0.0008907288922343495


def test_fold_of_an_empty_table_touches_nothing():
    m_cent = {3: (1.5, 2.0 ** -70)}
    with kahan_table(m_cent) as d_cent, ampc.ValueTable(U64) as d_dist:
        assert ampc.fold_harmonic(d_dist, d_cent, 0.25) == (0, 0)
        assert ampc.fold_harmonic(d_dist, d_cent, 0.25, skip_zero=True) == (0, 0)
        assert_table(d_cent, KAHAN, m_cent, [3, 4], "empty")


FOLD_REFUSALS = ["null_distances", "null_centralities", "distances_of_another_kind", "centralities_of_another_kind", "swapped", "unknown_flags",
                 "other_device"]


@pytest.mark.parametrize("refusal", FOLD_REFUSALS)
def test_fold_refuses_and_changes_nothing(refusal):
    """NULL, a wrong kind on either side, unknown flag bits, tables on two devices: HB_ERR_INVALID, the message on `centralities`, zero
    counts, and a read-back of both tables equals the one before.  (A broken table cannot be made through the API without a failed
    batch; that refusal is one line beside the others and is not provoked here.)"""
    lib = _lib.load()
    dist, m_cent = {1: 1, 2: 0, 3: 5}, {2: (1.0, 2.0 ** -60), 9: (0.5, 0.0)}
    space = [1, 2, 3, 9, 10]
    far = None
    with distance_table(dist) as d_dist, kahan_table(m_cent) as d_cent, ampc.ValueTable(ampc.KIND_F64) as other:
        other.batch_set(u128([1]), dev_values(ampc.KIND_F64, [2.0]))
        folded, inserted = ctypes.c_uint64(77), ctypes.c_uint64(77)

        def call(d, c, flags=0):
            return lib.hbu_fold_harmonic(d.h if d is not None else None, c.h if c is not None else None, 0.5, flags, ctypes.byref(folded), ctypes.byref(inserted))

        blamed = d_cent
        try:
            if refusal == "null_distances":
                rc = call(None, d_cent)
            elif refusal == "null_centralities":
                rc, blamed = call(d_dist, None), None
            elif refusal == "distances_of_another_kind":
                rc = call(other, d_cent)
            elif refusal == "centralities_of_another_kind":
                rc, blamed = call(d_dist, other), other
            elif refusal == "swapped":
                rc, blamed = call(d_cent, d_dist), d_dist
            elif refusal == "unknown_flags":
                rc = call(d_dist, d_cent, 2)
                assert call(d_dist, d_cent, 0x80000001) == _lib.HB_ERR_INVALID
            else:
                if _lib.device_count() < 2:
                    pytest.skip("needs two devices")
                far = ampc.ValueTable(U64, device=1)
                far.batch_set(u128([1]), dev_values(U64, [1]))
                rc = call(far, d_cent)
            assert rc == _lib.HB_ERR_INVALID and (folded.value, inserted.value) == (0, 0), refusal
            if blamed is not None:
                with pytest.raises(_lib.HyperballError) as err:
                    blamed._check(rc)
                assert str(err.value).split(": ", 1)[1], "no message"
            assert_table(d_dist, U64, dist, space, refusal)
            assert_table(d_cent, KAHAN, m_cent, space, refusal)
            assert items_of(d_cent, KAHAN) == model_items(KAHAN, m_cent)
            got, found = other.batch_get(u128(space))
            assert found.tolist() == [k == 1 for k in space] and len(other) == 1 and got[0] == 2.0
        finally:
            if far is not None:
                far.close()


# ---- 2. export --------------------------------------------------------------------------------------------------------------------
KINDS = [ampc.KIND_HLL64, ampc.KIND_U64, ampc.KIND_F32, ampc.KIND_F64, ampc.KIND_KAHAN]
KIND_IDS = ["hll64", "u64", "f32", "f64", "kahan"]


def model_table(kind, rng, ids):
    n = len(ids)
    if kind == ampc.KIND_HLL64:
        vals = list(rng.integers(0, 66, (n, 64)).astype(np.uint8))
    elif kind == ampc.KIND_U64:
        vals = [int(v) for v in rng.integers(0, 1 << 63, n)]
    elif kind == ampc.KIND_F32:
        vals = list(rng.random(n).astype(np.float32))
    elif kind == ampc.KIND_F64:
        vals = [float(v) for v in rng.random(n)]
    else:
        vals = [(float(a), float(b)) for a, b in zip(rng.random(n), rng.random(n) * 2.0 ** -53)]
    return dict(zip(ids, vals))


def device_table(kind, model):
    tab = ampc.CounterTable() if kind == ampc.KIND_HLL64 else ampc.ValueTable(kind)
    put(tab, kind, model)
    return tab


def put(tab, kind, model):
    if model:
        tab.batch_set(u128(list(model)), np.stack(list(model.values())) if kind == ampc.KIND_HLL64 else dev_values(kind, model.values()))


def assert_export(tab, kind, model, what):
    """items() equals the model as a set of pairs, and equals a batch_get of its own keys, position by position"""
    assert items_of(tab, kind) == model_items(kind, model), what
    keys, values = tab.items()
    got, found = tab.batch_get(keys)
    assert found.all() and np.array_equal(got.view(np.uint8), values.view(np.uint8)), what


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_export_every_kind(kind):
    """0, 1 and 1025 keys (the 1025 arrive in two batches: the index is rebuilt and the values grow in between), then a clone; the clone
    changes, the original's export does not"""
    rng = np.random.default_rng(kind + 10)
    ids = id_pool(rng, 1030)
    model = model_table(kind, rng, ids[:1025])
    first, rest = dict(list(model.items())[:1]), dict(list(model.items())[1:])
    with device_table(kind, {}) as tab:
        assert_export(tab, kind, {}, "empty")
        put(tab, kind, first)
        assert_export(tab, kind, first, "one key")
        put(tab, kind, dict(list(rest.items())[:399]))
        assert_export(tab, kind, dict(list(model.items())[:400]), "400 keys")
        put(tab, kind, rest)
        assert_export(tab, kind, model, "after the rebuild")
        with tab.clone() as copy:
            assert_export(copy, kind, model, "clone")
            extra = model_table(kind, rng, ids[1020:1030])
            put(copy, kind, extra)
            assert_export(copy, kind, {**model, **extra}, "changed clone")
            assert_export(tab, kind, model, "original")


def test_export_refuses_a_small_capacity():
    """capacity below len: HB_ERR_INVALID, nothing written, *written = 0; capacity above len is fine; NULL arrays only for an empty table"""
    lib = _lib.load()
    model = {k: k * 3 for k in range(1, 11)}
    with distance_table(model) as tab, ampc.ValueTable(U64) as empty:
        keys, values = np.zeros(12, dtype=_lib.U128), np.full(12, 0xAB, dtype=np.uint64)
        keys["lo"] = 0xAB
        written = ctypes.c_uint64(5)
        assert lib.hbu_export(tab.h, _lib._ptr(keys), _lib._ptr(values), 9, ctypes.byref(written)) == _lib.HB_ERR_INVALID
        assert written.value == 0 and (values == 0xAB).all() and (keys["lo"] == 0xAB).all()
        with pytest.raises(_lib.HyperballError) as err:
            tab._check(_lib.HB_ERR_INVALID)
        assert "capacity" in str(err.value)
        assert lib.hbu_export(tab.h, None, _lib._ptr(values), 12, ctypes.byref(written)) == _lib.HB_ERR_INVALID
        assert lib.hbu_export(tab.h, _lib._ptr(keys), None, 12, ctypes.byref(written)) == _lib.HB_ERR_INVALID
        assert lib.hbu_export(tab.h, _lib._ptr(keys), _lib._ptr(values), 12, None) == _lib.HB_ERR_INVALID
        assert (values == 0xAB).all()
        assert lib.hbu_export(tab.h, _lib._ptr(keys), _lib._ptr(values), 12, ctypes.byref(written)) == _lib.HB_OK
        assert written.value == 10 and {int(k["lo"]): int(v) for k, v in zip(keys[:10], values[:10])} == model
        assert (values[10:] == 0xAB).all()
        assert lib.hbu_export(empty.h, None, None, 0, ctypes.byref(written)) == _lib.HB_OK and written.value == 0


def test_large_fold_and_export():
    """2^23 + 1 keys: the distance table's index has 2^25 slots, more than the largest grid has threads (2^24), so the grid-stride loop
    of the fold and of the export takes a second turn.  Two folds (all inserted, then all added to) and the export, against numpy."""
    if interpreted():
        pytest.skip("2^25 slots thread by thread: the device only")
    n = (1 << 23) + 1
    keys = np.zeros(n, dtype=_lib.U128)
    keys["lo"] = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    keys["hi"] = np.arange(n, dtype=np.uint64) & np.uint64(3)
    d = (np.arange(n, dtype=np.uint64) % np.uint64(7)) + np.uint64(1)
    norm = 1.0 / 2657.0
    with ampc.ValueTable(U64) as dist, ampc.ValueTable(KAHAN) as cent:
        dist.batch_set(keys, d)
        assert ampc.fold_harmonic(dist, cent, norm) == (n, n)
        assert ampc.fold_harmonic(dist, cent, norm) == (n, 0)
        got_keys, got = cent.items()
        dk, dv = dist.items()
    assert len(got_keys) == n
    index = (got_keys["lo"] - np.uint64(1)) * np.uint64(pow(0x9E3779B97F4A7C15, -1, 1 << 64))  # wrapping: the key's number
    assert np.array_equal(np.sort(index), np.arange(n, dtype=np.uint64)) and np.array_equal(got_keys["hi"], index & np.uint64(3))
    v = (np.float64(1.0) / ((index % np.uint64(7)) + np.uint64(1)).astype(np.float64)) * np.float64(norm)
    t = v + v  # KahanSum{v, 0} += KahanSum{v, 0}
    assert np.array_equal(got["sum"].view(np.uint64), t.view(np.uint64))
    assert np.array_equal(got["err"].view(np.uint64), ((t - v) - v).view(np.uint64))
    dindex = (dk["lo"] - np.uint64(1)) * np.uint64(pow(0x9E3779B97F4A7C15, -1, 1 << 64))
    assert np.array_equal(np.sort(dindex), np.arange(n, dtype=np.uint64)) and np.array_equal(dv, (dindex % np.uint64(7)) + np.uint64(1))


# ---- 3. the node sketch -----------------------------------------------------------------------------------------------------------
def sketch_of(nodes):
    with graph_of(nodes, []) as g:
        return g.node_sketch()


def test_node_sketch_against_the_model():
    """0 nodes, 1 node, 5000 random ids (4096 registers: most are hit, many more than once); an id whose h << 12 is zero (p = 65) alone and
    among others of its register; two ids that differ in the high half only; two workers merged by a byte-wise max"""
    rng = np.random.default_rng(9)
    assert sketch_of([]).tolist() == [0] * 4096
    one = sketch_of([12345 | (5 << 64)])
    assert np.array_equal(one, aref.sketch([12345])) and np.count_nonzero(one) == 1
    ids = [int(a) | (int(b) << 64) for a, b in zip(rng.integers(0, 1 << 63, 5000), rng.integers(0, 1 << 20, 5000))]
    ids += [M64, 1 << 63, 0x8000000000000001]
    got = sketch_of(ids)
    assert got.dtype == np.uint8 and np.array_equal(got, aref.sketch(ids)) and np.count_nonzero(got) > 2500
    # register 65: h = j << 52
    zero_w = [(PRIME_INV * (j << 52)) & M64 for j in (0, 1, 4095)]
    assert [aref.sketch_register(k) for k in zero_w] == [(0, 65), (1, 65), (4095, 65)]
    low = [(PRIME_INV * ((1 << 52) | 1)) & M64, (PRIME_INV * ((1 << 52) | (1 << 51))) & M64]  # register 1 with p = 52 and p = 1
    got = sketch_of(low + zero_w + low)
    assert np.array_equal(got, aref.sketch(low + zero_w)) and got[0] == got[1] == got[4095] == 65
    assert np.array_equal(sketch_of(low), aref.sketch(low)) and sketch_of(low)[1] == 52
    # the high half is ignored
    assert np.array_equal(sketch_of([777 | (1 << 64), 777 | (2 << 64)]), aref.sketch([777]))
    # two workers
    a, b = ids[0::2], ids[1::2] + zero_w
    merged = np.maximum(sketch_of(a), sketch_of(b))
    assert np.array_equal(merged, aref.sketch_merge(aref.sketch(a), aref.sketch(b))) and np.array_equal(merged, aref.sketch(a + b))


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------------
def run_driver(workers, sources, n_samples, max_distance, space, skip_zero=False):
    model = aref.approx_harmonic_job(workers, sources, n_samples, max_distance, skip_zero)
    seen = []

    def on_source(state):
        cent, folded, inserted = next(model)
        seen.append(state["index"])
        assert (state["folded"], state["inserted"]) == (folded, inserted), state["index"]
        assert_table(state["centralities"], KAHAN, cent, space, state["index"])

    gs = [graph_of(n, e) for n, e in workers]
    try:
        result = ampc.run_approx_harmonic_job(gs, sources, n_samples, max_distance, skip_zero=skip_zero, on_source=on_source)
    finally:
        for g in gs:
            g.close()
    with pytest.raises(StopIteration) as done:
        next(model)
    want = done.value.value
    assert seen == list(range(len(sources)))
    assert result.keys() == want.keys()
    assert {k: aref.bits(v) for k, v in result.items()} == {k: aref.bits(v) for k, v in want.items()}
    return want


@pytest.mark.parametrize("skip_zero", [False, True], ids=["as_the_reference", "skip_zero"])
@pytest.mark.parametrize("max_distance", [1, 64])
@pytest.mark.parametrize("which", ["rmat", "fixture"])
def test_run_approx_harmonic_job(which, max_distance, skip_zero):
    """Two workers; the sources include a node without out-links, one source twice and nodes reached from several sources; max_distance 1
    and more than the diameter; after every source the centrality table and the fold's counts equal the model's, at the end the result.
    num_samples is larger than the number of sources: the norm comes from num_samples."""
    edges = dict(harmonic_graphs())[which]
    if which == "rmat":
        edges = edges[:600]
    sink = (1 << 90) | 5
    edges = edges + [(edges[0][0], sink), (edges[-1][0], sink)]  # (the fixture graph has no node without out-links of its own)
    nodes = sorted({x for e in edges for x in e})
    workers = two_workers(edges, nodes)
    with_out = {f for f, _ in edges}
    busy = [n for n in nodes if n in with_out][:3]
    sources = [busy[0], sink, busy[1], busy[0], busy[2]]
    want = run_driver(workers, sources, 9, max_distance, nodes + [1 << 100], skip_zero)
    assert len(want) >= 2
    if skip_zero:
        assert all(math.isfinite(v) for v in want.values())
    else:
        assert not math.isfinite(want[sink]) and not math.isfinite(want[busy[0]])  # inf, or NaN once more was folded in


def test_run_approx_harmonic_job_on_a_path_by_hand():
    """tests/test_ampc_approx_ref.py's a -> b -> c: {b: 1/2, c: 3/4} with the zero distances skipped; num_samples = 1 is norm = inf"""
    a, b, c = 10, 20 | (1 << 64), 30
    workers = [([a, b], [(a, b)]), ([c], [(b, c)])]
    assert run_driver(workers, [a, b], 3, 5, [a, b, c], skip_zero=True) == {b: 0.5, c: 0.75}
    assert run_driver(workers, [a, b], 3, 5, [a, b, c]) == {a: INF, b: INF, c: 0.75}
    assert run_driver(workers, [a], 1, 5, [a, b, c], skip_zero=True) == {b: INF, c: INF}
