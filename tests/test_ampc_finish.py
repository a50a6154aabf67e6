"""The finish of an AMPC job on the shard (include/hb_ampc.h: hbu_finish_centralities, hbu_top_centralities, hbu_store_centralities; kernels
in stract_amd/csrc/hb_ampc_finish.hip.h, the sorts in hb_ingest.hip; Python in stract_amd/ampc.py) against tests/ampc_finish_ref.py and,
for the store, against the host route hb_store_harmonic on the arrays the finish returns.  Every comparison is on bit patterns, except that
a NaN equals a NaN: x86 and gfx950 produce different default NaNs (tests/test_ampc_approx.py).  Because of that the ranks and the top lists
are checked against the model applied to the values the call itself returned, and the values against the model separately.
Not reached here: the refusal of a broken table (it takes a HIP error inside a batch to break one)."""
import ctypes
import hashlib
import math
import os
import struct

import numpy as np
import pytest

from stract_amd import _lib, ampc
from tests import ampc_finish_ref as fref
from tests import speedy_kv_reader as kv
from tests.test_ampc_round import graph_of, interpreted, two_workers
from tests.test_ampc_values import assert_table, dev_values, harmonic_graphs, u128

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
F64, KAHAN = ampc.KIND_F64, ampc.KIND_KAHAN
KINDS = [KAHAN, F64]
KIND_IDS = ["kahan", "f64"]
INF = math.inf
POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
TINY = 5e-324
DIVISORS = [1.0, 3.0, 2657.0, 0.0, -1.0, INF]
DIVISOR_IDS = ["one", "three", "2657", "zero", "minus_one", "inf"]
# both sides of every boundary of the bincode varint classes (1, 3, 5, 9, 17 key bytes)
CLASS_IDS = [0, 1, 5, 250, 251, 252, 253, 254, 65535, 65536, 65537, (1 << 32) - 1, 1 << 32, (1 << 32) + 9, M64, 1 << 64, (1 << 64) + 1, (1 << 100) + 7,
             (1 << 127) + 3, (1 << 128) - 1, 3 << 40]
POISON = 0xABABABABABABABAB


def fbits(vals):
    """bit patterns of f64 values, every NaN as one pattern"""
    a = np.ascontiguousarray(vals, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b.tolist()


def ints(ids):
    return kv.ids_to_ints(ids)


def hashed_ids(rng, n):
    """hashed-looking ids: both words random; the first two share their low word, the next two their high word"""
    lo = [int(x) for x in rng.integers(0, 1 << 63, n, dtype=np.uint64)]
    hi = [int(x) for x in rng.integers(0, 1 << 63, n, dtype=np.uint64)]
    if n >= 4:
        lo[1] = lo[0]
        hi[1] = hi[0] + 1
        hi[3] = hi[2]
        lo[3] = lo[2] + 1
    ids = [(h << 64) | l for l, h in zip(lo, hi)]
    assert len(set(ids)) == n
    return ids


def as_model(kind, ids, values, rng=None):
    """{id: what the table stores}: an f64, or a KahanSum whose err is NOT zero - it must not leak into the value"""
    if kind == F64:
        return {k: float(v) for k, v in zip(ids, values)}
    errs = rng.random(len(ids)) + 0.5 if rng is not None else np.full(len(ids), 0.75)
    return {k: (float(v), float(e)) for k, v, e in zip(ids, values, errs)}


def value_of(kind, stored):
    return stored if kind == F64 else stored[0]


def table_of(kind, model, batches=(None,)):
    """a table holding `model`, set in consecutive batches of the given sizes (None: the rest)"""
    tab = ampc.ValueTable(kind)
    keys, at = list(model), 0
    for size in batches:
        part = keys[at:] if size is None else keys[at:at + size]
        at += len(part)
        if part:
            tab.batch_set(u128(part), dev_values(kind, [model[k] for k in part]))
    assert at == len(keys)
    return tab


def check(tab, kind, model, divisor, ks=None, what=""):
    """finish and top of `tab` against the model; the table reads back unchanged afterwards.  Returns (ids, vals, ranks)."""
    n = len(model)
    ids, vals, ranks = ampc.finish_centralities(tab, divisor)
    want_ids, want_vals, _ = fref.finish({k: value_of(kind, v) for k, v in model.items()}, divisor)
    got_ids = ints(ids)
    assert got_ids == want_ids, what
    assert fbits(vals) == fbits(want_vals), what
    assert np.array_equal(np.isnan(vals), np.isnan(want_vals)), what
    assert ranks.tolist() == fref.ranks_of(got_ids, vals.tolist()), what
    for k in (0, 1, n - 1, n, n + 1, 1 << 40) if ks is None else ks:
        if k < 0:
            continue
        tids, tvals = ampc.top_centralities(tab, k, divisor)
        want = fref.top(got_ids, vals.tolist(), k)
        assert len(tids) == len(tvals) == min(k, n) == len(want), (what, k)
        assert ints(tids) == [i for i, _ in want], (what, k)
        assert fbits(tvals) == fbits([v for _, v in want]), (what, k)
    assert_table(tab, kind, model, list(model) + [2, (1 << 120) | 9], what)
    return ids, vals, ranks


# ---- 1. sizes: one block of the kernel and its edges, a grown value array, a rebuilt index, a clone, many blocks -----------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_finish_and_top_sizes(n, kind):
    """0 .. 257 keys: hashed-looking ids, values drawn from 7 levels (ties everywhere, the ids decide), the divisor inexact"""
    rng = np.random.default_rng(100 + n)
    ids = hashed_ids(rng, n)
    model = as_model(kind, ids, rng.integers(0, 7, n).astype(np.float64) / 8.0 + 1.0, rng)
    with table_of(kind, model) as tab:
        check(tab, kind, model, 2657.0, what=(n, kind))
        check(tab, kind, model, 1.0, ks=[n], what=(n, kind, "one"))


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_finish_after_the_value_array_grew(kind):
    """1000 keys, then 25 more: past the first value capacity (1024 rows), so the rows were copied to a new array"""
    rng = np.random.default_rng(7)
    ids = hashed_ids(rng, 1025)
    model = as_model(kind, ids, rng.integers(0, 50, 1025).astype(np.float64), rng)
    with table_of(kind, model, (1000, None)) as tab:
        check(tab, kind, model, 3.0, ks=[0, 1, 1000, 1024, 1025, 1026])


def test_finish_after_the_index_was_rebuilt():
    """500 keys, then 100 more: the index of 1024 slots passes 512 keys and is rebuilt; entry numbers survive, slots do not"""
    rng = np.random.default_rng(8)
    ids = hashed_ids(rng, 600)
    model = as_model(KAHAN, ids, rng.random(600), rng)
    with table_of(KAHAN, model, (500, None)) as tab:
        check(tab, KAHAN, model, 599.0, ks=[1, 599, 600])


def test_finish_of_a_clone():
    """a clone finishes like its source, also after the two went different ways"""
    rng = np.random.default_rng(9)
    ids = hashed_ids(rng, 300)
    model = as_model(KAHAN, ids[:280], rng.integers(0, 9, 280).astype(np.float64), rng)
    with table_of(KAHAN, model) as tab, tab.clone() as twin:
        check(twin, KAHAN, model, 2657.0, ks=[1, 280])
        more = as_model(KAHAN, ids[270:], rng.integers(20, 30, 30).astype(np.float64), rng)  # 10 overwritten, 20 new: only in the clone
        twin.batch_set(u128(list(more)), dev_values(KAHAN, more.values()))
        check(twin, KAHAN, {**model, **more}, 2657.0, ks=[1, 25, 300])
        check(tab, KAHAN, model, 2657.0, ks=[1, 280])


def test_finish_top_and_store_at_100001_keys(tmp_path):
    """100 001 keys: hundreds of blocks, and far above the size where the device sorts go from one block to several passes.  The model is
    numpy here (np.lexsort over (id, descending key)), the store is compared with the host route."""
    if interpreted():
        pytest.skip("100 001 keys through every sort pass thread by thread: the device only")
    n = 100_001
    keys = np.zeros(n, dtype=_lib.U128)
    keys["lo"] = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    keys["hi"] = (np.arange(n, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)) >> np.uint64(62)
    values = np.zeros(n, dtype=ampc.KAHAN)
    values["sum"] = (np.arange(n, dtype=np.uint64) % np.uint64(1000)).astype(np.float64) - 100.0  # 1000 levels, negatives among them
    values["err"] = 0.25
    with ampc.ValueTable(KAHAN) as tab:
        tab.batch_set(keys, values)
        ids, vals, ranks = tab.finish_centralities(2657.0)
        order = np.lexsort((keys["lo"], keys["hi"]))
        assert np.array_equal(ids, keys[order])
        want = values["sum"][order] / np.float64(2657.0)
        assert np.array_equal(vals.view(np.uint64), want.view(np.uint64))
        b = vals.view(np.uint64)
        key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
        by_rank = np.lexsort((np.arange(n), ~key))  # (ids are ascending: the position is the id order)
        want_ranks = np.zeros(n, dtype=np.uint64)
        want_ranks[by_rank] = np.arange(n, dtype=np.uint64)
        assert np.array_equal(ranks, want_ranks)
        tids, tvals = tab.top_centralities(50_000, 2657.0)
        assert np.array_equal(tids, ids[by_rank[:50_000]]) and np.array_equal(tvals.view(np.uint64), b[by_rank[:50_000]])
        assert_same_store(tab, 2657.0, tmp_path, ids, vals, ranks)
        got, found = tab.batch_get(keys[:1000])
        assert found.all() and np.array_equal(got.view(np.uint64), values[:1000].view(np.uint64))


# ---- 2. ids: 128 bits in both orders, every key-length class ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_id_order_and_tie_order_are_128_bit(kind):
    """pairs that differ only in the high word and pairs that differ only in the low word, the high-word pairs chosen so that the LOW
    word alone would order them the other way; all values equal, so the ranks ARE the id order"""
    ids = []
    for i in range(40):
        ids += [(i << 64) | (1000 - i), ((i + 1) << 64) | (1000 - i - 500), (i << 64) | (2000 + i), (i << 64) | (2001 + i + 40)]
    ids += CLASS_IDS
    ids = list(dict.fromkeys(ids))
    model = as_model(kind, ids, [2.5] * len(ids))
    with table_of(kind, model) as tab:
        got_ids, vals, ranks = check(tab, kind, model, 1.0, ks=[1, 7, len(ids)])
        assert ints(got_ids) == sorted(ids) and ranks.tolist() == list(range(len(ids)))


def test_300_equal_values_rank_in_id_order():
    rng = np.random.default_rng(11)
    ids = hashed_ids(rng, 300)
    model = as_model(KAHAN, ids, [1.0] * 300, rng)
    with table_of(KAHAN, model) as tab:
        _, vals, ranks = check(tab, KAHAN, model, 3.0, ks=[1, 299, 300])
        assert ranks.tolist() == list(range(300)) and len(set(fbits(vals))) == 1


def test_two_tie_groups_and_k_cutting_through_one():
    """150 keys at 2.0 and 150 at 1.0, interleaved in id order: k = 100 cuts the first group, 200 the second, 150 falls between them"""
    rng = np.random.default_rng(12)
    ids = sorted(hashed_ids(rng, 300))
    model = as_model(KAHAN, ids, [2.0 if i % 2 else 1.0 for i in range(300)], rng)
    with table_of(KAHAN, model) as tab:
        check(tab, KAHAN, model, 2657.0, ks=[100, 149, 150, 151, 200])
        tids, _ = tab.top_centralities(100, 2657.0)
        assert ints(tids) == ids[1::2][:100]


# ---- 3. values and divisors ---------------------------------------------------------------------------------------------------------
SPECIAL = [INF, -INF, 0.0, -0.0, POS_NAN, NEG_NAN, -1.0, -2.5, -1e300, TINY, -TINY, 2.2250738585072014e-308, 1e-310, -1e-310, 1.0, 2.0, 1e300, 0.1, 1.0 / 3.0,
           INF, -0.0, POS_NAN, 1.0, -1.0]


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("divisor", DIVISORS, ids=DIVISOR_IDS)
def test_special_values_under_every_divisor(divisor, kind):
    """both infinities, both zeros, both NaN signs, negatives, subnormals, each twice somewhere (ties among them), on ids of every key
    class: every key is a result, nothing is dropped; -1.0 reverses the order, 0.0 and inf fold the values onto inf / NaN / zeros"""
    ids = CLASS_IDS + hashed_ids(np.random.default_rng(13), 40)
    values = SPECIAL + [float(i % 5) - 2.0 for i in range(len(ids) - len(SPECIAL))]
    model = as_model(kind, ids, values)
    with table_of(kind, model) as tab:
        _, vals, _ = check(tab, kind, model, divisor, what=(divisor, kind))
        assert len(vals) == len(ids)
        if divisor == 1.0:
            assert sorted(fbits(vals)) == sorted(fbits(values))  # x / 1.0 is x: the NaNs keep their signs too


# ---- 4. NULL outputs, capacity, refusals ----------------------------------------------------------------------------------------------
def poisoned(n):
    ids = np.zeros(n, dtype=_lib.U128)
    ids["lo"] = ids["hi"] = POISON
    return ids, np.full(n, POISON, dtype=np.uint64).view(np.float64), np.full(n, POISON, dtype=np.uint64)


def is_poison(*arrays):
    return all(bool((np.frombuffer(a.tobytes(), dtype=np.uint64) == POISON).all()) for a in arrays)


def small_table():
    rng = np.random.default_rng(14)
    ids = hashed_ids(rng, 70)
    model = as_model(KAHAN, ids, rng.integers(0, 4, 70).astype(np.float64), rng)
    return model, table_of(KAHAN, model)


def test_every_combination_of_null_outputs():
    model, tab = small_table()
    with tab:
        lib, n = tab.lib, len(model)
        full_ids, full_vals, full_ranks = check(tab, KAHAN, model, 3.0, ks=[n])
        top_ids, top_vals = tab.top_centralities(9, 3.0)
        for mask in range(8):
            ids, vals, ranks = poisoned(n + 1)
            written = ctypes.c_uint64(99)
            rc = lib.hbu_finish_centralities(tab.h, 3.0, _lib._ptr(ids) if mask & 1 else None, _lib._ptr(vals) if mask & 2 else None,
                                             _lib._ptr(ranks) if mask & 4 else None, n + 1, ctypes.byref(written))
            assert rc == _lib.HB_OK and written.value == n, mask
            assert np.array_equal(ids[:n], full_ids) if mask & 1 else is_poison(ids), mask
            assert fbits(vals[:n]) == fbits(full_vals) if mask & 2 else is_poison(vals), mask
            assert np.array_equal(ranks[:n], full_ranks) if mask & 4 else is_poison(ranks), mask
            assert is_poison(ids[n:], vals[n:], ranks[n:]), mask  # nothing past len
        for mask in range(4):
            ids, vals, _ = poisoned(10)
            written = ctypes.c_uint64(99)
            rc = lib.hbu_top_centralities(tab.h, 3.0, 9, _lib._ptr(ids) if mask & 1 else None, _lib._ptr(vals) if mask & 2 else None, ctypes.byref(written))
            assert rc == _lib.HB_OK and written.value == 9, mask
            assert np.array_equal(ids[:9], top_ids) if mask & 1 else is_poison(ids), mask
            assert fbits(vals[:9]) == fbits(top_vals) if mask & 2 else is_poison(vals), mask
            assert is_poison(ids[9:], vals[9:]), mask
        # no capacity is needed where nothing is written; written may be NULL
        written = ctypes.c_uint64(99)
        assert lib.hbu_finish_centralities(tab.h, 3.0, None, None, None, 0, ctypes.byref(written)) == _lib.HB_OK and written.value == n
        assert lib.hbu_finish_centralities(tab.h, 3.0, None, None, None, 0, None) == _lib.HB_OK
        assert lib.hbu_top_centralities(tab.h, 3.0, 0, None, None, ctypes.byref(written)) == _lib.HB_OK and written.value == 0
        assert_table(tab, KAHAN, model, list(model), "after the NULL combinations")


def test_capacity_below_len_writes_nothing():
    model, tab = small_table()
    with tab:
        n = len(model)
        for mask in range(1, 8):
            ids, vals, ranks = poisoned(n)
            written = ctypes.c_uint64(99)
            rc = tab.lib.hbu_finish_centralities(tab.h, 1.0, _lib._ptr(ids) if mask & 1 else None, _lib._ptr(vals) if mask & 2 else None,
                                                 _lib._ptr(ranks) if mask & 4 else None, n - 1, ctypes.byref(written))
            assert rc == _lib.HB_ERR_INVALID and written.value == 0, mask
            assert b"capacity" in tab.lib.hbu_last_error(tab.h)
            assert is_poison(ids, vals, ranks), mask
        check(tab, KAHAN, model, 1.0, ks=[1])


def test_refusals_leave_the_table_as_it_was(tmp_path):
    """a NULL table, every other kind (HLL64, U64, F32, DIST64), an empty output: HB_ERR_INVALID with a message, nothing written"""
    lib = _lib.load()
    ids, vals, ranks = poisoned(4)
    written = ctypes.c_uint64(99)
    err = ctypes.create_string_buffer(256)
    assert lib.hbu_finish_centralities(None, 1.0, _lib._ptr(ids), _lib._ptr(vals), _lib._ptr(ranks), 4, ctypes.byref(written)) == _lib.HB_ERR_INVALID
    assert written.value == 0 and lib.hbu_last_error(None)
    assert lib.hbu_top_centralities(None, 1.0, 2, _lib._ptr(ids), _lib._ptr(vals), ctypes.byref(written)) == _lib.HB_ERR_INVALID and written.value == 0
    assert lib.hbu_store_centralities(None, 1.0, os.fsencode(str(tmp_path / "null")), err, len(err)) == _lib.HB_ERR_INVALID and err.value
    assert not os.path.exists(tmp_path / "null")
    keys = u128([5, 9 | (1 << 64), 11])

    def refused(tab, name):
        written = ctypes.c_uint64(99)
        assert lib.hbu_finish_centralities(tab.h, 1.0, _lib._ptr(ids), _lib._ptr(vals), _lib._ptr(ranks), 4, ctypes.byref(written)) == _lib.HB_ERR_INVALID, name
        assert written.value == 0 and b"KahanSum or an f64" in lib.hbu_last_error(tab.h), name
        assert lib.hbu_top_centralities(tab.h, 1.0, 2, _lib._ptr(ids), _lib._ptr(vals), ctypes.byref(written)) == _lib.HB_ERR_INVALID and written.value == 0, name
        out = tmp_path / ("refused_" + name)
        assert lib.hbu_store_centralities(tab.h, 1.0, os.fsencode(str(out)), err, len(err)) == _lib.HB_ERR_INVALID and b"KahanSum" in err.value, name
        assert not os.path.exists(out) and is_poison(ids, vals, ranks), name
        with pytest.raises(_lib.HyperballError):
            ampc.finish_centralities(tab)

    for kind, model in ((ampc.KIND_U64, {5: 7, 9 | (1 << 64): 1, 11: 0}), (ampc.KIND_F32, {5: np.float32(1.5), 9 | (1 << 64): np.float32(2.0), 11: np.float32(0.5)})):
        with table_of(kind, model) as tab:
            refused(tab, "kind%d" % kind)
            assert_table(tab, kind, model, [5, 9 | (1 << 64), 11, 12], kind)
    with ampc.CounterTable() as tab:
        counters = np.arange(3 * 64, dtype=np.uint8).reshape(3, 64) % 50
        tab.batch_set(keys, counters)
        refused(tab, "hll64")
        got, found = tab.batch_get(keys)
        assert found.all() and np.array_equal(got, counters)
    with ampc.LaneTable() as tab:
        rows = np.arange(3 * 64, dtype=np.uint8).reshape(3, 64)
        tab.batch_set(keys, rows)
        refused(tab, "dist64")
        got, found = tab.batch_get(keys)
        assert found.all() and np.array_equal(got, rows)
    model, tab = small_table()
    with tab:
        for output in (None, b""):
            assert lib.hbu_store_centralities(tab.h, 1.0, output, err, len(err)) == _lib.HB_ERR_INVALID and b"output is empty" in err.value
        assert lib.hbu_store_centralities(tab.h, 1.0, b"", None, 0) == _lib.HB_ERR_INVALID
        assert_table(tab, KAHAN, model, list(model), "after the refusals")


# ---- 5. the store -------------------------------------------------------------------------------------------------------------------
def store_files(out):
    """{(database, file kind): sha256}: a segment's files by their extension (its name is a fresh uuid), meta.json with that name taken out"""
    found = {}
    for db in sorted(os.listdir(out)):
        names = sorted(os.listdir(os.path.join(out, db)))
        stems = {os.path.splitext(f)[0] for f in names if f != "meta.json"}
        assert len(stems) <= 1, names
        for f in names:
            data = open(os.path.join(out, db, f), "rb").read()
            if f == "meta.json":
                for s in stems:
                    data = data.replace(s.encode(), b"<segment>")
            key = (db, f if f == "meta.json" else os.path.splitext(f)[1])
            assert key not in found
            found[key] = hashlib.sha256(data).hexdigest()
    return found


def assert_same_store(tab, divisor, tmp_path, ids, vals, ranks):
    dev, host = tmp_path / "dev", tmp_path / "host"
    tab.store_centralities(str(dev), divisor)
    _lib.store_harmonic(str(host), ids, vals, ranks)
    a, b = store_files(dev), store_files(host)
    assert sorted({db for db, _ in a}) == ["harmonic", "harmonic_rank"]
    assert a == b, sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k))
    if len(ids):
        assert sorted(ext for db, ext in a if db == "harmonic") == [".bid", ".blm", ".blobs", ".ids", "meta.json"]
    return dev


@pytest.mark.parametrize("n", [0, 1, 257, 20_000])
def test_store_equals_the_host_route_and_reads_back(n, tmp_path):
    """the files of store_centralities have the SHA-256 of hb_store_harmonic's from the arrays finish_centralities returns, file by file;
    every key read back gives the value and the rank (all of them through the blob files, up to 300 also through bloom filter and fst)"""
    rng = np.random.default_rng(200 + n)
    ids = (CLASS_IDS + hashed_ids(rng, max(n - len(CLASS_IDS), 0)))[:n]
    values = rng.integers(0, 97, n).astype(np.float64)
    values[:min(n, 6)] = [INF, -1.0, -0.0, POS_NAN, TINY, -INF][:min(n, 6)]
    model = as_model(KAHAN, ids, values, rng)
    with table_of(KAHAN, model) as tab:
        got_ids, vals, ranks = (check(tab, KAHAN, model, 2657.0, ks=[1, n]) if n <= 257 else tab.finish_centralities(2657.0))
        out = assert_same_store(tab, 2657.0, tmp_path, got_ids, vals, ranks)
        want_v = dict(zip(ints(got_ids), fbits(vals)))
        want_r = dict(zip(ints(got_ids), ranks.tolist()))
        assert sorted(want_r.values()) == list(range(n))
        hdb, rdb = kv.Db(str(out / "harmonic"), "f64", str(tmp_path)), kv.Db(str(out / "harmonic_rank"), "u64", str(tmp_path))
        assert len(hdb) == len(rdb) == n
        assert {k: fbits([v])[0] for k, v in hdb.items()} == want_v
        assert dict(rdb.items()) == want_r
        for k in ints(got_ids)[::max(n // 300, 1)]:
            assert fbits([hdb.get(k)])[0] == want_v[k] and rdb.get(k) == want_r[k]
        if n:
            with pytest.raises(_lib.HyperballError) as e:
                tab.store_centralities(str(out), 2657.0)  # the directory holds databases now: refused like the host entry point
            assert e.value.code == _lib.HB_ERR_INVALID and "already lists segments" in str(e.value)
        assert_table(tab, KAHAN, model, list(model)[:500] + [2, (1 << 120) | 9], "after the store")


def test_store_that_cannot_be_written_leaves_nothing_and_can_be_retried(tmp_path):
    """the second database cannot get its meta.json: HB_ERR_IO, no segment file and no meta.json of the first one stays, and the same call
    succeeds once the obstacle is gone (tests/test_store.py has the writer's own form of this)"""
    model, tab = small_table()
    with tab:
        out = tmp_path / "centrality"
        (out / "harmonic_rank" / "meta.json").mkdir(parents=True)
        with pytest.raises(_lib.HyperballError) as e:
            tab.store_centralities(str(out), 3.0)
        assert e.value.code == _lib.HB_ERR_IO
        assert os.listdir(out / "harmonic") == [] and os.listdir(out / "harmonic_rank") == ["meta.json"]
        blocker = tmp_path / "file"
        blocker.write_text("x")
        with pytest.raises(_lib.HyperballError) as e:
            tab.store_centralities(str(blocker / "sub"), 3.0)
        assert e.value.code == _lib.HB_ERR_IO and blocker.read_text() == "x"
        os.rmdir(out / "harmonic_rank" / "meta.json")
        tab.store_centralities(str(out), 3.0)
        ids, vals, ranks = check(tab, KAHAN, model, 3.0, ks=[1])
        _lib.store_harmonic(str(tmp_path / "host"), ids, vals, ranks)
        assert store_files(out) == store_files(tmp_path / "host")


# ---- 6. the drivers -------------------------------------------------------------------------------------------------------------------
def job_graph(which):
    edges = dict(harmonic_graphs())[which]
    if which == "rmat":
        edges = edges[:600]
    sink = (1 << 90) | 5
    edges = edges + [(edges[0][0], sink), (edges[-1][0], sink)]
    nodes = sorted({x for e in edges for x in e})
    return edges, nodes, sink


def assert_store_is(out, result, tmp_path):
    """the two databases under `out` read back as the dictionary a driver returned, bit for bit, with the model's ranks"""
    ids = sorted(result)
    vals = [result[k] for k in ids]
    hdb, rdb = kv.Db(str(out / "harmonic"), "f64", str(tmp_path)), kv.Db(str(out / "harmonic_rank"), "u64", str(tmp_path))
    stored = dict(hdb.items())
    assert sorted(stored) == ids and len(hdb) == len(ids)
    assert fbits([stored[k] for k in ids]) == fbits(vals)
    assert dict(rdb.items()) == dict(zip(ids, fref.ranks_of(ids, [stored[k] for k in ids])))
    assert hdb.get(ids[0]) is not None and rdb.get(ids[-1]) is not None and hdb.get((1 << 101) | 1) is None


@pytest.mark.parametrize("which", ["rmat", "fixture"])
def test_run_harmonic_job_with_output(which, tmp_path):
    edges, nodes, _ = job_graph(which)
    gs = [graph_of(n, e, 700) for n, e in two_workers(edges, nodes)]
    try:
        plain = ampc.run_harmonic_job(gs)
        stored = ampc.run_harmonic_job(gs, output=str(tmp_path / "out"))
    finally:
        for g in gs:
            g.close()
    assert len(plain) >= 2 and plain.keys() == stored.keys()
    assert [fref.bits(plain[k]) for k in plain] == [fref.bits(stored[k]) for k in plain]
    assert_store_is(tmp_path / "out", stored, tmp_path)


@pytest.mark.parametrize("sources_per_walk", [1, 64])
@pytest.mark.parametrize("which", ["rmat", "fixture"])
def test_run_approx_harmonic_job_with_output(which, sources_per_walk, tmp_path):
    """sources that include a node without out-links and one source twice: the sampled sources end up inf or NaN, and are stored so"""
    edges, nodes, sink = job_graph(which)
    with_out = {f for f, _ in edges}
    busy = [n for n in nodes if n in with_out][:3]
    sources = [busy[0], sink, busy[1], busy[0], busy[2]]
    gs = [graph_of(n, e, 700) for n, e in two_workers(edges, nodes)]
    try:
        plain = ampc.run_approx_harmonic_job(gs, sources, 9, 4, sources_per_walk=sources_per_walk)
        stored = ampc.run_approx_harmonic_job(gs, sources, 9, 4, sources_per_walk=sources_per_walk, output=str(tmp_path / "out"))
    finally:
        for g in gs:
            g.close()
    assert len(plain) >= 2 and plain.keys() == stored.keys() and not math.isfinite(plain[sink])
    assert fbits([plain[k] for k in plain]) == fbits([stored[k] for k in plain])
    assert_store_is(tmp_path / "out", stored, tmp_path)
