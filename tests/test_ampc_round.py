"""The resident worker of the AMPC shard (include/hb_ampc.h: hbu_graph, hbu_filter, hbu_setup_counters, hbu_round_counters,
hbu_round_distances, hbu_round_centralities; kernels in stract_amd/csrc/hb_ampc_round.hip.h; drivers in stract_amd/ampc.py) against
tests/ampc_round_ref.py and against the route a worker had to take before: the filter in host code, hbu_update_counters on the selected
edges, the filter update in host code.  Every comparison is exact: bit-vector words, id sets, registers, distances, counts."""
import collections
import ctypes

import numpy as np
import pytest

from stract_amd import _lib, ampc
from tests import ampc_ref as ref
from tests import ampc_round_ref as rref
from tests import graphs
from tests.test_ampc_edges import counter_table, distance_table, split
from tests.test_ampc_values import assert_counters, assert_table, dev_values, harmonic_graphs, key_int, u128

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
U64, KAHAN = ampc.KIND_U64, ampc.KIND_KAHAN
PRIME_INV = pow(rref.LARGE_PRIME, -1, 1 << 64)


def interpreted():
    return hasattr(_lib.load(), "hb_simt_interpreter")


def id_with_slot(slot, num_bits, k=0):
    """a low half whose product with the prime is slot + k * num_bits: its bit is `slot`"""
    return ((slot + k * num_bits) * PRIME_INV) & M64


def graph_of(nodes, edges, chunk=0):
    f, t = split(edges)
    return ampc.WorkerGraph(u128(nodes), f, t, chunk_edges=chunk)


def device_filter(model):
    """a device filter with the content of a model filter (rref.Bloom / rref.Exact)"""
    if model.kind == "sketch":
        f = ampc.ChangedFilter.bloom(model.num_bits)
        f.import_bits(model.words())
    else:
        f = ampc.ChangedFilter.exact()
        f.insert(u128(sorted(model.ids)))
    return f


def assert_filter(dev, model, probe, what=""):
    """count, contains of every probe id, and the whole content: the words of a bloom filter, the ids of an exact set"""
    assert dev.count() == model.count(), what
    assert dev.contains(u128(probe)).tolist() == [model.contains(k) for k in probe], what
    if model.kind == "sketch":
        assert dev.kind == ampc.FILTER_BLOOM and dev.num_bits == model.num_bits, what
        assert np.array_equal(dev.export_bits(), model.words()), what
    else:
        assert dev.kind == ampc.FILTER_EXACT, what
        ids = [key_int(k) for k in dev.export_ids()]
        assert len(ids) == len(set(ids)) and set(ids) == model.ids, what


# ---- 1. the filter ----------------------------------------------------------------------------------------------------------------
def test_bloom_known_answer_of_the_reference():
    """crates/bloom/src/lib.rs:198-216: U64BloomFilter::new(100, 0.01), insert 1..5: contains 1..5 and none of 6..10"""
    nb = ampc.bloom_num_bits(100, 0.01)
    assert nb == rref.bloom_num_bits(100, 0.01) == 120
    with ampc.ChangedFilter.bloom(nb) as f:
        f.insert(u128([1, 2, 3, 4, 5]))
        assert f.contains(u128(list(range(1, 11)))).tolist() == [True] * 5 + [False] * 5
        assert f.count() == 5


@pytest.mark.parametrize("items,fp", [(100, 0.01), (1, 0.05), (10 ** 8, 0.05), (3 * 10 ** 8, 0.01)])
def test_bloom_num_bits(items, fp):
    assert ampc.bloom_num_bits(items, fp) == rref.bloom_num_bits(items, fp) > 0


@pytest.mark.parametrize("num_bits", [1, 63, 64, 65, 120, 4099])
def test_bloom_filter_against_the_model(num_bits):
    """Random ids with high halves, ids whose product with the prime exceeds 2^63 and 2^64 - 1 itself, ids whose slot is the first and the
    last bit, two ids with one low half: insert, contains, count, the exported words; fill (count == num_bits, the tail bits zero), clear;
    export -> import -> export is the identity."""
    rng = np.random.default_rng(num_bits)
    pool = [int(x) | (int(y) << 64) for x, y in zip(rng.integers(0, 1 << 63, 300), rng.integers(0, 1 << 20, 300))]
    pool += [M64, M64 - 1, 1 << 63, (1 << 63) + 12345, 0, 3]
    pool += [id_with_slot(num_bits - 1, num_bits, k) | (k << 64) for k in (0, 1, 5)] + [id_with_slot(0, num_bits, 2)]
    assert all(rref.bloom_slot(k, num_bits) == num_bits - 1 for k in pool[-4:-1]) and rref.bloom_slot(pool[-1], num_bits) == 0
    assert any(((k & M64) * rref.LARGE_PRIME) & M64 >= 1 << 63 for k in pool)
    twin = (pool[0] & M64) | (77 << 64)
    model = rref.Bloom(num_bits)
    with ampc.ChangedFilter.bloom(num_bits) as f, ampc.ChangedFilter.bloom(num_bits) as g:
        assert_filter(f, model, pool, "empty")
        put = pool[0:300:7] + pool[300:303] + [pool[-2]]
        f.insert(u128(put))
        for k in put:
            model.insert(k)
        assert model.contains(twin) and model.contains(pool[-3]) and model.contains(pool[-4])
        assert_filter(f, model, pool + [twin], "inserted")
        words = f.export_bits()
        g.import_bits(words)
        assert np.array_equal(g.export_bits(), words)
        assert_filter(g, model, pool, "imported")
        f.fill()
        model.fill()
        assert f.count() == num_bits
        assert_filter(f, model, pool, "filled")
        if num_bits % 64:
            assert int(f.export_bits()[-1]) >> (num_bits % 64) == 0
        f.clear()
        assert_filter(f, rref.Bloom(num_bits), pool, "cleared")


def test_bloom_filter_of_the_largest_size():
    """num_bits = 2^32 - 1: a handful of ids, among them the first and the last bit; contains and count only"""
    if interpreted():
        pytest.skip("512 MB of bits word by word: the device only")
    nb = (1 << 32) - 1
    ids = [1, M64, id_with_slot(nb - 1, nb, 3), id_with_slot(0, nb, 1), (1 << 63) | 99, 5 | (9 << 64)]
    probe = ids + [2, 6, 7, id_with_slot(nb - 2, nb), 5 | (1 << 64)]
    model = rref.Bloom(nb)
    with ampc.ChangedFilter.bloom(nb) as f:
        f.insert(u128(ids))
        for k in ids:
            model.insert(k)
        assert {rref.bloom_slot(k, nb) for k in ids} >= {0, nb - 1}
        assert f.contains(u128(probe)).tolist() == [model.contains(k) for k in probe]
        assert f.count() == model.count() == len(ids)


def test_ids_with_one_low_half():
    """Two ids with equal low halves and different high halves: one bit of a bloom filter, two members of an exact set"""
    a, b, c = 12345 | (1 << 64), 12345 | (2 << 64), 12345 | (3 << 64)
    with ampc.ChangedFilter.bloom(4099) as f, ampc.ChangedFilter.exact() as e:
        f.insert(u128([a, b]))
        e.insert(u128([a, b]))
        assert f.count() == 1 and f.contains(u128([a, b, c])).tolist() == [True, True, True]
        assert e.count() == 2 and e.contains(u128([a, b, c, 12345])).tolist() == [True, True, False, False]


def test_import_with_a_tail_bit_is_refused():
    with ampc.ChangedFilter.bloom(70) as f:
        f.insert(u128([1, 2, 3]))
        before = f.export_bits()
        lib = f.lib
        bad = np.array([5, 1 << 6], dtype=np.uint64)  # bit 70
        assert lib.hbu_filter_import_bits(f.h, _lib._ptr(bad)) == _lib.HB_ERR_INVALID
        assert lib.hbu_last_error(None)
        assert np.array_equal(f.export_bits(), before)
        good = np.array([5, 1 << 5], dtype=np.uint64)  # bit 69, the last one
        f.import_bits(good)
        assert np.array_equal(f.export_bits(), good) and f.count() == 3
        with ampc.ChangedFilter.bloom(64) as g:  # no tail
            g.import_bits(np.array([M64], dtype=np.uint64))
            assert g.count() == 64


def test_union():
    """blooms of one size: a word-wise OR (the destination keeps its own bits); unequal sizes or kinds: refused, both unchanged"""
    rng = np.random.default_rng(9)
    ids = [int(x) for x in rng.integers(1, 1 << 62, 120)]
    ma, mb = rref.Bloom(1000), rref.Bloom(1000)
    with ampc.ChangedFilter.bloom(1000) as a, ampc.ChangedFilter.bloom(1000) as b, ampc.ChangedFilter.bloom(1001) as c, ampc.ChangedFilter.exact() as e, \
            ampc.ChangedFilter.exact() as e2:
        a.insert(u128(ids[:60]))
        b.insert(u128(ids[40:]))
        for k in ids[:60]:
            ma.insert(k)
        for k in ids[40:]:
            mb.insert(k)
        assert ma.ones - mb.ones and mb.ones - ma.ones
        a.union(b)
        ma.union(mb)
        assert_filter(a, ma, ids, "a |= b")
        assert_filter(b, mb, ids, "b")
        e.insert(u128(ids[:10]))
        for dst, src in ((a, c), (c, a), (a, e), (e, a)):
            assert a.lib.hbu_filter_union(dst.h, src.h) == _lib.HB_ERR_INVALID
            assert a.lib.hbu_last_error(None)
        assert a.lib.hbu_filter_union(a.h, None) == _lib.HB_ERR_INVALID
        assert_filter(a, ma, ids, "a after refusals")
        assert c.count() == 0 and e.count() == 10
        e2.insert(u128(ids[5:30]))
        e.union(e2)
        assert_filter(e, rref.Exact(ids[:30]), ids, "exact union")
        assert_filter(e2, rref.Exact(ids[5:30]), ids, "exact source")
        for f, call in ((e, "hbu_filter_fill"), (e, "hbu_filter_export_bits"), (a, "hbu_filter_export_ids")):  # calls of the other kind
            args = {"hbu_filter_fill": (f.h,), "hbu_filter_export_bits": (f.h, _lib._ptr(np.zeros(16, np.uint64))),
                    "hbu_filter_export_ids": (f.h, _lib._ptr(np.zeros(4, _lib.U128)), 4, ctypes.byref(ctypes.c_uint64(0)))}[call]
            assert getattr(a.lib, call)(*args) == _lib.HB_ERR_INVALID, call


def test_filter_create_limits():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.hbu_filter_create(-1, ampc.FILTER_BLOOM, 0, ctypes.byref(h)) == _lib.HB_ERR_INVALID and not h
    assert lib.hbu_filter_create(-1, ampc.FILTER_BLOOM, 1 << 32, ctypes.byref(h)) == _lib.HB_ERR_LIMIT and not h
    assert lib.hbu_filter_create(-1, 7, 64, ctypes.byref(h)) == _lib.HB_ERR_INVALID and not h
    assert lib.hbu_last_error(None)


@pytest.mark.parametrize("count", [0, 1, 16384, 16385])
def test_exact_set(count):
    """0, 1, 16 384 and 16 385 distinct ids with duplicates among them, inserted in two calls (the index grows): count, contains,
    export_ids as a set; clear empties it and it can be filled again"""
    ids = [((i * 2654435761) & M64) | ((i % 3) << 64) for i in range(1, count + 1)]
    assert len(set(ids)) == count
    batch = ids + ids[: count // 3]
    model = rref.Exact(ids)
    others = [k ^ (1 << 70) for k in ids[:50]] + [0, 1 << 100]
    with ampc.ChangedFilter.exact() as f:
        half = len(batch) // 2
        f.insert(u128(batch[:half]))
        f.insert(u128(batch[half:]))
        probe = ids[:100] + ids[-100:] + others
        assert_filter(f, model, probe, count)
        f.clear()
        assert_filter(f, rref.Exact(), probe, "cleared")
        f.insert(u128(others))
        assert_filter(f, rref.Exact(others), probe, "again")


# ---- 2. round_counters -----------------------------------------------------------------------------------------------------------
NUM_BITS = 4099


def counters_case():
    """~3 500 edges for chunk_edges = 1000 over ~300 keys and a bloom filter of 4099 bits: chunk 0 selects everything, chunk 1 nothing,
    chunk 2 exactly one edge, chunk 3 (500 edges) some; the hub destination has selected edges in chunks 0, 2 and 3 (its group spans
    chunk boundaries).  Crafted: an Inserted destination, a bloom false positive that answers NoChange, a changed source absent from prev."""
    rng = np.random.default_rng(2024)
    pool = [int(x) | (int(y) << 64) for x, y in zip(rng.integers(1, 1 << 62, 300), rng.integers(0, 4, 300))]
    changed_src, rest = pool[:120], pool[120:]
    filt = rref.Bloom(NUM_BITS)
    for k in changed_src:
        filt.insert(k)
    quiet = [k for k in rest if not filt.contains(k)]  # sources the filter really rejects
    assert len(quiet) > 100
    fp = id_with_slot(rref.bloom_slot(changed_src[0], NUM_BITS), NUM_BITS, 7) | (5 << 64)  # shares a bit with a changed source
    assert fp not in changed_src and filt.contains(fp)
    absent_src = changed_src[1]  # in the filter, not in prev
    m_prev = {k: r for k, r in zip(pool[:250], graphs.random_registers(rng, 250)) if k != absent_src}
    m_prev[fp] = graphs.random_registers(rng, 1)[0]
    m_next = ref.clone_table(m_prev)
    hub, fresh, fp_dest, absent_dest = pool[260], (8 << 64) | 1, pool[261], pool[262]
    m_next[hub] = np.zeros(64, np.uint8)
    m_next[absent_dest] = np.zeros(64, np.uint8)
    settled = m_prev[fp].copy()
    ref.hbo.hll_add(settled, fp)
    m_next[fp_dest] = settled  # already holds everything the false positive brings
    dests = pool[200:260]
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    edges = [(pick(changed_src), hub if i % 10 == 0 else pick(dests)) for i in range(1000)]       # chunk 0: everything
    edges += [(pick(quiet), hub if i % 10 == 0 else pick(dests)) for i in range(1000)]             # chunk 1: nothing
    third = [(pick(quiet), pick(dests)) for i in range(1000)]                                      # chunk 2: exactly one
    third[617] = (changed_src[5], hub)
    edges += third
    last = [(pick(changed_src) if i % 3 == 0 else pick(quiet), hub if i % 7 == 0 else pick(dests)) for i in range(500)]
    last[10], last[20], last[30] = (changed_src[7], fresh), (fp, fp_dest), (absent_src, absent_dest)
    edges += last
    for lo, want in ((0, 1000), (1000, 0), (2000, 1)):
        assert sum(filt.contains(f) for f, _ in edges[lo:lo + 1000]) == want
    assert 1 < sum(filt.contains(f) for f, _ in edges[3000:]) < 500
    space = sorted(set(pool) | {fp, fresh})
    return dict(edges=edges, filt=filt, m_prev=m_prev, m_next=m_next, space=space, fresh=fresh, fp=fp, fp_dest=fp_dest, absent_src=absent_src,
                absent_dest=absent_dest, hub=hub, nodes=pool[:50])


@pytest.fixture(scope="module")
def counters_expected():
    case = counters_case()
    m_prev, m_next = ref.clone_table(case["m_prev"]), ref.clone_table(case["m_next"])
    new = rref.Bloom(NUM_BITS)
    counts = rref.round_counters(m_prev, m_next, case["edges"], case["filt"], new)
    case.update(want_prev=m_prev, want_next=m_next, want_new=new, want_counts=counts)
    return case


def test_round_counters_case_pins_what_it_should(counters_expected):
    c = counters_expected
    picked = [e for e in c["edges"] if c["filt"].contains(e[0])]
    keys, actions = ref.update_counters(ref.clone_table(c["m_prev"]), ref.clone_table(c["m_next"]), picked)
    by_edge = dict(zip(picked, actions))  # (these crafted edges occur once)
    assert actions[[k for k in keys].index(c["fresh"])] == ref.INSERTED and keys.count(c["fresh"]) == 1
    assert not c["want_new"].contains(c["fresh"]) and c["fresh"] in c["want_next"]
    assert by_edge[(c["fp"], c["fp_dest"])] == ref.NO_CHANGE
    assert by_edge[(c["absent_src"], c["absent_dest"])] == ref.MERGED
    assert np.array_equal(c["want_next"][c["absent_dest"]], ref.hll_of(c["absent_src"]))
    assert set(actions) == {ref.NO_CHANGE, ref.MERGED, ref.INSERTED} and c["want_counts"][2] >= 1
    assert c["want_new"].count() > 5


@pytest.mark.parametrize("route", ["chunks_of_1000", "default_chunk", "composed", "without_new_changed"])
def test_round_counters(counters_expected, route):
    """hbu_round_counters with chunk_edges = 1000 and with the default, and the composed route of the calls that existed before (the model's
    contains on the host, hbu_update_counters on the selected edges as ONE batch, the model's insert of the Merged destinations): tables,
    the words of new_changed and the three counts equal the model's; new_changed = NULL changes none of the rest."""
    c = counters_expected
    with counter_table(c["m_prev"]) as prev, counter_table(c["m_next"]) as nxt, device_filter(c["filt"]) as changed, ampc.ChangedFilter.bloom(NUM_BITS) as new:
        if route == "composed":
            picked = [e for e in c["edges"] if c["filt"].contains(e[0])]
            actions = ampc.update_counters(prev, nxt, *split(picked))
            merged = [t for (_, t), a in zip(picked, actions) if a == ampc.MERGED]
            new.insert(u128(merged))
            counts = (len(picked), len(merged), int((actions == ampc.INSERTED).sum()))
        else:
            with graph_of(c["nodes"], c["edges"], 1000 if route == "chunks_of_1000" else 0) as g:
                assert len(g) == len(c["edges"])
                counts = ampc.round_counters(prev, nxt, g, changed, None if route == "without_new_changed" else new)
        assert counts == c["want_counts"]
        assert_counters(nxt, c["want_next"], c["space"], route)
        assert_counters(prev, c["want_prev"], c["space"], route)
        assert_filter(changed, c["filt"], c["space"], route)
        assert_filter(new, rref.Bloom(NUM_BITS) if route == "without_new_changed" else c["want_new"], c["space"], route)


def test_round_counters_with_an_exact_filter():
    """the same step with exact sets on both sides: chunk boundaries inside the destinations' groups, new_changed grows from empty"""
    rng = np.random.default_rng(31)
    pool = [int(x) for x in rng.integers(1, 1 << 62, 200)]
    edges = [(pool[int(a)], pool[int(b)]) for a, b in zip(rng.integers(0, 200, 700), rng.integers(100, 130, 700))]
    m_prev = {k: r for k, r in zip(pool, graphs.random_registers(rng, 200))}
    m_next = ref.clone_table(m_prev)
    filt, new = rref.Exact(pool[:60]), rref.Exact()
    want = rref.round_counters(m_prev, m_next, edges, filt, new)
    assert new.count() > 3
    with counter_table(m_prev) as prev, counter_table(m_prev) as nxt, device_filter(filt) as changed, ampc.ChangedFilter.exact() as d_new, \
            graph_of(pool, edges, 64) as g:
        assert ampc.round_counters(prev, nxt, g, changed, d_new) == want
        assert_counters(nxt, m_next, pool, "next")
        assert_filter(d_new, new, pool, "new_changed")


# ---- 3. round_distances ----------------------------------------------------------------------------------------------------------
def distances_case():
    """The shape of counters_case for the distance step: chunks of 1000 that select everything, nothing, one edge and some; sources with
    and without a distance; a destination reached only by selected sources without a distance; an Inserted destination; destinations
    with exactly 32, 33, 64 and 65 candidates inside one chunk (either side of the fold's switch to a wave, and of a wave's width)."""
    rng = np.random.default_rng(77)
    pool = [int(x) | (int(y) << 64) for x, y in zip(rng.integers(1, 1 << 62, 300), rng.integers(0, 4, 300))]
    changed_src = pool[:120]
    sketch = rref.Bloom(NUM_BITS)
    for k in changed_src:
        sketch.insert(k)
    quiet_pool = [k for k in pool[120:200] if not sketch.contains(k)]  # rejected by the exact set and by the bloom filter alike
    assert len(quiet_pool) > 60
    m_prev = {k: int(rng.integers(1, 40)) for k in changed_src[:90]}  # changed_src[90:]: selected, but without a distance
    m_prev.update({k: int(rng.integers(1, 40)) for k in quiet_pool[:40]})
    lost = changed_src[90:]
    dests = pool[200:260]
    m_next = dict(m_prev)
    m_next.update({k: int(rng.integers(1, 60)) for k in dests[:40]})  # dests[40:]: absent, Inserted when reached
    hub, only_lost, fresh = pool[260], pool[261], pool[262]
    lengths = {pool[270]: 32, pool[271]: 33, pool[272]: 64, pool[273]: 65}
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    first = [(pick(changed_src), hub if i % 10 == 0 else pick(dests)) for i in range(1000)]
    at = 100
    for d, n in lengths.items():  # exactly n candidates each, all in chunk 0, interleaved with skipped edges
        for j in range(n):
            first[at] = (changed_src[j % 90], d)
            first[at + 1] = (pick(lost), d)
            at += 2
    first[900], first[901] = (lost[0], only_lost), (lost[1], only_lost)
    first[902] = (changed_src[3], fresh)
    third = [(pick(quiet_pool), pick(dests)) for i in range(1000)]
    third[333] = (changed_src[5], hub)
    last = [(pick(changed_src) if i % 3 == 0 else pick(quiet_pool), hub if i % 7 == 0 else pick(dests)) for i in range(500)]
    edges = first + [(pick(quiet_pool), hub if i % 10 == 0 else pick(dests)) for i in range(1000)] + third + last
    for d, n in lengths.items():
        assert sum(1 for f, t in edges if t == d and f in m_prev) == n
    space = sorted(set(pool))
    return dict(edges=edges, changed_src=changed_src, m_prev=m_prev, m_next=m_next, space=space, only_lost=only_lost, fresh=fresh, nodes=pool[:20])


@pytest.mark.parametrize("kind", ["bloom", "exact"])
def test_round_distances(kind):
    """hbu_round_distances with chunk_edges = 1000 against the model (a batch per chunk): next, new_changed and both counts; then the
    same round again on the result: nothing changes and changed_nodes == 0."""
    c = distances_case()
    if kind == "bloom":
        filt, new = rref.Bloom(NUM_BITS), rref.Bloom(NUM_BITS)
        for k in c["changed_src"]:
            filt.insert(k)
    else:
        filt, new = rref.Exact(c["changed_src"]), rref.Exact()
    assert [sum(filt.contains(f) for f, _ in c["edges"][lo:lo + 1000]) for lo in (0, 1000, 2000)] == [1000, 0, 1]
    m_prev, m_next = dict(c["m_prev"]), dict(c["m_next"])
    want = rref.round_distances(m_prev, m_next, c["edges"], filt, new, 1000)
    assert c["only_lost"] not in m_next and (kind == "bloom" or not new.contains(c["only_lost"]))
    assert c["fresh"] in m_next and new.contains(c["fresh"]) and want[1] > 10
    with distance_table(c["m_prev"]) as prev, distance_table(c["m_next"]) as nxt, device_filter(filt) as changed, device_filter(rref.Bloom(NUM_BITS) if kind == "bloom" else rref.Exact()) as d_new, \
            graph_of(c["nodes"], c["edges"], 1000) as g:
        assert ampc.round_distances(prev, nxt, g, changed, d_new) == want
        assert_table(nxt, U64, m_next, c["space"], "next")
        assert_table(prev, U64, m_prev, c["space"], "prev")
        assert_filter(d_new, new, c["space"], "new_changed")
        # again: every candidate is at least what next holds now
        again = rref.round_distances(m_prev, m_next, c["edges"], filt, None, 1000)
        assert again == (want[0], 0)
        d_new.clear()
        assert ampc.round_distances(prev, nxt, g, changed, d_new) == again
        assert d_new.count() == 0
        assert_table(nxt, U64, m_next, c["space"], "next, again")
        assert ampc.round_distances(prev, nxt, g, changed, None) == again


# ---- 4. round_centralities and setup_counters --------------------------------------------------------------------------------------
def test_round_centralities():
    """Nodes in chunks of 16 through a bloom filter: a node listed twice, a node in one counter table only, a node that the filter rejects
    although its size grew (it stays unwritten), nodes whose size did not grow; two rounds with different divisors."""
    rng = np.random.default_rng(5)
    pool = [int(x) | (int(y) << 64) for x, y in zip(rng.integers(1, 1 << 62, 80), rng.integers(0, 3, 80))]
    filt = rref.Bloom(NUM_BITS)
    for k in pool[:50]:
        filt.insert(k)
    rejected = next(k for k in pool[50:] if not filt.contains(k))
    m_prev_c = {k: ref.hll_of(k) for k in pool[:70]}
    m_next_c = ref.clone_table(m_prev_c)
    for k in pool[:40] + [rejected]:  # these grow
        for other in rng.integers(1, 1 << 62, 30):
            ref.hbo.hll_add(m_next_c[k], int(other))
    only_next = pool[45]
    del m_prev_c[only_next]
    nodes = pool[:60] + [pool[3], rejected, pool[3]]
    m_prev_v = {pool[0]: (1.5, 0.25), pool[1]: (2.0, 0.0)}
    m_next_v = ref.clone_table(m_prev_v)
    with counter_table(m_prev_c) as prev_c, counter_table(m_next_c) as next_c, ampc.ValueTable(KAHAN) as prev_v, device_filter(filt) as changed, \
            graph_of(nodes, [], 16) as g, graph_of(nodes, [], 0) as g0:
        prev_v.batch_set(u128(list(m_prev_v)), dev_values(KAHAN, m_prev_v.values()))
        for round_, graph, chunk in ((0, g, 16), (6, g0, 0)):
            with prev_v.clone() as next_v:
                want_v = ref.clone_table(m_next_v)
                want = rref.round_centralities(m_prev_c, m_next_c, m_prev_v, want_v, nodes, filt, round_, chunk)
                assert rejected not in want_v and only_next not in want_v and pool[3] in want_v and 30 < len(want_v) < 60
                assert ampc.round_centralities(prev_c, next_c, prev_v, next_v, graph, changed, round_) == want
                assert_table(next_v, KAHAN, want_v, pool, round_)
                assert_table(prev_v, KAHAN, m_prev_v, pool, round_)


def test_setup_counters():
    """Both tables equal batch_set of HyperLogLog::default() + add(node) (the oracle's add), stored counters are overwritten, and the
    filter holds every node; nodes with one low half share a counter value; more nodes than one pass takes (chunk_edges = 100)."""
    rng = np.random.default_rng(6)
    nodes = [int(x) | (int(y) << 64) for x, y in zip(rng.integers(1, 1 << 62, 333), rng.integers(0, 3, 333))]
    nodes[7] = (nodes[8] & M64) | (9 << 64)
    m_prev = {nodes[0]: graphs.random_registers(rng, 1)[0], 424242: ref.hll_of(1)}
    m_next = {nodes[1]: graphs.random_registers(rng, 1)[0]}
    for filt in (rref.Bloom(NUM_BITS), rref.Exact(), None):
        want_prev, want_next = ref.clone_table(m_prev), ref.clone_table(m_next)
        rref.setup_counters(want_prev, want_next, nodes, filt)
        with counter_table(m_prev) as prev, counter_table(m_next) as nxt, graph_of(nodes, [(1, 2)], 100) as g:
            d_filt = device_filter(filt) if filt is not None else None
            try:
                ampc.setup_counters(prev, nxt, g, d_filt)
                assert_counters(prev, want_prev, nodes + [424242, 5], "prev")
                assert_counters(nxt, want_next, nodes + [424242, 5], "next")
                if d_filt is not None:
                    assert_filter(d_filt, filt, nodes + [424242, 5], "changed")
            finally:
                if d_filt is not None:
                    d_filt.close()


# ---- 5. whole jobs ---------------------------------------------------------------------------------------------------------------
def two_workers(edges, nodes):
    return [(nodes[w::2], edges[w::2]) for w in (0, 1)]


@pytest.mark.parametrize("which", ["rmat", "fixture"])
def test_run_harmonic_job(which):
    """run_harmonic_job with two workers (chunks of 700 edges) against the model's loop: after every round both counter tables, the new
    centrality table, every worker's filter and the counts; at the end the centralities."""
    edges = dict(harmonic_graphs())[which]
    nodes = sorted({x for e in edges for x in e})
    workers = two_workers(edges, nodes)
    model = rref.harmonic_job(workers)
    rounds = []

    def on_round(state):
        want = next(model)
        rounds.append(state["round"])
        assert state["counts"] == want["counts"] and state["written"] == want["written"] and state["had_changes"] == want["had_changes"], state["round"]
        assert_counters(state["prev_counters"], want["prev_counters"], nodes, state["round"])
        assert_counters(state["next_counters"], want["next_counters"], nodes, state["round"])
        assert_table(state["next_centrality"], KAHAN, want["next_centrality"], nodes, state["round"])
        for got, f in zip(state["filters"], want["filters"]):
            assert_filter(got, f, nodes[:200], state["round"])

    gs = [graph_of(n, e, 700) for n, e in workers]
    try:
        result = ampc.run_harmonic_job(gs, on_round=on_round)
    finally:
        for g in gs:
            g.close()
    with pytest.raises(StopIteration) as done:
        next(model)
    want = done.value.value
    assert rounds == list(range(len(rounds))) and len(rounds) >= 3 and len(want) > 0
    assert result.keys() == want.keys()
    assert all(np.float64(result[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64) for k in want)


def bfs(edges, source):
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
    return dist


def run_shortest_path(workers, source, nodes, chunk, max_distance=None):
    """the driver against the model's loop, round by round; returns (final model table, rounds, kinds of the filters seen)"""
    model = rref.shortest_path_job(workers, source, max_distance, chunk)
    kinds, rounds = set(), []

    def on_round(state):
        want = next(model)
        rounds.append(state["round"])
        assert state["counts"] == want["counts"] and state["had_changes"] == want["had_changes"], state["round"]
        assert_table(state["next"], U64, want["next"], nodes, state["round"])
        for got, f in list(zip(state["filters"], want["filters"])) + list(zip(state["saved"], want["saved"])):
            assert_filter(got, f.inner, nodes[:300], state["round"])
            kinds.add(f.inner.kind)

    gs = [graph_of(n, e, chunk) for n, e in workers]
    try:
        table = ampc.run_shortest_path_job(gs, source, max_distance, on_round=on_round)
    finally:
        for g in gs:
            g.close()
    with table:
        with pytest.raises(StopIteration) as done:
            next(model)
        want = done.value.value
        assert_table(table, U64, want, nodes, "final")
    return want, rounds, kinds


def test_run_shortest_path_job_small():
    """300 nodes, 5000 edges, two workers, chunks of 900: the sets stay exact; the final distances are those of a BFS; with max_distance
    the loop stops after that many rounds"""
    edges = graphs.lcg_graph(300, 5000)
    nodes = list(range(1, 301))
    workers = two_workers(edges, nodes)
    want, rounds, kinds = run_shortest_path(workers, 1, nodes + [777], 900)
    dist = bfs(edges, 1)
    assert want == dist and len(rounds) == max(dist.values()) + 1 and kinds == {"exact"}
    want, rounds, _ = run_shortest_path(workers, 1, nodes + [777], 900, max_distance=2)
    assert len(rounds) == 2 and want == {k: d for k, d in dist.items() if d <= 2}


def star(leaves, base, second=50):
    """source 1 -> `leaves` leaves -> a second level of `second` nodes (leaf i -> base + 10^6 + i % second)"""
    ls = [base + i for i in range(leaves)]
    return [(1, x) for x in ls] + [(x, base + 10 ** 6 + i % second) for i, x in enumerate(ls)]


def test_run_shortest_path_job_crosses_the_sketch_threshold():
    """One worker whose source has 17 000 leaves: the new set crosses 16 384 inside one round and becomes a sketch of ALL of its ids (add(),
    updated_nodes.rs:89-103): the second level is reached and the distances are those of a BFS."""
    edges = star(17_000, 1 << 40)
    nodes = sorted({x for e in edges for x in e})
    want, rounds, kinds = run_shortest_path([(nodes, edges)], 1, nodes[:400] + nodes[-100:], 6000)
    assert want == bfs(edges, 1) and kinds == {"exact", "sketch"} and max(want.values()) == 2


def test_run_shortest_path_job_restates_the_left_set_only_union():
    """Two workers with 9 000 and 8 000 leaves: each new set is exact, their union is over the threshold and the reference builds the
    sketch from the LEFT set only (updated_nodes.rs:48-58) - of the second worker's leaves (one second-level node each) only the sketch's
    false positives are relaxed.  The driver restates that: it equals the model, and the model differs from a BFS exactly there."""
    a, b = star(9_000, 1 << 40), star(8_000, 1 << 41, 8_000)
    nodes_a, nodes_b = sorted({x for e in a for x in e}), sorted({x for e in b for x in e})
    probe = nodes_a[:200] + nodes_a[-60:] + nodes_b[:200] + nodes_b[-400:]
    want, rounds, kinds = run_shortest_path([(nodes_a, a), (nodes_b, b)], 1, probe, 5000)
    dist = bfs(a + b, 1)
    missing = set(dist) - set(want)
    assert kinds == {"exact", "sketch"} and len(missing) > 1000 and all(k >= (1 << 41) + 10 ** 6 for k in missing)
    assert all(want[k] == dist[k] for k in want)


# ---- 6. refusals and empty graphs -------------------------------------------------------------------------------------------------
class Shard:
    """tables, a graph and filters with known content, one raw call per round step, and the read-back that shows nothing changed"""

    def __init__(self):
        regs = graphs.random_registers(np.random.default_rng(5), 60)
        self.space = list(range(1, 41))
        self.m = {"prev_c": {k: r for k, r in zip(self.space[:30], regs)}, "next_c": {k: r for k, r in zip(self.space[10:40], regs[30:])},
                  "prev_d": {k: 3 * k for k in self.space[:30]}, "next_d": {k: 100 + k for k in self.space[20:40]}, "prev_v": {}, "next_v": {}}
        self.t = {"prev_c": counter_table(self.m["prev_c"]), "next_c": counter_table(self.m["next_c"]), "prev_d": distance_table(self.m["prev_d"]),
                  "next_d": distance_table(self.m["next_d"]), "prev_v": ampc.ValueTable(KAHAN), "next_v": ampc.ValueTable(KAHAN)}
        self.edges = [(k, (k * 7) % 40 + 1) for k in self.space for _ in range(3)]
        self.graph = graph_of(self.space, self.edges, 50)
        self.m_changed = rref.Bloom(257)
        for k in self.space[:25]:
            self.m_changed.insert(k)
        self.changed, self.new = device_filter(self.m_changed), ampc.ChangedFilter.bloom(257)
        self.out = (ctypes.c_uint64 * 3)(9, 9, 9)
        self.far = []

    def call(self, step, **swap):
        """the step with its usual arguments, some of them replaced: a table / graph / filter object, or None for NULL"""
        a = dict(prev_c=self.t["prev_c"], next_c=self.t["next_c"], prev_d=self.t["prev_d"], next_d=self.t["next_d"], prev_v=self.t["prev_v"], next_v=self.t["next_v"],
                 graph=self.graph, changed=self.changed, new=self.new)
        a.update(swap)
        h = {k: (v.h if v is not None else None) for k, v in a.items()}
        lib, o = _lib.load(), [ctypes.byref(self.out, 8 * i) for i in range(3)]
        o = [ctypes.cast(x, ctypes.POINTER(ctypes.c_uint64)) for x in o]
        if step == "setup_counters":
            return lib.hbu_setup_counters(h["prev_c"], h["next_c"], h["graph"], h["changed"])
        if step == "round_counters":
            return lib.hbu_round_counters(h["prev_c"], h["next_c"], h["graph"], h["changed"], h["new"], o[0], o[1], o[2])
        if step == "round_distances":
            return lib.hbu_round_distances(h["prev_d"], h["next_d"], h["graph"], h["changed"], h["new"], o[0], o[1])
        return lib.hbu_round_centralities(h["prev_c"], h["next_c"], h["prev_v"], h["next_v"], h["graph"], h["changed"], 0, o[0], o[1])

    def unchanged(self, what):
        for name in ("prev_c", "next_c"):
            assert_counters(self.t[name], self.m[name], self.space, what)
        for name in ("prev_d", "next_d"):
            assert_table(self.t[name], U64, self.m[name], self.space, what)
        for name in ("prev_v", "next_v"):
            assert_table(self.t[name], KAHAN, self.m[name], self.space, what)
        assert_filter(self.changed, self.m_changed, self.space, what)
        assert_filter(self.new, rref.Bloom(257), self.space, what)

    def close(self):
        for x in list(self.t.values()) + [self.graph, self.changed, self.new] + self.far:
            x.close()


STEPS = {"setup_counters": ("prev_c", "next_c"), "round_counters": ("prev_c", "next_c"), "round_distances": ("prev_d", "next_d"),
         "round_centralities": ("prev_v", "next_v")}
REFUSALS = ["null_prev", "null_next", "null_graph", "null_changed", "prev_of_another_kind", "next_of_another_kind", "prev_is_next", "changed_is_new_changed",
            "other_device"]


# (setup_counters takes NULL for its filter; only the two edge steps have a second one)
CASES = [(step, refusal) for step in STEPS for refusal in REFUSALS
         if not (refusal == "null_changed" and step == "setup_counters") and not (refusal == "changed_is_new_changed" and step in ("setup_counters", "round_centralities"))]


@pytest.mark.parametrize("step,refusal", CASES)
def test_round_steps_refuse_and_change_nothing(step, refusal):
    """NULL for a table, the graph or the filter, a table of another kind on either side, one table as prev and next, one filter as changed
    and new_changed, an object on another device: HB_ERR_INVALID, a message on the table that changes (if there is one), zero counts, and a
    read-back of every table and filter equals the one before.  (A broken table cannot be made through the API without a failed batch.)"""
    if refusal == "other_device" and _lib.device_count() < 2:
        pytest.skip("needs two devices")
    prev, nxt = STEPS[step]
    wrong = {"prev_c": "prev_d", "next_c": "next_d", "prev_d": "prev_c", "next_d": "next_c", "prev_v": "prev_d", "next_v": "next_d"}
    s = Shard()
    try:
        blamed = s.t[nxt]
        if refusal == "null_prev":
            rc = s.call(step, **{prev: None})
        elif refusal == "null_next":
            rc, blamed = s.call(step, **{nxt: None}), None
        elif refusal == "null_graph":
            rc = s.call(step, graph=None)
        elif refusal == "null_changed":
            rc = s.call(step, changed=None)
        elif refusal == "prev_of_another_kind":
            rc = s.call(step, **{prev: s.t[wrong[prev]]})
        elif refusal == "next_of_another_kind":
            rc, blamed = s.call(step, **{nxt: s.t[wrong[nxt]]}), s.t[wrong[nxt]]
        elif refusal == "prev_is_next":
            rc = s.call(step, **{prev: s.t[nxt]})
        elif refusal == "changed_is_new_changed":
            rc = s.call(step, new=s.changed)
        else:
            s.far.append(ampc.ChangedFilter.bloom(257, device=1))
            rc = s.call(step, changed=s.far[0])
        assert rc == _lib.HB_ERR_INVALID, refusal
        if blamed is not None:
            with pytest.raises(_lib.HyperballError) as err:
                blamed._check(rc)
            assert str(err.value).split(": ", 1)[1], "no message"
        assert list(s.out) == {"setup_counters": [9, 9, 9], "round_counters": [0, 0, 0]}.get(step, [0, 0, 9])
        s.unchanged(refusal)
    finally:
        s.close()


@pytest.mark.parametrize("edges", [False, True])
def test_round_steps_on_an_empty_graph(edges):
    """an empty graph, and one with nodes but no edges (edges=True: a graph with edges and a filter that selects nothing): HB_OK, zero
    counts, nothing touched by the edge steps"""
    s = Shard()
    try:
        empty = graph_of([] if not edges else s.space, [], 50)
        s.far.append(empty)
        nothing = ampc.ChangedFilter.bloom(257)
        s.far.append(nothing)
        for step in ("round_counters", "round_distances"):
            for kw in (dict(graph=empty), dict(changed=nothing)):
                s.out[:] = [9, 9, 9]
                assert s.call(step, **kw) == _lib.HB_OK
                assert list(s.out)[:2] == [0, 0] and (step == "round_distances" or s.out[2] == 0)
        assert s.call("round_centralities", changed=nothing) == _lib.HB_OK and list(s.out)[:2] == [0, 0]
        if not edges:
            assert s.call("round_centralities", graph=empty) == _lib.HB_OK and list(s.out)[:2] == [0, 0]
            assert s.call("setup_counters", graph=empty) == _lib.HB_OK
        s.unchanged("empty")
        assert len(empty) == 0
    finally:
        s.close()
