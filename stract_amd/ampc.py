"""ctypes binding of include/hb_ampc.h: a GPU-resident shard of the AMPC table store.  CounterTable is the harmonic-centrality
counter table (`DefaultDhtTable<NodeID, HyperLogLog<64>>`, crates/core/src/entrypoint/ampc/harmonic_centrality/mod.rs:47-53) with the
three batch operations its mappers use (mapper.rs:52-118): batch_set, batch_get, batch_upsert(HyperLogLog64Upsert).  ValueTable is a
table of one of the scalar kinds (u64, f32, f64, KahanSum) with the scalar upsert operators (dht/upsert.rs:92-152): the `centrality`
table of that job and the `distances` table of the shortest-path job (shortest_path/mod.rs:51-55).  Both have clone() (clone_table,
dht/store.rs:192-195); update_centralities is mapper.rs:157-209 as one device call, update_counters (mapper.rs:89-111) and
update_distances (shortest_path/mapper.rs:64-86) are the two jobs' edge steps between two resident tables: edge ids go up, actions come back.
WorkerGraph and ChangedFilter keep a worker's edges and its changed-node filter (U64BloomFilter, or the Exact arm of UpdatedNodes) on the
device as well; setup_counters, round_counters, round_distances and round_centralities are the mapper steps between them and the tables
(only counts cross the link), run_harmonic_job and run_shortest_path_job the coordinator's loop over one resident shard.  items() is
DhtTable::iter(); fold_harmonic, WorkerGraph.node_sketch, num_samples and run_approx_harmonic_job are the approximated harmonic centrality
coordinator (approximated_harmonic_centrality/coordinator.rs:82-148) on top of the shortest-path job.  LaneTable holds one u8 distance
for each of up to 64 sources per row (HBU_KIND_DIST64); round_lane_distances, fold_harmonic_lanes and run_shortest_paths_job walk a whole
batch of sampled sources in one pass over the edges, and run_approx_harmonic_job(sources_per_walk=2..64) is the coordinator on top of them."""
import ctypes
import math
import os

import numpy as np

from . import _lib

NO_CHANGE, MERGED, INSERTED = 0, 1, 2  # UpsertAction, dht/upsert.rs:24-28
KIND_HLL64, KIND_U64, KIND_F32, KIND_F64, KIND_KAHAN = range(5)  # HBU_KIND_*
OP_HLL64, OP_U64_ADD, OP_U64_MIN, OP_F32_ADD, OP_F64_ADD, OP_KAHAN_ADD = range(6)  # HBU_OP_*
KAHAN = np.dtype([("sum", "<f8"), ("err", "<f8")])  # KahanSum, kahan_sum.rs:30-33
DTYPES = {KIND_U64: np.dtype(np.uint64), KIND_F32: np.dtype(np.float32), KIND_F64: np.dtype(np.float64), KIND_KAHAN: KAHAN}
KIND_DIST64, OP_DIST64_MIN = 5, 6  # HBU_KIND_DIST64, HBU_OP_DIST64_MIN: LaneTable's (not in DTYPES / OPS: those list the scalar kinds)
DIST_LANES, DIST_NONE = 64, 0xFF  # HBU_DIST_LANES, HBU_DIST_NONE
OPS = {KIND_HLL64: (OP_HLL64,), KIND_U64: (OP_U64_ADD, OP_U64_MIN), KIND_F32: (OP_F32_ADD,), KIND_F64: (OP_F64_ADD,), KIND_KAHAN: (OP_KAHAN_ADD,)}


class _Table:
    """What the two table classes share: the handle, its length, clone()."""

    def clone(self):
        """clone_table: a new table with the same kind, keys and values (device-to-device copies), independent afterwards"""
        h = ctypes.c_void_p()
        self._check(self.lib.hbu_clone(self.h, ctypes.byref(h)))
        new = object.__new__(type(self))
        new.__dict__.update(self.__dict__)
        new.h = h
        return new

    def close(self):
        if getattr(self, "h", None):
            self.lib.hbu_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _lib.HB_OK:
            raise _lib.HyperballError(rc, (self.lib.hbu_last_error(self.h) or b"").decode())

    def __len__(self):
        n = ctypes.c_uint64(0)
        self._check(self.lib.hbu_len(self.h, ctypes.byref(n)))
        return n.value

    def items(self):
        """DhtTable::iter(): (keys, values) of the whole table, keys[i] with values[i], in no particular order.  values: the kind's dtype,
        uint8[n, 64] for a counter table or a lane table."""
        n = len(self)
        keys = np.zeros(n, dtype=_lib.U128)
        values = np.zeros((n, 64), dtype=np.uint8) if self.kind in (KIND_HLL64, KIND_DIST64) else np.zeros(n, dtype=self.dtype)
        written = ctypes.c_uint64(0)
        self._check(self.lib.hbu_export(self.h, _lib._ptr(keys), _lib._ptr(values), n, ctypes.byref(written)))
        assert written.value == n
        return keys, values


class CounterTable(_Table):
    kind = KIND_HLL64

    def __init__(self, device=-1, capacity_hint=0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.hbu_create(device, capacity_hint, ctypes.byref(h))
        if rc != _lib.HB_OK:
            raise _lib.HyperballError(rc, (self.lib.hbu_last_error(None) or b"").decode())
        self.h = h

    @staticmethod
    def _args(keys, counters):
        keys = np.ascontiguousarray(keys, dtype=_lib.U128)
        counters = np.ascontiguousarray(counters, dtype=np.uint8).reshape(len(keys), 64)
        return keys, counters

    def batch_set(self, keys, counters):
        keys, counters = self._args(keys, counters)
        self._check(self.lib.hbu_batch_set(self.h, _lib._ptr(keys), _lib._ptr(counters), len(keys)))

    def batch_get(self, keys):
        keys = np.ascontiguousarray(keys, dtype=_lib.U128)
        out = np.zeros((len(keys), 64), dtype=np.uint8)
        found = np.zeros(len(keys), dtype=np.uint8)
        self._check(self.lib.hbu_batch_get(self.h, _lib._ptr(keys), len(keys), _lib._ptr(out), _lib._ptr(found)))
        return out, found.astype(bool)

    def batch_upsert(self, keys, counters):
        keys, counters = self._args(keys, counters)
        actions = np.zeros(len(keys), dtype=np.uint8)
        self._check(self.lib.hbu_batch_upsert(self.h, _lib._ptr(keys), _lib._ptr(counters), len(keys), _lib._ptr(actions)))
        return actions


class ValueTable(_Table):
    """A table of one scalar kind; values are numpy arrays of DTYPES[kind] (KIND_KAHAN: the (sum, err) structured dtype)."""

    def __init__(self, kind, device=-1, capacity_hint=0):
        self.lib = _lib.load()
        if kind not in DTYPES:
            raise ValueError("ValueTable kinds: KIND_U64, KIND_F32, KIND_F64, KIND_KAHAN (counters: CounterTable)")
        self.kind, self.dtype = kind, DTYPES[kind]
        h = ctypes.c_void_p()
        rc = self.lib.hbu_create_kind(device, capacity_hint, kind, ctypes.byref(h))
        if rc != _lib.HB_OK:
            raise _lib.HyperballError(rc, (self.lib.hbu_last_error(None) or b"").decode())
        self.h = h

    def _args(self, keys, values):
        keys = np.ascontiguousarray(keys, dtype=_lib.U128)
        values = np.ascontiguousarray(values, dtype=self.dtype)
        if values.shape != (len(keys),):
            raise ValueError("one value per key")
        return keys, values

    def batch_set(self, keys, values):
        keys, values = self._args(keys, values)
        self._check(self.lib.hbu_batch_set_values(self.h, _lib._ptr(keys), _lib._ptr(values), len(keys)))

    def batch_get(self, keys):
        """(values, found): an absent key reads as 0 / 0.0 / KahanSum::default()"""
        keys = np.ascontiguousarray(keys, dtype=_lib.U128)
        out = np.zeros(len(keys), dtype=self.dtype)
        found = np.zeros(len(keys), dtype=np.uint8)
        self._check(self.lib.hbu_batch_get_values(self.h, _lib._ptr(keys), len(keys), _lib._ptr(out), _lib._ptr(found)))
        return out, found.astype(bool)

    def batch_upsert(self, op, keys, values):
        """The pairs in order under operator `op` (OP_*); returns the action of every pair."""
        keys, values = self._args(keys, values)
        actions = np.zeros(len(keys), dtype=np.uint8)
        self._check(self.lib.hbu_batch_upsert_values(self.h, op, _lib._ptr(keys), _lib._ptr(values), len(keys), _lib._ptr(actions)))
        return actions

    def finish_centralities(self, divisor=1.0):
        """finish_centralities(self, divisor)"""
        return finish_centralities(self, divisor)

    def top_centralities(self, k, divisor=1.0):
        """top_centralities(self, k, divisor)"""
        return top_centralities(self, k, divisor)

    def store_centralities(self, output, divisor=1.0):
        """store_centralities(self, output, divisor)"""
        return store_centralities(self, output, divisor)


class LaneTable(_Table):
    """A table of 64-lane distance rows (HBU_KIND_DIST64): values are uint8[n, 64], lane l = the distance from source l of a batch, DIST_NONE
    (0xFF) = none.  batch_upsert is the byte-wise minimum (OP_DIST64_MIN)."""
    kind = KIND_DIST64

    def __init__(self, device=-1, capacity_hint=0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.hbu_create_kind(device, capacity_hint, KIND_DIST64, ctypes.byref(h))
        if rc != _lib.HB_OK:
            raise _lib.HyperballError(rc, (self.lib.hbu_last_error(None) or b"").decode())
        self.h = h

    @staticmethod
    def _args(keys, rows):
        keys = np.ascontiguousarray(keys, dtype=_lib.U128)
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(len(keys), DIST_LANES)
        return keys, rows

    def batch_set(self, keys, rows):
        keys, rows = self._args(keys, rows)
        self._check(self.lib.hbu_batch_set_values(self.h, _lib._ptr(keys), _lib._ptr(rows), len(keys)))

    def batch_get(self, keys):
        """(rows, found): an absent key reads as 64 x DIST_NONE"""
        keys = np.ascontiguousarray(keys, dtype=_lib.U128)
        out = np.zeros((len(keys), DIST_LANES), dtype=np.uint8)
        found = np.zeros(len(keys), dtype=np.uint8)
        self._check(self.lib.hbu_batch_get_values(self.h, _lib._ptr(keys), len(keys), _lib._ptr(out), _lib._ptr(found)))
        return out, found.astype(bool)

    def batch_upsert(self, keys, rows, op=OP_DIST64_MIN):
        """The pairs in order under the byte-wise minimum; returns the action of every pair."""
        keys, rows = self._args(keys, rows)
        actions = np.zeros(len(keys), dtype=np.uint8)
        self._check(self.lib.hbu_batch_upsert_values(self.h, op, _lib._ptr(keys), _lib._ptr(rows), len(keys), _lib._ptr(actions)))
        return actions

    def round_lane_distances(self, next, graph, changed, new_changed=None):
        """round_lane_distances(self, next, ...)"""
        return round_lane_distances(self, next, graph, changed, new_changed)

    def fold_harmonic_lanes(self, centralities, norm, n_lanes, skip_zero=False):
        """fold_harmonic_lanes(self, centralities, ...)"""
        return fold_harmonic_lanes(self, centralities, norm, n_lanes, skip_zero)


def wave_group_length():
    """Pairs of one key in a batch up to this many are folded by one thread of the upsert kernel, more by a whole wave."""
    return int(_lib.load().hbu_wave_group_length())


def update_centralities(prev_counters, next_counters, prev_centrality, next_centrality, nodes, round):
    """CentralityMapper::update_centralities (mapper.rs:157-209) on four resident tables: every node of `nodes` found in both
    counter tables whose size grew gets next_centrality[node] = prev_centrality[node] + growth / (round + 1).  Returns the number of
    distinct nodes written."""
    nodes = np.ascontiguousarray(nodes, dtype=_lib.U128)
    written = ctypes.c_uint64(0)
    rc = next_centrality.lib.hbu_update_centralities(prev_counters.h, next_counters.h, prev_centrality.h, next_centrality.h, _lib._ptr(nodes), len(nodes),
                                                     round, ctypes.byref(written))
    next_centrality._check(rc)
    return written.value


def _edges(from_ids, to_ids):
    from_ids = np.ascontiguousarray(from_ids, dtype=_lib.U128)
    to_ids = np.ascontiguousarray(to_ids, dtype=_lib.U128)
    if from_ids.shape != to_ids.shape or from_ids.ndim != 1:
        raise ValueError("one source and one destination per edge")
    return from_ids, to_ids


def update_counters(prev, next, from_ids, to_ids):
    """CentralityMapper::update_counters (mapper.rs:89-111) on two resident counter tables: for every edge in order, the counter of
    `from` in `prev` (or the default one) with `from` itself added is upserted into `to` of `next` with HyperLogLog64Upsert.  Returns
    the action of every edge (uint8 array)."""
    from_ids, to_ids = _edges(from_ids, to_ids)
    actions = np.zeros(len(from_ids), dtype=np.uint8)
    next._check(next.lib.hbu_update_counters(prev.h, next.h, _lib._ptr(from_ids), _lib._ptr(to_ids), len(from_ids), _lib._ptr(actions)))
    return actions


def update_distances(prev, next, from_ids, to_ids):
    """ShortestPathMapper::update_distances (shortest_path/mapper.rs:64-86) on two resident u64 tables: an edge whose source has no
    distance in `prev` is skipped; every other destination is upserted once into `next` with U64Min and the smallest `prev[from] + 1`
    of its edges.  Returns (keys, actions): one entry per such destination, in no particular order."""
    from_ids, to_ids = _edges(from_ids, to_ids)
    keys = np.zeros(len(from_ids), dtype=_lib.U128)
    actions = np.zeros(len(from_ids), dtype=np.uint8)
    written = ctypes.c_uint64(0)
    next._check(next.lib.hbu_update_distances(prev.h, next.h, _lib._ptr(from_ids), _lib._ptr(to_ids), len(from_ids), _lib._ptr(keys), _lib._ptr(actions),
                                              ctypes.byref(written)))
    return keys[:written.value].copy(), actions[:written.value].copy()


FOLD_SKIP_ZERO = 1  # HBU_FOLD_SKIP_ZERO


def fold_harmonic(distances, centralities, norm, skip_zero=False):
    """coordinator.rs:139-145 of the approximated harmonic centrality for one finished shortest-path job, as one device call: every
    (node, d) of `distances` (KIND_U64) adds KahanSum::from((1.0 / d as f64) * norm) to centralities[node] (KIND_KAHAN), inserting an absent
    node.  A distance of 0 (the source) gives inf, as in the reference, unless skip_zero.  Returns (folded, inserted)."""
    folded, inserted = ctypes.c_uint64(0), ctypes.c_uint64(0)
    centralities._check(centralities.lib.hbu_fold_harmonic(distances.h, centralities.h, float(norm), FOLD_SKIP_ZERO if skip_zero else 0, ctypes.byref(folded),
                                                           ctypes.byref(inserted)))
    return folded.value, inserted.value


def fold_harmonic_lanes(lanes, centralities, norm, n_lanes, skip_zero=False):
    """fold_harmonic for a finished batch held as lane rows (LaneTable): per node the lanes 0 .. n_lanes - 1 that hold a distance are folded
    in ascending order, which equals n_lanes calls of fold_harmonic, one per source in source order, bit for bit.  A node with no lane to
    fold is not inserted.  Returns (lanes folded, nodes inserted)."""
    folded, inserted = ctypes.c_uint64(0), ctypes.c_uint64(0)
    centralities._check(centralities.lib.hbu_fold_harmonic_lanes(lanes.h, centralities.h, float(norm), int(n_lanes), FOLD_SKIP_ZERO if skip_zero else 0,
                                                                 ctypes.byref(folded), ctypes.byref(inserted)))
    return folded.value, inserted.value


def finish_centralities(table, divisor=1.0):
    """The finished job's results from its centrality table (KIND_KAHAN: f64::from(KahanSum) = .sum; or KIND_F64), every key a result:
    (ids, vals, ranks) in ascending NodeID order - vals = value / divisor (harmonic_centrality/coordinator.rs:204-211 passes num_nodes - 1,
    the approximated job 1.0), ranks = the position in store_harmonic's order (value descending under f64::total_cmp, ties by NodeID
    ascending; webgraph/centrality/mod.rs:92-103).  Sorted on the device; the table is only read."""
    n = len(table)
    ids, vals, ranks = np.zeros(n, dtype=_lib.U128), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint64)
    written = ctypes.c_uint64(0)
    table._check(table.lib.hbu_finish_centralities(table.h, float(divisor), _lib._ptr(ids), _lib._ptr(vals), _lib._ptr(ranks), n, ctypes.byref(written)))
    assert written.value == n
    return ids, vals, ranks


def top_centralities(table, k, divisor=1.0):
    """top_nodes (webgraph/centrality/mod.rs:33-52): (ids, vals) of the first min(k, len) entries of the rank order of finish_centralities,
    gathered on the device."""
    top = min(int(k), len(table))
    ids, vals = np.zeros(top, dtype=_lib.U128), np.zeros(top, dtype=np.float64)
    written = ctypes.c_uint64(0)
    table._check(table.lib.hbu_top_centralities(table.h, float(divisor), int(k), _lib._ptr(ids), _lib._ptr(vals), ctypes.byref(written)))
    assert written.value == top
    return ids, vals


def store_centralities(table, output, divisor=1.0):
    """store_harmonic (webgraph/centrality/mod.rs:72-114): the databases `harmonic` and `harmonic_rank` under `output`, the same files as
    _lib.store_harmonic(output, *finish_centralities(table, divisor)); values, ranks and key order come off the device."""
    err = ctypes.create_string_buffer(512)
    rc = table.lib.hbu_store_centralities(table.h, float(divisor), os.fsencode(output), err, len(err))
    if rc != _lib.HB_OK:
        raise _lib.HyperballError(rc, err.value.decode(errors="replace"))


def num_samples(num_nodes, sample_rate):
    """coordinator.rs:82-84: ((num_nodes as f64).log2() / sample_rate.powi(2)).ceil() as u64 (`as u64` saturates: NaN and negatives are 0)"""
    n = float(int(num_nodes))
    log2 = math.log2(n) if n > 0.0 else -math.inf  # (libm's log2, as Rust's f64::log2)
    with np.errstate(all="ignore"):
        v = float(np.ceil(np.float64(log2) / (np.float64(sample_rate) * np.float64(sample_rate))))
    if not v > 0.0:
        return 0
    return min(int(v), (1 << 64) - 1) if v != math.inf else (1 << 64) - 1


# ---- a worker's graph and changed-node filter on the device, the mapper steps, the two jobs' loops ----------------------------------
FILTER_BLOOM, FILTER_EXACT = 0, 1  # HBU_FILTER_*
SKETCH_THRESHOLD = 16_384  # shortest_path/updated_nodes.rs:22


def _raise_thread_error(lib, rc):
    if rc != _lib.HB_OK:
        raise _lib.HyperballError(rc, (lib.hbu_last_error(None) or b"").decode())


class _Handle:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WorkerGraph(_Handle):
    """What worker.graph() yields, resident on one device (hbu_graph): `nodes` in host_nodes() order, the edges (from_ids[i], to_ids[i])
    in the worker's iteration order, edges with skipped rel flags already dropped.  chunk_edges: edges per internal pass of a round call
    (0 = the library's default).  `nodes` stays available on the host for reading results back."""

    def __init__(self, nodes, from_ids, to_ids, chunk_edges=0, device=-1):
        self.lib = _lib.load()
        self.nodes = np.ascontiguousarray(nodes, dtype=_lib.U128)
        from_ids, to_ids = _edges(from_ids, to_ids)
        h = ctypes.c_void_p()
        _raise_thread_error(self.lib, self.lib.hbu_graph_create(device, _lib._ptr(self.nodes), len(self.nodes), _lib._ptr(from_ids), _lib._ptr(to_ids), len(from_ids),
                                                                int(chunk_edges), ctypes.byref(h)))
        self.h = h
        self.n_nodes, self.n_edges = len(self.nodes), len(from_ids)

    def close(self):
        if getattr(self, "h", None):
            self.lib.hbu_graph_destroy(self.h)
            self.h = None

    def __len__(self):
        n, m = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _raise_thread_error(self.lib, self.lib.hbu_graph_len(self.h, ctypes.byref(n), ctypes.byref(m)))
        assert (n.value, m.value) == (self.n_nodes, self.n_edges)
        return m.value

    def node_sketch(self):
        """ShortestPathWorker::nodes_sketch (shortest_path/worker.rs:44-49): the registers of HyperLogLog<4096> after add_u128 of every node,
        uint8[4096].  Workers' sketches merge with np.maximum; the estimate stays with the caller."""
        out = np.zeros(4096, dtype=np.uint8)
        _raise_thread_error(self.lib, self.lib.hbu_graph_node_sketch(self.h, _lib._ptr(out)))
        return out


class ChangedFilter(_Handle):
    """The changed-node filter on the device (hbu_filter): ChangedFilter.bloom(num_bits) is U64BloomFilter (crates/bloom/src/lib.rs:60-130),
    ChangedFilter.exact() the Exact arm of UpdatedNodes (shortest_path/updated_nodes.rs:27-44), a set of whole 128-bit ids."""

    def __init__(self, kind, num_bits=0, device=-1):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        _raise_thread_error(self.lib, self.lib.hbu_filter_create(device, kind, int(num_bits), ctypes.byref(h)))
        self.h, self.kind, self.num_bits, self.device = h, kind, (int(num_bits) if kind == FILTER_BLOOM else 0), device

    @classmethod
    def bloom(cls, num_bits, device=-1):
        return cls(FILTER_BLOOM, num_bits, device)

    @classmethod
    def exact(cls, device=-1):
        return cls(FILTER_EXACT, 0, device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.hbu_filter_destroy(self.h)
            self.h = None

    def _check(self, rc):
        _raise_thread_error(self.lib, rc)

    def clear(self):
        """empty_from"""
        self._check(self.lib.hbu_filter_clear(self.h))

    def fill(self):
        self._check(self.lib.hbu_filter_fill(self.h))

    def insert(self, ids):
        ids = np.ascontiguousarray(ids, dtype=_lib.U128)
        self._check(self.lib.hbu_filter_insert(self.h, _lib._ptr(ids), len(ids)))

    def contains(self, ids):
        ids = np.ascontiguousarray(ids, dtype=_lib.U128)
        out = np.zeros(len(ids), dtype=np.uint8)
        self._check(self.lib.hbu_filter_contains(self.h, _lib._ptr(ids), len(ids), _lib._ptr(out)))
        return out.astype(bool)

    def union(self, other):
        """self |= other (one kind, one size)"""
        self._check(self.lib.hbu_filter_union(self.h, other.h))

    def count(self):
        """count_ones() of a bloom filter, len() of an exact set"""
        n = ctypes.c_uint64(0)
        self._check(self.lib.hbu_filter_count(self.h, ctypes.byref(n)))
        return n.value

    def export_bits(self):
        """the bit vector's data words (uint64, bit i = bit i % 64 of word i // 64); bloom only"""
        words = np.zeros((self.num_bits + 63) // 64 if self.kind == FILTER_BLOOM else 1, dtype=np.uint64)
        self._check(self.lib.hbu_filter_export_bits(self.h, _lib._ptr(words)))
        return words

    def import_bits(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        if self.kind == FILTER_BLOOM and len(words) != (self.num_bits + 63) // 64:
            raise ValueError("ceil(num_bits / 64) words")
        self._check(self.lib.hbu_filter_import_bits(self.h, _lib._ptr(words)))

    def export_ids(self):
        """the members of an exact set (U128 array, no particular order)"""
        cap = self.count() if self.kind == FILTER_EXACT else 1
        out = np.zeros(max(cap, 1), dtype=_lib.U128)
        written = ctypes.c_uint64(0)
        self._check(self.lib.hbu_filter_export_ids(self.h, _lib._ptr(out), len(out), ctypes.byref(written)))
        return out[:written.value].copy()


def bloom_num_bits(estimated_items, fp):
    """num_bits() of the bloom crate (lib.rs:40-42)"""
    return int(_lib.load().hbu_bloom_num_bits(int(estimated_items), float(fp)))


def _h(x):
    return x.h if x is not None else None


def setup_counters(prev, next, graph, changed=None):
    """map_setup_counters (mapper.rs:211-242): both tables get HyperLogLog::default() + add_u128(node) for every node of the graph; every
    node is inserted into `changed` if given."""
    next._check(next.lib.hbu_setup_counters(prev.h, next.h, graph.h, _h(changed)))


def round_counters(prev, next, graph, changed, new_changed=None):
    """map_cardinalities (mapper.rs:253-296): the edges whose source `changed` contains go through update_counters; the destinations of
    the Merged pairs are inserted into new_changed.  Returns (selected, merged, inserted)."""
    s, m, i = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    next._check(next.lib.hbu_round_counters(prev.h, next.h, graph.h, _h(changed), _h(new_changed), ctypes.byref(s), ctypes.byref(m), ctypes.byref(i)))
    return s.value, m.value, i.value


def round_distances(prev, next, graph, changed, new_changed=None):
    """RelaxEdges for the graph's edges (shortest_path/mapper.rs:105-190): the edges whose source `changed` contains go through
    update_distances, a chunk at a time; every Merged or Inserted destination is inserted into new_changed.  Returns (selected,
    changed_nodes)."""
    s, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
    next._check(next.lib.hbu_round_distances(prev.h, next.h, graph.h, _h(changed), _h(new_changed), ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def round_lane_distances(prev, next, graph, changed, new_changed=None):
    """RelaxEdges for 64 sources in one pass over the graph's edges, between two LaneTables: an edge whose source `changed` contains and
    that has a row in `prev` gives its destination that row + 1 on every lane with a distance (254 + 1: none), upserted into `next` with the
    byte-wise minimum in edge order; every Merged or Inserted destination is inserted into new_changed.  Returns (selected, merged,
    inserted)."""
    s, m, i = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    next._check(next.lib.hbu_round_lane_distances(prev.h, next.h, graph.h, _h(changed), _h(new_changed), ctypes.byref(s), ctypes.byref(m), ctypes.byref(i)))
    return s.value, m.value, i.value


def round_centralities(prev_counters, next_counters, prev_centrality, next_centrality, graph, changed, round):
    """map_centralities (mapper.rs:298-333): the graph's nodes that `changed` contains go through update_centralities.  Returns (selected,
    written)."""
    s, w = ctypes.c_uint64(0), ctypes.c_uint64(0)
    next_centrality._check(next_centrality.lib.hbu_round_centralities(prev_counters.h, next_counters.h, prev_centrality.h, next_centrality.h, graph.h, _h(changed),
                                                                      round, ctypes.byref(s), ctypes.byref(w)))
    return s.value, w.value


def run_harmonic_job(graphs, device=-1, on_round=None, output=None):
    """The harmonic-centrality coordinator's loop (harmonic_centrality/coordinator.rs:122-135, ampc/coordinator.rs:151-213) over one resident
    shard and the workers `graphs` (WorkerGraph each): per round clone, then SetupCounters (round 0), SetupBloom (round 0: every filter
    filled, num_bits = bloom_num_bits(sum of the workers' node counts, 0.05), worker.rs:49-71), Cardinalities, SaveBloom / UpdateBloom
    (every worker's filter becomes the union of all of them), Centralities, swap - until a round neither merged nor inserted.  Returns
    {node id as int: f64::from(centrality) / (num_keys - 1)} (coordinator.rs:204-211).  on_round(state): called at the end of every round
    with the live tables, filters and counts (tests).  output: a directory that gets store_harmonic's two databases (coordinator.rs:213-214)
    from the resident table, store_centralities(centrality, output, num_keys - 1), before the tables close."""
    graphs = list(graphs)
    total_nodes = sum(g.n_nodes for g in graphs)
    if not total_nodes:
        return {}
    num_bits = bloom_num_bits(total_nodes, 0.05)
    prev_c, prev_v = CounterTable(device), ValueTable(KIND_KAHAN, device)
    changed = [ChangedFilter.bloom(num_bits, device) for _ in graphs]
    spare = [ChangedFilter.bloom(num_bits, device) for _ in graphs]
    union = ChangedFilter.bloom(num_bits, device)
    open_tables = []  # the clones of the round under way: closed if the round does not end
    try:
        for f in changed:
            f.fill()
        had_changes, worker_round = True, 0  # Meta.round_had_changes of prev (forced for the first round), CentralityWorker::round
        while had_changes:  # CentralityFinish::is_finished
            next_c = prev_c.clone()
            open_tables.append(next_c)
            next_v = prev_v.clone()
            open_tables.append(next_v)
            now, counts = False, []
            if worker_round == 0:
                for g in graphs:
                    setup_counters(prev_c, next_c, g)
            for w, g in enumerate(graphs):  # Cardinalities
                spare[w].clear()
                selected, merged, inserted = round_counters(prev_c, next_c, g, changed[w], spare[w])
                changed[w], spare[w] = spare[w], changed[w]
                now |= merged + inserted > 0
                counts.append((selected, merged, inserted))
            union.clear()  # SaveBloom, UpdateBloom
            for f in changed:
                union.union(f)
            for f in changed:
                f.union(union)
            written = [round_centralities(prev_c, next_c, prev_v, next_v, g, changed[w], worker_round) for w, g in enumerate(graphs)]  # Centralities
            worker_round += 1
            if on_round:
                on_round(dict(round=worker_round - 1, prev_counters=prev_c, next_counters=next_c, prev_centrality=prev_v, next_centrality=next_v, filters=changed,
                              counts=counts, written=written, had_changes=now))
            prev_c.close()
            prev_v.close()
            prev_c, prev_v, had_changes = next_c, next_v, now
            open_tables.clear()
        if output is not None:
            store_centralities(prev_v, output, float(len(prev_c) - 1))
        nodes = np.unique(np.concatenate([g.nodes for g in graphs]))
        vals, found = prev_v.batch_get(nodes)
        with np.errstate(all="ignore"):
            scaled = vals["sum"] / np.float64(len(prev_c) - 1)
        return {(int(k["hi"]) << 64) | int(k["lo"]): float(v) for k, v, f in zip(nodes, scaled, found) if f}
    finally:
        for f in changed + spare + [union] + open_tables:
            f.close()
        prev_c.close()
        prev_v.close()


class _UpdatedNodes:
    """UpdatedNodes (shortest_path/updated_nodes.rs) around device filters: the Exact -> Sketch policy the C ABI leaves to its caller."""

    def __init__(self, total_nodes, device, filt=None):
        self.total_nodes, self.device = total_nodes, device
        self.f = filt if filt is not None else ChangedFilter.exact(device)

    def _sketch(self):
        return ChangedFilter.bloom(bloom_num_bits(self.total_nodes, 0.01), self.device)

    def settle(self):
        """what add() does as soon as an exact set exceeds the threshold (updated_nodes.rs:89-103): a sketch of ALL of its ids"""
        if self.f.kind == FILTER_EXACT and self.f.count() > SKETCH_THRESHOLD:
            sketch = self._sketch()
            sketch.insert(self.f.export_ids())
            self.f.close()
            self.f = sketch
        return self

    def add(self, node_ids):
        self.f.insert(node_ids)
        return self.settle()

    def union(self, other):
        """updated_nodes.rs:46-87; returns a new _UpdatedNodes"""
        a, b = self.f, other.f
        if a.kind == FILTER_EXACT and b.kind == FILTER_EXACT:
            both = ChangedFilter.exact(self.device)
            both.union(a)
            both.union(b)
            if both.count() <= SKETCH_THRESHOLD:
                return _UpdatedNodes(self.total_nodes, self.device, both)
            # Exact u Exact over the threshold: the reference builds the sketch from the LEFT set only (updated_nodes.rs:48-58, `for node in
            # nodes`, not new_nodes); restated as it is
            both.close()
            sketch = self._sketch()
            sketch.insert(a.export_ids())
            return _UpdatedNodes(self.total_nodes, self.device, sketch)
        sketch = self._sketch()
        for f in (a, b):
            if f.kind == FILTER_BLOOM:
                sketch.union(f)
            else:
                sketch.insert(f.export_ids())
        return _UpdatedNodes(self.total_nodes, self.device, sketch)

    def close(self):
        self.f.close()


def run_shortest_path_job(graphs, source, max_distance=None, device=-1, on_round=None):
    """The shortest-path coordinator's loop (shortest_path/coordinator.rs:73-133) over one resident shard and the workers `graphs`: the
    source gets distance 0; per round clone, RelaxEdges on every worker (its changed set, with the source added, selects the edges; the
    changed destinations form its new set), UpdateChangedNodes (every worker's set becomes the union of all new sets, folded from an empty
    exact set in worker order), until a round changed nothing or `max_distance` rounds ran.  A set is exact up to 16 384 ids, then a bloom
    filter of bloom_num_bits(total_nodes, 0.01) bits.  round_had_changes is the OR over the workers (the reference stores the flag of
    whichever worker wrote last).  Returns the distance table (ValueTable of KIND_U64); the caller closes it."""
    graphs = list(graphs)
    total_nodes = max(sum(g.n_nodes for g in graphs), 1)
    src = np.zeros(1, dtype=_lib.U128)
    src["lo"], src["hi"] = int(source) & ((1 << 64) - 1), int(source) >> 64
    prev = ValueTable(KIND_U64, device)
    changed = [_UpdatedNodes(total_nodes, device) for _ in graphs]
    saved, nxt = [], None  # nxt: the clone of the round under way, closed if the round does not end
    try:
        prev.batch_set(src, np.zeros(1, dtype=np.uint64))
        rounds, had_changes = 0, True
        while had_changes and not (max_distance is not None and rounds >= max_distance):  # ShortestPathFinish::is_finished
            nxt = prev.clone()
            now, counts, saved = False, [], []
            for w, g in enumerate(graphs):  # RelaxEdges
                changed[w].add(src)
                new = _UpdatedNodes(total_nodes, device)
                saved.append(new)
                selected, changed_nodes = round_distances(prev, nxt, g, changed[w].f, new.f)
                new.settle()
                now |= changed_nodes > 0
                counts.append((selected, changed_nodes))
            for w in range(len(graphs)):  # UpdateChangedNodes
                acc = _UpdatedNodes(total_nodes, device)
                for other in saved:
                    merged = acc.union(other)
                    acc.close()
                    acc = merged
                changed[w].close()
                changed[w] = acc
            rounds += 1
            if on_round:
                on_round(dict(round=rounds - 1, prev=prev, next=nxt, filters=[c.f for c in changed], saved=[s.f for s in saved], counts=counts, had_changes=now))
            for s_ in saved:
                s_.close()
            saved = []
            prev.close()
            prev, had_changes, nxt = nxt, now, None
        return prev
    except BaseException:
        prev.close()
        if nxt is not None:
            nxt.close()
        raise
    finally:
        for c in changed + saved:
            c.close()


def _ids(values):
    ids = np.zeros(len(values), dtype=_lib.U128)
    ids["lo"] = [int(v) & ((1 << 64) - 1) for v in values]
    ids["hi"] = [int(v) >> 64 for v in values]
    return ids


def run_shortest_paths_job(graphs, sources, max_distance, device=-1, on_round=None):
    """run_shortest_path_job's loop for 1 .. 64 sources at once, lane l of every row = the distance from sources[l] (max_distance <= 254: a
    lane is a u8 and 0xFF means none).  The first table holds one row per DISTINCT source with 0 in every lane that names it (a source
    listed twice has two lanes); every worker's changed set gets ALL the batch's sources added each round; the loop ends when a round
    changed nothing or `max_distance` rounds ran.  The table does not depend on which edges the changed sets select (a candidate is never
    below the BFS distance, and the union over the lanes misses no edge a lane needs), so lane l equals run_shortest_path_job(sources[l]).
    Returns the LaneTable; the caller closes it."""
    graphs, sources = list(graphs), [int(s) for s in sources]
    if not 1 <= len(sources) <= DIST_LANES:
        raise ValueError("1 .. 64 sources per walk")
    if not 0 <= int(max_distance) <= DIST_NONE - 1:
        raise ValueError("max_distance <= 254 in a lane table (255 stays with run_shortest_path_job, the per-source route)")
    total_nodes = max(sum(g.n_nodes for g in graphs), 1)
    first = {}
    for lane, s in enumerate(sources):
        first.setdefault(s, np.full(DIST_LANES, DIST_NONE, dtype=np.uint8))[lane] = 0
    src = _ids(list(first))
    prev = LaneTable(device)
    changed = [_UpdatedNodes(total_nodes, device) for _ in graphs]
    saved, nxt = [], None  # nxt: the clone of the round under way, closed if the round does not end
    try:
        prev.batch_set(src, np.stack(list(first.values())))
        rounds, had_changes = 0, True
        while had_changes and rounds < int(max_distance):  # ShortestPathFinish::is_finished
            nxt = prev.clone()
            now, counts, saved = False, [], []
            for w, g in enumerate(graphs):  # RelaxEdges
                changed[w].add(src)
                new = _UpdatedNodes(total_nodes, device)
                saved.append(new)
                selected, merged, inserted = round_lane_distances(prev, nxt, g, changed[w].f, new.f)
                new.settle()
                now |= merged + inserted > 0
                counts.append((selected, merged, inserted))
            for w in range(len(graphs)):  # UpdateChangedNodes
                acc = _UpdatedNodes(total_nodes, device)
                for other in saved:
                    merged_set = acc.union(other)
                    acc.close()
                    acc = merged_set
                changed[w].close()
                changed[w] = acc
            rounds += 1
            if on_round:
                on_round(dict(round=rounds - 1, prev=prev, next=nxt, filters=[c.f for c in changed], saved=[s.f for s in saved], counts=counts, had_changes=now))
            for s_ in saved:
                s_.close()
            saved = []
            prev.close()
            prev, had_changes, nxt = nxt, now, None
        return prev
    except BaseException:
        prev.close()
        if nxt is not None:
            nxt.close()
        raise
    finally:
        for c in changed + saved:
            c.close()


def run_approx_harmonic_job(graphs, sampled_nodes, num_samples, max_distance, device=-1, skip_zero=False, on_source=None, sources_per_walk=1, output=None):
    """The approximated harmonic centrality coordinator's loop (approximated_harmonic_centrality/coordinator.rs:107-148) over one resident
    shard and the workers `graphs`: norm = 1.0 / (num_samples - 1) - from num_samples, not from len(sampled_nodes), which the per-worker
    div_ceil can make larger -, then for every source of `sampled_nodes` IN THE ORDER GIVEN (it is a node's summation order and therefore its
    bits) the shortest-path job with `max_distance`, its distances folded into one KahanSum table (fold_harmonic), its tables dropped.
    Sampling the sources and sizing the sample (node_sketch, num_samples) stay with the caller.  A source's own distance is 0 and folds as
    inf, as in the reference, unless skip_zero.  Returns {node id as int: f64::from(sum)}.  on_source(state): called after every source
    with the live centrality table and the fold's counts (tests).
    sources_per_walk = 2 .. 64: the sources are taken in the order given in consecutive batches of that many, each batch is one
    run_shortest_paths_job (one walk over the edges per round for all of its sources) and one fold_harmonic_lanes; the result is the same
    dictionary bit for bit.  on_source is then called once per batch: index = the batch's first index, sources = its list, lanes = the
    batch's LaneTable (closed after the call).  max_distance above 254 does not fit a lane.
    output: a directory that gets store_harmonic's two databases (coordinator.rs:159-160) from the resident table,
    store_centralities(centralities, output, 1.0), before the table closes."""
    graphs = list(graphs)
    sources_per_walk = int(sources_per_walk)
    if not 1 <= sources_per_walk <= DIST_LANES:
        raise ValueError("sources_per_walk: 1 .. 64")
    if sources_per_walk > 1 and int(max_distance) > DIST_NONE - 1:
        raise ValueError("max_distance above 254 does not fit a lane: use the per-source route (sources_per_walk=1)")
    if int(num_samples) < 1:
        raise ValueError("num_samples - 1 underflows (the reference panics)")
    with np.errstate(all="ignore"):
        norm = float(np.float64(1.0) / np.float64(int(num_samples) - 1))  # num_samples == 1: 1.0 / 0 = inf
    with ValueTable(KIND_KAHAN, device) as centralities:
        batched = [int(s) for s in sampled_nodes] if sources_per_walk > 1 else []
        for i in range(0, len(batched), sources_per_walk):  # several sources per walk: one lane table per batch
            batch = batched[i:i + sources_per_walk]
            lanes = run_shortest_paths_job(graphs, batch, int(max_distance), device)
            try:
                folded, inserted = fold_harmonic_lanes(lanes, centralities, norm, len(batch), skip_zero)
                if on_source:
                    on_source(dict(index=i, sources=batch, lanes=lanes, centralities=centralities, folded=folded, inserted=inserted))
            finally:
                lanes.close()  # drop_tables
        for i, source in enumerate(sampled_nodes if sources_per_walk == 1 else ()):
            distances = run_shortest_path_job(graphs, source, int(max_distance), device)
            try:
                folded, inserted = fold_harmonic(distances, centralities, norm, skip_zero)
            finally:
                distances.close()  # drop_tables
            if on_source:
                on_source(dict(index=i, source=int(source), centralities=centralities, folded=folded, inserted=inserted))
        if output is not None:
            store_centralities(centralities, output, 1.0)
        keys, values = centralities.items()
        return {(int(k["hi"]) << 64) | int(k["lo"]): float(v) for k, v in zip(keys, values["sum"])}
