"""ctypes binding of include/hb_ampc.h: a GPU-resident shard of the AMPC table store.  CounterTable is the harmonic-centrality
counter table (`DefaultDhtTable<NodeID, HyperLogLog<64>>`, crates/core/src/entrypoint/ampc/harmonic_centrality/mod.rs:47-53) with the
three batch operations its mappers use (mapper.rs:52-118): batch_set, batch_get, batch_upsert(HyperLogLog64Upsert).  ValueTable is a
table of one of the scalar kinds (u64, f32, f64, KahanSum) with the scalar upsert operators (dht/upsert.rs:92-152): the `centrality`
table of that job and the `distances` table of the shortest-path job (shortest_path/mod.rs:51-55).  Both have clone() (clone_table,
dht/store.rs:192-195); update_centralities is mapper.rs:157-209 as one device call, update_counters (mapper.rs:89-111) and
update_distances (shortest_path/mapper.rs:64-86) are the two jobs' edge steps between two resident tables: edge ids go up, actions come back."""
import ctypes

import numpy as np

from . import _lib

NO_CHANGE, MERGED, INSERTED = 0, 1, 2  # UpsertAction, dht/upsert.rs:24-28
KIND_HLL64, KIND_U64, KIND_F32, KIND_F64, KIND_KAHAN = range(5)  # HBU_KIND_*
OP_HLL64, OP_U64_ADD, OP_U64_MIN, OP_F32_ADD, OP_F64_ADD, OP_KAHAN_ADD = range(6)  # HBU_OP_*
KAHAN = np.dtype([("sum", "<f8"), ("err", "<f8")])  # KahanSum, kahan_sum.rs:30-33
DTYPES = {KIND_U64: np.dtype(np.uint64), KIND_F32: np.dtype(np.float32), KIND_F64: np.dtype(np.float64), KIND_KAHAN: KAHAN}
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
