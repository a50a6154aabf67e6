"""One model of an AMPC shard "world" for the state tests (tests/test_ampc_state.py, tools/diff_fuzz.py --mode ampc): the live tables by
kind, the live WorkerGraphs and the live ChangedFilters as plain dicts and sets, and a table of operations that covers every public call
of stract_amd/ampc.py.  An operation has four members: draw(rng, world) -> args or None, model(world, args) -> the expected answer (and
the state change), device(handles, args) -> the answer of the library, compare(got, want).  The model adds no arithmetic of its own: every
value comes from tests/ampc_ref.py, ampc_round_ref.py, ampc_approx_ref.py, ampc_lanes_ref.py, ampc_finish_ref.py and oracle/hbo.py.

What a table carries from one call to the next - committed / d_next, the key index and its rebuild at load factor 1/2, the value array,
the work memory that only grows, the pinned word - is what the sequences are after; the conditions (a) .. (m) of DESIGN.md section 35
are counted here from the model alone (`python -m tests.ampc_model --seeds ...` loads no library)."""
import argparse
import collections
import json
import sys

import numpy as np

from tests import ampc_approx_ref as aref
from tests import ampc_finish_ref as fref
from tests import ampc_lanes_ref as lref
from tests import ampc_ref as ref
from tests import ampc_round_ref as rref
from tests.ampc_slots import FIRST_SLOTS, keys_with_home, slots_for

M64 = (1 << 64) - 1
NAN64 = 0x7FF8000000000000
KINDS = ["HLL64", "U64", "F32", "F64", "KAHAN", "DIST64"]
KIND_CODE = {k: i for i, k in enumerate(KINDS)}  # HBU_KIND_*
OPS_OF = {"HLL64": [ref.HLL64], "U64": [ref.U64_ADD, ref.U64_MIN], "F32": [ref.F32_ADD], "F64": [ref.F64_ADD], "KAHAN": [ref.KAHAN_ADD], "DIST64": [6]}
WAVE_GROUP = 32  # hbu_wave_group_length(); the device runs assert that the library says the same
EDGES_AHEAD = 8  # kEdgesAhead of hb_ampc_edges.hip.h
SIZES = [0, 1, 16, 17, 64, 65, 257, 1000]
SIZE_WEIGHTS = [1, 1, 1, 2, 2, 3, 4, 6]  # a batch to write: the long ones more often, so that tables pass 512 and 1024 keys in mid-life
MULTIPLICITIES = [EDGES_AHEAD, EDGES_AHEAD + 1, WAVE_GROUP, WAVE_GROUP + 1, 64, 65]
INDEX_SIZES = [1024, 2048, 4096]
BLOOM_BITS = [257, 4099]
NORMS = [1.0, 1.0 / 3.0, 1.0 / 2657.0, 0.5]
DIVISORS = [1.0, 3.0, 2657.0, 0.5, -2.0]
CHUNKS = [0, 64, 100, 1000]
N_OPS = 100  # operations of one sequence
COMPARE_EVERY = 8
MAX_KEYS, MAX_LANE_KEYS = 2600, 600  # a table above this is closed and made anew (the lane model folds 64 lanes per key in Python)
NEED = {"a": 5, "b": 3, "c": 3, "d": 2, "e_upsert_after_round": 20, "e_round_after_upsert": 20, "f": 5, "g": 10, "h": 5, "i": 5, "j": 5, "k_fresh": 3, "k_stored": 3, "l": 3,
        "m": 20}
MAX_DROPPED, MAX_REFUSED = 0.05, 0.15


# ---- canonical forms: what an answer is compared as --------------------------------------------------------------------------------
def keys_of(keys):
    return [(hi << 64) | lo for lo, hi in zip(keys["lo"].tolist(), keys["hi"].tolist())]


def u128(ints):
    from stract_amd import _lib
    a = np.zeros(len(ints), dtype=_lib.U128)
    a["lo"] = np.array([k & M64 for k in ints], dtype=np.uint64)
    a["hi"] = np.array([k >> 64 for k in ints], dtype=np.uint64)
    return a


def canon_value(kind, v):
    """a model value as bit patterns; every NaN as one pattern (its sign and payload are not pinned, tests/test_ampc_values.py)"""
    if kind in ("HLL64", "DIST64"):
        return v.tobytes()  # (the 64 registers or lanes of a row)
    if kind == "U64":
        return int(v)
    if kind == "F32":
        return 0x7FC00000 if v != v else int(np.float32(v).view(np.uint32))
    if kind == "F64":
        return aref.bits(float(v))
    return (aref.bits(v[0]), aref.bits(v[1]))


def canon_array(kind, arr):
    """a device array as the list of canon_value()s"""
    if kind in ("HLL64", "DIST64"):
        raw = np.ascontiguousarray(arr, dtype=np.uint8).tobytes()
        return [raw[i:i + 64] for i in range(0, len(raw), 64)]
    if kind == "U64":
        return [int(x) for x in arr.tolist()]
    if kind == "F32":
        b = arr.view(np.uint32).copy()
        b[np.isnan(arr)] = 0x7FC00000
        return [int(x) for x in b.tolist()]

    def bits64(f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        b = f.view(np.uint64).copy()
        b[np.isnan(f)] = NAN64
        return [int(x) for x in b.tolist()]
    if kind == "F64":
        return bits64(arr)
    return list(zip(bits64(arr["sum"]), bits64(arr["err"])))


def default_of(kind):
    return {"HLL64": np.zeros(64, np.uint8), "DIST64": lref.row(), "U64": 0, "F32": np.float32(0.0), "F64": 0.0, "KAHAN": ref.KAHAN_DEFAULT}[kind]


def device_values(kind, values):
    """model values as the array the device takes"""
    from stract_amd import ampc
    values = list(values)
    if kind in ("HLL64", "DIST64"):
        return np.stack(values).astype(np.uint8) if values else np.zeros((0, 64), np.uint8)
    if kind == "KAHAN":
        a = np.zeros(len(values), dtype=ampc.KAHAN)
        a["sum"], a["err"] = [v[0] for v in values], [v[1] for v in values]
        return a
    return np.array(values, dtype=ampc.DTYPES[KIND_CODE[kind]]).reshape(len(values))


def model_items(t):
    return sorted((k, canon_value(t.kind, v)) for k, v in t.data.items())


def device_items(tab, kind):
    """items() sorted by the 128-bit key; len() and the export agree"""
    keys, values = tab.items()
    assert len(keys) == len(values) == len(tab)
    return sorted(zip(keys_of(keys), canon_array(kind, values)))


# ---- the world ---------------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, kind, data=None, slots=FIRST_SLOTS, rebuilds=0):
        self.kind, self.data, self.slots, self.rebuilds = kind, data if data is not None else {}, slots, rebuilds
        self.cap = max(len(self.data), 1024)  # create() / hbu_clone reserve max(committed, 1) rows: 1024 at least
        self.max_upsert = self.max_round = 0
        self.was_prev, self.finished = False, 0  # finished: 1 = finished or topped, 2 = changed since


class World:
    """the live objects by id, the key pool, and the counts of the conditions the sequences must reach"""

    def __init__(self, rng):
        self.tables, self.graphs, self.filters = {}, {}, {}
        self.closed = {}  # "table" / "graph" / "filter" -> the id of a closed one (the device side keeps its handle)
        self.clones = []  # [origin, clone, origin changed, clone changed, counted]
        self.ids = 0
        self.counts = collections.Counter()
        self.pool, self.wrap = make_pool(rng)

    def new_id(self):
        self.ids += 1
        return self.ids

    def of_kind(self, *kinds):
        return [i for i, t in self.tables.items() if t.kind in kinds]

    # -- what a call does to a table, counted -------------------------------------------------------------------------------------
    def room(self, t, more, where):
        """ensure_room(t, more): the index is rebuilt when 2 x (committed + more) exceeds the slots, the value array grows when
        committed + more exceeds it.  Counts an input condition; asserts nothing about the device."""
        keys = len(t.data) + more
        rebuilt = False
        if 2 * keys > t.slots:
            for home, need in ((t.slots - 1, 2), (t.slots - 2, 3)):  # (l): a key whose probe chain wrapped sits in the index that is rebuilt
                if sum(k in t.data for k in self.wrap[t.slots][home]) >= need:
                    self.counts["l"] += 1
                    break
            t.slots, t.rebuilds, rebuilt = slots_for(keys), t.rebuilds + 1, True
            self.counts[where] += 1
        if keys > t.cap:
            t.cap = max(keys, 2 * t.cap, 1024)
            self.counts["d"] += rebuilt

    def changed(self, tid):
        t = self.tables[tid]
        if t.finished == 1:
            t.finished = 2
        for c in self.clones:
            if tid in c[:2]:
                c[2 + c[:2].index(tid)] = True

    def upsert_sized(self, t, n):
        if 0 < n < t.max_round:
            self.counts["e_upsert_after_round"] += 1
        t.max_upsert = max(t.max_upsert, n)

    def round_sized(self, t, pairs):
        if 0 < pairs < t.max_upsert:
            self.counts["e_round_after_upsert"] += 1
        t.max_round = max(t.max_round, pairs)

    def roles(self, prevs, nexts):
        for i in prevs:
            self.tables[i].was_prev = True
        for i in nexts:
            if self.tables[i].was_prev:
                self.counts["g"] += 1
            self.changed(i)

    def graph_used(self, gid, step):
        used = self.graphs[gid]["steps"]
        if step not in used:
            used.add(step)
            self.counts["j"] += len(used) == 3

    def filter_roles(self, changed, new):
        if changed is not None and self.filters[changed]["state"] == 0:
            self.filters[changed]["state"] = 1
        if new is not None and self.filters[new]["state"] == 2:
            self.counts["i"] += 1
            self.filters[new]["state"] = 0

    def filter_reset(self, fid):
        if self.filters[fid]["state"] == 1:
            self.filters[fid]["state"] = 2

    def compared(self):
        """a full comparison took place"""
        for c in self.clones:
            if c[2] and c[3] and not c[4] and c[0] in self.tables and c[1] in self.tables:
                c[4] = True
                self.counts["f"] += 1


WRAP_IDS = {s: {home: keys_with_home(home, s, 3, high=h) for h, home in enumerate((s - 1, s - 2, 0))} for s in INDEX_SIZES}


def make_pool(rng):
    """~1 450 ids: random ones with small and large upper halves, pairs that share their low 64 bits, and ids whose home slot is the
    last, the last but one and the first slot of an index of 1024, 2048 and 4096 slots (three each: their probe chains wrap round)"""
    lo = rng.integers(1, 1 << 62, 1400).tolist()
    hi = np.where(rng.random(1400) < 0.5, 0, rng.integers(1, 1 << 40, 1400)).tolist()
    pool = [int(a) | (int(b) << 64) for a, b in zip(lo, hi)]
    for i in range(0, 40, 2):  # the same low half, another upper half
        pool[i + 1] = (pool[i] & M64) | (((pool[i] >> 64) + 1 + i) << 64)
    wrap = {s: dict(homes) for s, homes in WRAP_IDS.items()}
    special = [k for s in INDEX_SIZES for ids in wrap[s].values() for k in ids]
    for s in (8192, 16384, 32768):  # (larger indexes: nothing chosen, the rule of room() still reads them)
        wrap[s] = collections.defaultdict(list)
    pool = list(dict.fromkeys(pool + special))
    return pool, wrap


# ---- draws ------------------------------------------------------------------------------------------------------------------------
def pick(rng, xs):
    xs = list(xs)
    return xs[int(rng.integers(0, len(xs)))]


def draw_keys(rng, w, n, table=None, window=None):
    """n keys: one key 8, 9, wave_group_length(), + 1, 64 or 65 times (fresh or stored), the ids whose probe chains wrap, the rest from a
    window of the pool; shuffled, so that the batch order of a key's pairs is not their order in memory"""
    if not n:
        return [], None
    keys, group = [], None
    fits = [m for m in MULTIPLICITIES if m <= n]
    if fits and rng.random() < 0.7:
        m = pick(rng, fits)
        stored = table is not None and len(table.data) > 0 and rng.random() < 0.5
        hot = pick(rng, table.data) if stored else pick(rng, w.pool)
        keys += [hot] * m
        group = (hot, m)
    if rng.random() < 0.5:
        s = pick(rng, INDEX_SIZES)
        keys += [k for ids in w.wrap[s].values() for k in ids][:n - len(keys)]
    lim = window or pick(rng, [40, 300, len(w.pool)])
    keys += [w.pool[int(i)] for i in rng.integers(0, lim, n - len(keys))]
    return [keys[int(i)] for i in rng.permutation(n)], group


def draw_floats(rng, n, f32=False):
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.05:
            x = (0.0, -0.0)[int(rng.integers(0, 2))]
        elif r < 0.10:
            x = pick(rng, [1e-45, -1e-40, 3e-39] if f32 else [5e-324, -1e-310, 2e-308])
        elif r < 0.12:
            x = (float("inf"), float("-inf"))[int(rng.integers(0, 2))]
        else:
            x = float((1.0 + rng.random()) * 2.0 ** int(rng.integers(-20, 41)) * (1, -1)[int(rng.integers(0, 2))])
        out.append(np.float32(x) if f32 else x)
    return out


def draw_values(rng, kind, n):
    if kind == "HLL64":
        return list(np.where(rng.random((n, 64)) < 0.5, 0, rng.integers(0, 12, (n, 64))).astype(np.uint8))
    if kind == "DIST64":
        d = np.where(rng.random((n, 64)) < 0.05, 254, rng.integers(0, 7, (n, 64)))
        return list(np.where(rng.random((n, 64)) < 0.7, lref.NONE, d).astype(np.uint8))
    if kind == "U64":  # distance-like, some large; below 2^60, so that a distance + 1 never wraps
        return [int(x) if rng.random() < 0.85 else pick(rng, [(1 << 53) + 1, (1 << 60) - 1, int(x) << 40]) for x in rng.integers(0, 40, n).tolist()]
    if kind == "KAHAN":
        return [(x, 0.0 if rng.random() < 0.5 else float(rng.standard_normal() * 2.0 ** -55)) for x in draw_floats(rng, n)]
    return draw_floats(rng, n, kind == "F32")


def draw_edges(rng, w, m, window=None):
    if not m:
        return []
    lim = window or pick(rng, [40, 300, len(w.pool)])
    src = [w.pool[int(i)] for i in rng.integers(0, lim, m)]
    dst, _ = draw_keys(rng, w, m, window=lim)
    return list(zip(src, dst))


# ---- the operations ---------------------------------------------------------------------------------------------------------------
# Every model() returns the expected answer in canonical form; every device() the library's, in the same form.
def _table_dev(h, kind):
    from stract_amd import ampc
    return ampc.CounterTable() if kind == "HLL64" else ampc.LaneTable() if kind == "DIST64" else ampc.ValueTable(KIND_CODE[kind])


def create_table_draw(rng, w, kind=None):
    if len(w.tables) >= 14 and kind is None:
        return None
    return dict(kind=kind or pick(rng, KINDS), id=w.new_id())


def create_table_model(w, a):
    w.tables[a["id"]] = Table(a["kind"])
    return 0


def create_table_device(h, a):
    h.tables[a["id"]] = _table_dev(h, a["kind"])
    return len(h.tables[a["id"]])


def close_table_draw(rng, w, tid=None):
    if tid is None:
        many = [i for i, t in w.tables.items() if len(w.of_kind(t.kind)) > 2]
        if not many:
            return None
        tid = pick(rng, many)
    return dict(t=tid)


def close_table_model(w, a):
    del w.tables[a["t"]]
    w.closed["table"] = a["t"]


def close_table_device(h, a):
    h.closed["table"] = h.tables.pop(a["t"])
    h.closed["table"].close()


def batch_write_draw(rng, w):
    tid = pick(rng, w.tables)
    t = w.tables[tid]
    lane = t.kind == "DIST64"
    sizes = [s for s, k in zip(SIZES, SIZE_WEIGHTS) for _ in range(k) if not lane or s <= 257]
    n = pick(rng, sizes)
    keys, group = draw_keys(rng, w, n, t, 300 if lane else None)
    return dict(t=tid, op=pick(rng, OPS_OF[t.kind] + [None]), keys=keys, values=draw_values(rng, t.kind, n), group=group)


def batch_write_model(w, a):
    t = w.tables[a["t"]]
    n = len(a["keys"])
    if n:
        if a["group"] and a["group"][1] >= WAVE_GROUP and t.rebuilds:
            w.counts["k_stored" if a["group"][0] in t.data else "k_fresh"] += 1
        w.room(t, n, "a")
        w.upsert_sized(t, n)
        w.changed(a["t"])
    if a["op"] is None:
        ref.batch_set(t.data, a["keys"], a["values"])
        return None
    if t.kind == "DIST64":
        return lref.batch_upsert(t.data, a["keys"], a["values"])
    return ref.batch_upsert(t.data, a["op"], a["keys"], a["values"])


def batch_write_device(h, a):
    tab, kind = h.tables[a["t"]], h.kinds[a["t"]]
    keys, values = u128(a["keys"]), device_values(kind, a["values"])
    if a["op"] is None:
        tab.batch_set(keys, values)
        return None
    acts = tab.batch_upsert(keys, values) if kind in ("HLL64", "DIST64") else tab.batch_upsert(a["op"], keys, values)
    return acts.tolist()


def batch_get_draw(rng, w):
    tid = pick(rng, w.tables)
    return dict(t=tid, keys=draw_keys(rng, w, pick(rng, SIZES), w.tables[tid])[0])


def batch_get_model(w, a):
    t = w.tables[a["t"]]
    return [canon_value(t.kind, t.data.get(k, default_of(t.kind))) for k in a["keys"]], [k in t.data for k in a["keys"]]


def batch_get_device(h, a):
    got, found = h.tables[a["t"]].batch_get(u128(a["keys"]))
    return canon_array(h.kinds[a["t"]], got), found.tolist()


def items_draw(rng, w):
    return dict(t=pick(rng, w.tables))


def items_model(w, a):
    return model_items(w.tables[a["t"]])


def items_device(h, a):
    return device_items(h.tables[a["t"]], h.kinds[a["t"]])


def clone_draw(rng, w):
    if len(w.tables) >= 16:
        return None
    return dict(t=pick(rng, w.tables), id=w.new_id())


def clone_model(w, a):
    t = w.tables[a["t"]]
    data = ref.clone_table(t.data)
    w.tables[a["id"]] = Table(t.kind, data, t.slots, t.rebuilds)
    w.clones.append([a["t"], a["id"], False, False, False])
    return len(data)


def clone_device(h, a):
    h.tables[a["id"]] = h.tables[a["t"]].clone()
    h.kinds[a["id"]] = h.kinds[a["t"]]
    return len(h.tables[a["id"]])


def two_of(rng, w, kind):
    ids = w.of_kind(kind)
    if len(ids) < 2:
        return None
    a = pick(rng, ids)
    return a, pick(rng, [i for i in ids if i != a])


def update_counters_draw(rng, w):
    pair = two_of(rng, w, "HLL64")
    return pair and dict(prev=pair[0], next=pair[1], edges=draw_edges(rng, w, pick(rng, SIZES)))


def update_counters_model(w, a):
    prev, nxt = w.tables[a["prev"]], w.tables[a["next"]]
    if a["edges"]:
        w.room(nxt, len(a["edges"]), "step")
        w.round_sized(nxt, len(a["edges"]))
    w.roles([a["prev"]], [a["next"]])
    return ref.update_counters(prev.data, nxt.data, a["edges"])[1]


def update_counters_device(h, a):
    from stract_amd import ampc
    return ampc.update_counters(h.tables[a["prev"]], h.tables[a["next"]], u128([f for f, _ in a["edges"]]), u128([t for _, t in a["edges"]])).tolist()


def update_distances_draw(rng, w):
    pair = two_of(rng, w, "U64")
    return pair and dict(prev=pair[0], next=pair[1], edges=draw_edges(rng, w, pick(rng, SIZES)))


def update_distances_model(w, a):
    prev, nxt = w.tables[a["prev"]], w.tables[a["next"]]
    pairs = sum(f in prev.data for f, _ in a["edges"])
    if pairs:
        w.room(nxt, pairs, "step")
        w.round_sized(nxt, pairs)
    w.roles([a["prev"]], [a["next"]])
    keys, actions = ref.update_distances(prev.data, nxt.data, a["edges"])
    return sorted(zip(keys, actions))  # (one entry per destination, in no particular order)


def update_distances_device(h, a):
    from stract_amd import ampc
    keys, actions = ampc.update_distances(h.tables[a["prev"]], h.tables[a["next"]], u128([f for f, _ in a["edges"]]), u128([t for _, t in a["edges"]]))
    return sorted(zip(keys_of(keys), actions.tolist()))


def four_tables(rng, w):
    c, v = two_of(rng, w, "HLL64"), two_of(rng, w, "KAHAN")
    return None if c is None or v is None else dict(prev_c=c[0], next_c=c[1], prev_v=v[0], next_v=v[1])


def update_centralities_draw(rng, w):
    a = four_tables(rng, w)
    if a is None:
        return None
    held = list(w.tables[a["next_c"]].data)  # mostly nodes that next_counters holds
    n = pick(rng, SIZES)
    nodes = [pick(rng, held) if held and rng.random() < 0.8 else pick(rng, w.pool) for _ in range(n)]
    return dict(a, nodes=nodes, round=pick(rng, [0, 1, 6, 1 << 53]))


def update_centralities_model(w, a):
    t = {k: w.tables[a[k]].data for k in ("prev_c", "next_c", "prev_v", "next_v")}
    before = len(t["next_v"])
    want = w.tables[a["next_v"]]
    probe = dict(want.data)
    written = ref.update_centralities(t["prev_c"], t["next_c"], t["prev_v"], probe, a["nodes"], a["round"])
    if written:  # (room for the pairs before the keys go in: the count of distinct nodes written stands for the pairs)
        w.room(want, written, "step")
        w.round_sized(want, written)
    want.data.clear()
    want.data.update(probe)
    assert len(want.data) >= before
    w.roles([a["prev_c"], a["next_c"], a["prev_v"]], [a["next_v"]])
    return written


def update_centralities_device(h, a):
    from stract_amd import ampc
    return ampc.update_centralities(*(h.tables[a[k]] for k in ("prev_c", "next_c", "prev_v", "next_v")), u128(a["nodes"]), a["round"])


def fold_draw(rng, w):
    src, dst = w.of_kind("U64", "DIST64"), w.of_kind("KAHAN")
    if not src or not dst:
        return None
    s = pick(rng, src)
    return dict(src=s, dst=pick(rng, dst), norm=pick(rng, NORMS), skip_zero=bool(rng.random() < 0.5), n_lanes=pick(rng, [1, 2, 63, 64]) if w.tables[s].kind == "DIST64" else 0)


def fold_model(w, a):
    src, dst = w.tables[a["src"]], w.tables[a["dst"]]
    if src.data:
        w.room(dst, len(src.data), "b")
        w.round_sized(dst, len(src.data))
    w.roles([a["src"]], [a["dst"]])
    if a["n_lanes"]:
        return lref.fold_lanes(dst.data, src.data, a["norm"], a["n_lanes"], a["skip_zero"])
    return aref.fold(dst.data, src.data, a["norm"], a["skip_zero"])


def fold_device(h, a):
    from stract_amd import ampc
    if a["n_lanes"]:
        return ampc.fold_harmonic_lanes(h.tables[a["src"]], h.tables[a["dst"]], a["norm"], a["n_lanes"], a["skip_zero"])
    return ampc.fold_harmonic(h.tables[a["src"]], h.tables[a["dst"]], a["norm"], a["skip_zero"])


def value_of(kind, v):
    return v[0] if kind == "KAHAN" else v  # f64::from(KahanSum)


def finish_draw(rng, w):
    """a KahanSum or f64 table without a NaN (and without an inf where the divisor makes one): the sign of a NaN an addition made is the
    device's own, and f64::total_cmp ranks by it"""
    ok = [i for i in w.of_kind("KAHAN", "F64") if all(value_of(w.tables[i].kind, v) == value_of(w.tables[i].kind, v) for v in w.tables[i].data.values())]
    if not ok:
        return None
    tid = pick(rng, ok)
    n = len(w.tables[tid].data)
    return dict(t=tid, divisor=pick(rng, DIVISORS), k=pick(rng, [None, None, 0, 1, 10, n, n + 5]))


def finish_model(w, a):
    t = w.tables[a["t"]]
    if t.finished == 2:
        w.counts["h"] += 1
    t.finished = 1
    ids, vals, ranks = fref.finish({k: value_of(t.kind, v) for k, v in t.data.items()}, a["divisor"])
    if a["k"] is None:
        answer = (ids, [aref.bits(float(v)) for v in vals], ranks)
    else:
        top = fref.top(ids, vals, a["k"])
        answer = ([k for k, _ in top], [aref.bits(float(v)) for _, v in top])
    return answer, model_items(t)


def finish_device(h, a):
    tab = h.tables[a["t"]]
    if a["k"] is None:
        ids, vals, ranks = tab.finish_centralities(a["divisor"])
        answer = (keys_of(ids), canon_array("F64", vals), [int(r) for r in ranks.tolist()])
    else:
        ids, vals = tab.top_centralities(a["k"], a["divisor"])
        answer = (keys_of(ids), canon_array("F64", vals))
    return answer, device_items(tab, h.kinds[a["t"]])  # the table is only read


def create_graph_draw(rng, w):
    if len(w.graphs) >= 5:
        return None
    window = pick(rng, [40, 300, len(w.pool)])
    nodes = [w.pool[int(i)] for i in rng.integers(0, window, pick(rng, [0, 1, 17, 65, 300]))]
    return dict(id=w.new_id(), nodes=nodes, edges=draw_edges(rng, w, pick(rng, [0, 1, 65, 257, 1000, 2500]), window), chunk=pick(rng, CHUNKS))


def create_graph_model(w, a):
    w.graphs[a["id"]] = dict(nodes=a["nodes"], edges=a["edges"], chunk=a["chunk"], steps=set())
    return len(a["edges"])


def create_graph_device(h, a):
    from stract_amd import ampc
    h.graphs[a["id"]] = ampc.WorkerGraph(u128(a["nodes"]), u128([f for f, _ in a["edges"]]), u128([t for _, t in a["edges"]]), chunk_edges=a["chunk"])
    return len(h.graphs[a["id"]])


def close_graph_draw(rng, w):
    return dict(g=pick(rng, w.graphs)) if len(w.graphs) > 2 else None


def close_graph_model(w, a):
    del w.graphs[a["g"]]
    w.closed["graph"] = a["g"]


def close_graph_device(h, a):
    h.closed["graph"] = h.graphs.pop(a["g"])
    h.closed["graph"].close()


def node_sketch_draw(rng, w):
    return dict(g=pick(rng, w.graphs)) if w.graphs else None


def node_sketch_model(w, a):
    return aref.sketch(w.graphs[a["g"]]["nodes"]).tolist()


def node_sketch_device(h, a):
    return h.graphs[a["g"]].node_sketch().tolist()


def create_filter_draw(rng, w):
    if len(w.filters) >= 8:
        return None
    return dict(id=w.new_id(), bits=pick(rng, BLOOM_BITS + [0, 0]))  # 0: an exact set


def create_filter_model(w, a):
    w.filters[a["id"]] = dict(m=rref.Bloom(a["bits"]) if a["bits"] else rref.Exact(), state=0)
    return 0


def create_filter_device(h, a):
    from stract_amd import ampc
    h.filters[a["id"]] = ampc.ChangedFilter.bloom(a["bits"]) if a["bits"] else ampc.ChangedFilter.exact()
    return h.filters[a["id"]].count()


def close_filter_draw(rng, w):
    many = [i for i, f in w.filters.items() if sum(g["m"].kind == f["m"].kind for g in w.filters.values()) > 2]
    return dict(f=pick(rng, many)) if many else None


def close_filter_model(w, a):
    del w.filters[a["f"]]
    w.closed["filter"] = a["f"]


def close_filter_device(h, a):
    h.closed["filter"] = h.filters.pop(a["f"])
    h.closed["filter"].close()


def filter_ids_draw(rng, w):
    if not w.filters:
        return None
    return dict(f=pick(rng, w.filters), ids=draw_keys(rng, w, pick(rng, SIZES))[0], what=pick(rng, ["insert", "contains", "contains"]))


def filter_ids_model(w, a):
    m = w.filters[a["f"]]["m"]
    if a["what"] == "contains":
        return [m.contains(k) for k in a["ids"]]
    for k in a["ids"]:
        m.insert(k)
    return m.count()


def filter_ids_device(h, a):
    f = h.filters[a["f"]]
    if a["what"] == "contains":
        return f.contains(u128(a["ids"])).tolist()
    f.insert(u128(a["ids"]))
    return f.count()


def filter_whole_draw(rng, w):
    if not w.filters:
        return None
    fid = pick(rng, w.filters)
    m = w.filters[fid]["m"]
    same = [i for i, g in w.filters.items() if i != fid and g["m"].kind == m.kind and getattr(g["m"], "num_bits", 0) == getattr(m, "num_bits", 0)]
    what = pick(rng, ["clear", "clear", "count", "export"] + (["fill"] if m.kind == "sketch" else []) + (["union", "union", "union"] + (["copy_bits"] if m.kind == "sketch" else []) if same else []))
    return dict(f=fid, what=what, other=pick(rng, same) if what in ("union", "copy_bits") else None)


def filter_content(m):
    return [int(x) for x in m.words().tolist()] if m.kind == "sketch" else sorted(m.ids)


def filter_whole_model(w, a):
    m = w.filters[a["f"]]["m"]
    if a["what"] == "clear":
        if m.kind == "sketch":
            m.ones = set()
        else:
            m.ids = set()
        w.filter_reset(a["f"])
    elif a["what"] == "fill":
        m.fill()
    elif a["what"] == "union":
        other = w.filters[a["other"]]["m"]
        if m.kind == "sketch":
            m.union(other)
        else:
            m.ids |= other.ids
        w.filter_reset(a["f"])
    elif a["what"] == "copy_bits":  # export_bits of `other`, import_bits into this one
        m.ones = set(w.filters[a["other"]]["m"].ones)
    return m.count(), filter_content(m) if a["what"] in ("export", "copy_bits") else None


def device_filter_content(f):
    from stract_amd import ampc
    if f.kind == ampc.FILTER_BLOOM:
        return [int(x) for x in f.export_bits().tolist()]
    ids = keys_of(f.export_ids())
    assert len(ids) == len(set(ids)), "an id twice in an exact set"
    return sorted(ids)


def filter_whole_device(h, a):
    f = h.filters[a["f"]]
    if a["what"] == "clear":
        f.clear()
    elif a["what"] == "fill":
        f.fill()
    elif a["what"] == "union":
        f.union(h.filters[a["other"]])
    elif a["what"] == "copy_bits":
        f.import_bits(h.filters[a["other"]].export_bits())
    return f.count(), device_filter_content(f) if a["what"] in ("export", "copy_bits") else None


ROUND_STEPS = {"setup_counters": "HLL64", "round_counters": "HLL64", "round_distances": "U64", "round_lane_distances": "DIST64", "round_centralities": "KAHAN"}


def round_draw(rng, w, step=None):
    step = step or pick(rng, ROUND_STEPS)
    if not w.graphs or not w.filters:
        return None
    if step == "round_centralities":
        a = four_tables(rng, w)
    else:
        pair = two_of(rng, w, ROUND_STEPS[step])
        a = pair and dict(prev=pair[0], next=pair[1])
    if a is None:
        return None
    changed = pick(rng, w.filters)
    others = [i for i in w.filters if i != changed]
    new = pick(rng, others) if others and step in ("round_counters", "round_distances", "round_lane_distances") and rng.random() < 0.6 else None
    if step == "setup_counters" and rng.random() < 0.4:
        changed = None
    return dict(a, step=step, g=pick(rng, w.graphs), changed=changed, new=new, round=pick(rng, [0, 1, 6]))


def round_model(w, a):
    g, step = w.graphs[a["g"]], a["step"]
    changed = w.filters[a["changed"]]["m"] if a["changed"] is not None else None
    new = w.filters[a["new"]]["m"] if a["new"] is not None else None
    w.graph_used(a["g"], step)
    w.filter_roles(a["changed"] if step != "setup_counters" else None, a["new"])
    total = [0, 0, 0]

    def add(counts):
        for i, c in enumerate(counts):
            total[i] += c

    def sized(t, pairs):
        if pairs:
            w.room(t, pairs, "c")
            w.round_sized(t, pairs)
    if step == "round_centralities":
        t = {k: w.tables[a[k]] for k in ("prev_c", "next_c", "prev_v", "next_v")}
        for part in rref.chunks(g["nodes"], g["chunk"]):
            probe = dict(t["next_v"].data)
            s, written = rref.round_centralities(t["prev_c"].data, t["next_c"].data, t["prev_v"].data, probe, part, changed, a["round"])
            sized(t["next_v"], written)
            t["next_v"].data.clear()
            t["next_v"].data.update(probe)
            add((s, written))
        w.roles([a["prev_c"], a["next_c"], a["prev_v"]], [a["next_v"]])
        return tuple(total[:2])
    prev, nxt = w.tables[a["prev"]], w.tables[a["next"]]
    if step == "setup_counters":  # writes BOTH tables
        for part in rref.chunks(g["nodes"], g["chunk"]):
            sized(prev, len(part))
            sized(nxt, len(part))
            rref.setup_counters(prev.data, nxt.data, part, changed)
        w.roles([], [a["prev"], a["next"]])
        return None
    for part in rref.chunks(g["edges"], g["chunk"]):
        if step == "round_counters":
            sized(nxt, sum(changed.contains(f) for f, _ in part))
            add(rref.round_counters(prev.data, nxt.data, part, changed, new))
        elif step == "round_distances":
            sized(nxt, sum(changed.contains(f) and f in prev.data for f, _ in part))
            add(rref.round_distances(prev.data, nxt.data, part, changed, new))
        else:
            sized(nxt, sum(changed.contains(f) and f in prev.data for f, _ in part))
            add(lref.round_lane_distances(prev.data, nxt.data, part, changed, new))
    w.roles([a["prev"]], [a["next"]])
    return tuple(total[:2]) if step == "round_distances" else tuple(total)


def round_device(h, a):
    from stract_amd import ampc
    g, step = h.graphs[a["g"]], a["step"]
    changed = h.filters[a["changed"]] if a["changed"] is not None else None
    new = h.filters[a["new"]] if a["new"] is not None else None
    if step == "round_centralities":
        return ampc.round_centralities(*(h.tables[a[k]] for k in ("prev_c", "next_c", "prev_v", "next_v")), g, changed, a["round"])
    prev, nxt = h.tables[a["prev"]], h.tables[a["next"]]
    if step == "setup_counters":
        return ampc.setup_counters(prev, nxt, g, changed)
    return getattr(ampc, step)(prev, nxt, g, changed, new)


REFUSALS = ["wrong_op", "kind_mismatch", "prev_is_next", "changed_is_new_changed", "closed_table", "closed_prev", "closed_graph", "closed_filter", "union_mismatch",
            "finish_of_another_kind"]


def refusal_draw(rng, w):
    """a call the library must refuse (the lists of tests/test_ampc_values.py, test_ampc_edges.py, test_ampc_round.py, test_ampc_lanes.py,
    test_ampc_approx.py and test_ampc_finish.py), drawn until one fits the world"""
    for _ in range(8):
        what = pick(rng, REFUSALS)
        a = dict(what=what)
        if what == "wrong_op":
            a["t"] = pick(rng, w.of_kind("U64", "F32", "F64", "KAHAN", "DIST64"))
            kind = w.tables[a["t"]].kind
            a["op"] = pick(rng, [o for k in KINDS for o in OPS_OF[k] if o not in OPS_OF[kind]])
            a["keys"] = draw_keys(rng, w, 17, w.tables[a["t"]])[0]
            a["values"] = draw_values(rng, kind, 17)
        elif what == "kind_mismatch":
            a["call"] = pick(rng, ["update_counters", "update_distances", "fold_harmonic", "round_distances"])
            want = {"update_counters": "HLL64", "update_distances": "U64", "fold_harmonic": "U64", "round_distances": "U64"}[a["call"]]
            right, wrong = w.of_kind(want), [i for i, t in w.tables.items() if t.kind not in (want, "KAHAN")]
            if not right or not wrong or (a["call"] == "fold_harmonic" and not w.of_kind("KAHAN")):
                continue
            a["prev"], a["next"] = (pick(rng, wrong), pick(rng, right)) if rng.random() < 0.5 or a["call"] == "fold_harmonic" else (pick(rng, right), pick(rng, wrong))
            if a["call"] == "fold_harmonic":
                a["next"] = pick(rng, w.of_kind("KAHAN"))
                if w.tables[a["prev"]].kind == "DIST64":
                    continue
            if a["call"] == "round_distances":
                if not w.graphs or not w.filters:
                    continue
                a["g"], a["changed"] = pick(rng, w.graphs), pick(rng, w.filters)
            a["edges"] = draw_edges(rng, w, 17)
        elif what in ("prev_is_next", "changed_is_new_changed", "closed_prev", "closed_graph", "closed_filter"):
            a["call"] = pick(rng, ["update_counters", "update_distances"] if what == "prev_is_next" and rng.random() < 0.4 else ["round_counters", "round_distances", "round_lane_distances"])
            pair = two_of(rng, w, {"update_counters": "HLL64", "update_distances": "U64"}.get(a["call"]) or ROUND_STEPS[a["call"]])
            needs = {"closed_prev": "table", "closed_graph": "graph", "closed_filter": "filter"}.get(what)
            if pair is None or len(w.filters) < 2 or not w.graphs or (needs and needs not in w.closed):
                continue
            a["prev"], a["next"] = pair
            a["edges"], a["g"] = draw_edges(rng, w, 17), pick(rng, w.graphs)
            a["changed"] = pick(rng, w.filters)
            a["new"] = pick(rng, [i for i in w.filters if i != a["changed"]])
        elif what == "closed_table":
            if "table" not in w.closed:
                continue
            a["keys"] = draw_keys(rng, w, 17)[0]
        elif what == "union_mismatch":
            fid = pick(rng, w.filters)
            m = w.filters[fid]["m"]
            other = [i for i, g in w.filters.items() if g["m"].kind != m.kind or getattr(g["m"], "num_bits", 0) != getattr(m, "num_bits", 0)]
            if not other:
                continue
            a["f"], a["other"] = fid, pick(rng, other)
        else:
            a["t"] = pick(rng, w.of_kind("HLL64", "U64", "F32", "DIST64"))
            a["k"] = pick(rng, [None, 3])
        return a
    return None


def refusal_model(w, a):
    w.counts["m"] += 1
    return "refused"


def refusal_device(h, a):
    from stract_amd import _lib, ampc
    what = a["what"]

    def call():
        if what == "wrong_op":
            tab, kind = h.tables[a["t"]], h.kinds[a["t"]]
            if kind == "DIST64":
                return tab.batch_upsert(u128(a["keys"]), device_values(kind, a["values"]), op=a["op"])
            return tab.batch_upsert(a["op"], u128(a["keys"]), device_values(kind, a["values"]))
        if what == "closed_table":
            return h.closed["table"].batch_get(u128(a["keys"]))
        if what == "union_mismatch":
            return h.filters[a["f"]].union(h.filters[a["other"]])
        if what == "finish_of_another_kind":
            tab = h.tables[a["t"]]
            return ampc.finish_centralities(tab, 1.0) if a["k"] is None else ampc.top_centralities(tab, a["k"], 1.0)
        prev, nxt = h.tables[a["prev"]], h.tables[a["next"]]
        g, changed, new = h.graphs.get(a.get("g")), h.filters.get(a.get("changed")), h.filters.get(a.get("new"))
        if what == "prev_is_next":
            prev = nxt
        elif what == "changed_is_new_changed":
            new = changed
        elif what == "closed_prev":
            prev = h.closed["table"]
        elif what == "closed_graph":
            g = h.closed["graph"]
        elif what == "closed_filter":
            changed = h.closed["filter"]
        if a["call"] in ("update_counters", "update_distances"):
            return getattr(ampc, a["call"])(prev, nxt, u128([f for f, _ in a["edges"]]), u128([t for _, t in a["edges"]]))
        if a["call"] == "fold_harmonic":
            return ampc.fold_harmonic(prev, nxt, 0.5)
        return getattr(ampc, a["call"])(prev, nxt, g, changed, new)
    try:
        call()
    except _lib.HyperballError as e:
        assert e.code in (_lib.HB_ERR_INVALID, _lib.HB_ERR_LIMIT), e
        return "refused"
    return "accepted"


def same(got, want):
    """the comparison of every operation: both answers are canonical forms (integers, lists, bytes, bit patterns), so it is =="""
    assert got == want, "the library's answer differs from the model's"


Op = collections.namedtuple("Op", "name weight draw model device compare", defaults=(same,))
OPERATIONS = [
    Op("create_table", 2, create_table_draw, create_table_model, create_table_device),
    Op("close_table", 1, close_table_draw, close_table_model, close_table_device),
    Op("batch_write", 22, batch_write_draw, batch_write_model, batch_write_device),  # batch_set, batch_upsert with every operator of the kind
    Op("batch_get", 6, batch_get_draw, batch_get_model, batch_get_device),
    Op("items", 3, items_draw, items_model, items_device),
    Op("clone", 5, clone_draw, clone_model, clone_device),
    Op("update_counters", 4, update_counters_draw, update_counters_model, update_counters_device),
    Op("update_distances", 4, update_distances_draw, update_distances_model, update_distances_device),
    Op("update_centralities", 4, update_centralities_draw, update_centralities_model, update_centralities_device),
    Op("fold", 8, fold_draw, fold_model, fold_device),  # fold_harmonic, fold_harmonic_lanes
    Op("finish", 7, finish_draw, finish_model, finish_device),  # finish_centralities, top_centralities
    Op("create_graph", 2, create_graph_draw, create_graph_model, create_graph_device),
    Op("close_graph", 1, close_graph_draw, close_graph_model, close_graph_device),
    Op("node_sketch", 1, node_sketch_draw, node_sketch_model, node_sketch_device),
    Op("create_filter", 2, create_filter_draw, create_filter_model, create_filter_device),
    Op("close_filter", 1, close_filter_draw, close_filter_model, close_filter_device),
    Op("filter_ids", 6, filter_ids_draw, filter_ids_model, filter_ids_device),  # insert, contains
    Op("filter_whole", 8, filter_whole_draw, filter_whole_model, filter_whole_device),  # clear, fill, union, count, export_* / import_bits
    Op("round", 24, round_draw, round_model, round_device),  # setup_counters and the four round steps
    Op("refusal", 8, refusal_draw, refusal_model, refusal_device),
]
BY_NAME = {op.name: op for op in OPERATIONS}
WEIGHTS = np.array([op.weight for op in OPERATIONS], dtype=np.float64) / sum(op.weight for op in OPERATIONS)


class Handles:
    """the device side of a world: the library's objects under the model's ids"""

    def __init__(self):
        self.tables, self.graphs, self.filters, self.closed, self.kinds = {}, {}, {}, {}, {}

    def close(self):
        for x in list(self.tables.values()) + list(self.graphs.values()) + list(self.filters.values()):
            x.close()


def compare_all(w, h):
    """the whole content of every live table, as items() sorted by the 128-bit key, and every filter, as its words or its ids and its count"""
    if h is not None:
        for tid, t in w.tables.items():
            assert device_items(h.tables[tid], t.kind) == model_items(t), ("table", tid, t.kind)
        for fid, f in w.filters.items():
            assert h.filters[fid].count() == f["m"].count(), ("count of filter", fid)
            assert device_filter_content(h.filters[fid]) == filter_content(f["m"]), ("filter", fid)
        for gid, g in w.graphs.items():
            assert len(h.graphs[gid]) == len(g["edges"]), ("graph", gid)
    w.compared()


def summary(name, a):
    """an operation as it is printed: the arguments without the long lists"""
    return [name, {k: (len(v) if isinstance(v, list) else v) for k, v in (a or {}).items() if k != "values"}]


PROLOGUE = [("create_table", k) for k in ("HLL64", "HLL64", "U64", "U64", "KAHAN", "KAHAN", "DIST64", "DIST64", "F32", "F64")]


def run(seed, handles=None, n_ops=N_OPS, log=None):
    """One sequence.  handles: a Handles to make every call on the library too and compare (None: the model alone).  Returns the world
    with its counts; a failure raises AssertionError with the seed, the operation index and the operations so far."""
    rng = np.random.default_rng(seed)
    w = World(rng)
    h = handles
    log = log if log is not None else []

    def one(op, a):
        if h is not None and op.name in ("create_table",):
            h.kinds[a["id"]] = a["kind"]
        log.append(summary(op.name, a))
        try:
            want = op.model(w, a)
            if h is not None:
                op.compare(op.device(h, a), want)
            if op.name == "refusal":
                compare_all(w, h)
        except Exception as e:  # noqa: BLE001  (whatever it is, it is reported with the way to it)
            raise AssertionError(json.dumps(dict(seed=seed, operation=len(log) - 1, failed=repr(e)[:600], operations=log), default=str)) from e

    def compare_now():
        try:
            compare_all(w, h)
        except Exception as e:  # noqa: BLE001
            raise AssertionError(json.dumps(dict(seed=seed, operation=len(log) - 1, failed="full comparison: " + repr(e)[:600], operations=log), default=str)) from e

    for name, kind in PROLOGUE:
        one(BY_NAME[name], create_table_draw(rng, w, kind))
    for name in ("create_graph", "create_graph", "create_filter", "create_filter", "create_filter", "create_filter"):
        one(BY_NAME[name], BY_NAME[name].draw(rng, w))
    drawn = dropped = refused = 0
    while drawn < n_ops:
        # upkeep, read from the world alone: a table that grew too large is closed, a kind with fewer than two tables gets one
        big = [i for i, t in w.tables.items() if len(t.data) > (MAX_LANE_KEYS if t.kind == "DIST64" else MAX_KEYS)]
        short = [k for k in ("HLL64", "U64", "KAHAN", "DIST64") if len(w.of_kind(k)) < 2]
        if big:
            one(BY_NAME["close_table"], close_table_draw(rng, w, big[0]))
            continue
        if short:
            one(BY_NAME["create_table"], create_table_draw(rng, w, short[0]))
            continue
        op = OPERATIONS[int(rng.choice(len(OPERATIONS), p=WEIGHTS))]
        a = op.draw(rng, w)
        drawn += 1
        if a is None:
            dropped += 1
            continue
        refused += op.name == "refusal"
        one(op, a)
        if drawn % COMPARE_EVERY == 0:
            compare_now()
    compare_now()
    w.counts["operations"], w.counts["dropped"], w.counts["refused"] = drawn, dropped, refused
    w.counts["largest_table"] = max([len(t.data) for t in w.tables.values()] + [0])
    return w


def totals(worlds):
    total = collections.Counter()
    for w in worlds:
        total.update({k: v for k, v in w.counts.items() if k != "largest_table"})
    return total


def unmet(worlds):
    """the conditions of NEED the seed list misses, and the sequences that break a cap"""
    total = totals(worlds)
    bad = ["%s: %d < %d" % (k, total[k], n) for k, n in NEED.items() if total[k] < n]
    for w in worlds:
        c = w.counts
        if c["dropped"] >= MAX_DROPPED * c["operations"]:
            bad.append("dropped %d of %d" % (c["dropped"], c["operations"]))
        if c["refused"] >= MAX_REFUSED * c["operations"]:
            bad.append("refused %d of %d" % (c["refused"], c["operations"]))
    return bad


def main():
    ap = argparse.ArgumentParser(description="the counts (a) .. (m) of a seed list, from the model alone")
    ap.add_argument("--seeds", type=int, nargs="+", required=True)
    ap.add_argument("--ops", type=int, default=N_OPS)
    a = ap.parse_args()
    worlds = [run(s, None, a.ops) for s in a.seeds]
    for s, w in zip(a.seeds, worlds):
        print(json.dumps(dict(seed=s, **{k: w.counts[k] for k in list(NEED) + ["step", "operations", "dropped", "refused", "largest_table"]})))
    print(json.dumps(dict(total={k: totals(worlds)[k] for k in NEED}, need=NEED, unmet=unmet(worlds))))
    assert "stract_amd._lib" not in sys.modules, "the model alone loads no library"
    sys.exit(1 if unmet(worlds) else 0)


if __name__ == "__main__":
    main()
