"""The AMPC table store restated for the tests: what include/hb_ampc.h must compute, written from the reference's semantics
(dht/store.rs:159-195 batch_set / batch_get / batch_upsert / clone_table, dht/upsert.rs:67-152 the operators, kahan_sum.rs:47-54,
harmonic_centrality/mapper.rs:91-209 update_counters / update_centralities, shortest_path/mapper.rs:57-88 update_distances).  A table
is a dict key -> value; keys are Python ints (the NodeID as u128).  Values: u64 = int below 2^64, f32 = numpy.float32, f64 = float,
KahanSum = (sum, err) of floats, HyperLogLog<64> = numpy uint8[64].  `!=` on floats is the IEEE comparison, as Rust's derived PartialEq
is: NaN != NaN, -0.0 == +0.0.  HyperLogLog sizes and insertions come from the CPU oracle (oracle.hbo)."""
import numpy as np

from oracle import hbo

NO_CHANGE, MERGED, INSERTED = 0, 1, 2
HLL64, U64_ADD, U64_MIN, F32_ADD, F64_ADD, KAHAN_ADD = range(6)
M64 = (1 << 64) - 1
KAHAN_DEFAULT = (0.0, 0.0)


def kahan_add(k, rhs):
    """KahanSum += f64, kahan_sum.rs:47-54"""
    s, e = k
    y = rhs - e
    t = s + y
    return (t, (t - s) - y)


def _f32_add(old, new):
    with np.errstate(all="ignore"):
        return np.float32(old) + np.float32(new)


def _f64_add(old, new):
    with np.errstate(all="ignore"):
        return float(np.float64(old) + np.float64(new))  # (numpy: inf + -inf is NaN, not an exception)


# op -> (merge(old, new), changed(merged, old))
OPS = {
    HLL64: (lambda old, new: np.maximum(old, new), lambda m, old: not np.array_equal(m, old)),  # hyperloglog.rs:4531-4535
    U64_ADD: (lambda old, new: (old + new) & M64, lambda m, old: m != old),  # wraps (the reference: panics in a debug build)
    U64_MIN: (lambda old, new: min(old, new), lambda m, old: m != old),
    F32_ADD: (_f32_add, lambda m, old: bool(m != old)),
    F64_ADD: (_f64_add, lambda m, old: m != old),
    KAHAN_ADD: (lambda old, new: kahan_add(old, new[0]), lambda m, old: m[0] != old[0] or m[1] != old[1]),  # new.err ignored, upsert.rs:143-151
}


def batch_set(table, keys, values):
    for k, v in zip(keys, values):
        table[k] = v


def batch_get(table, keys):
    """the stored value, or None for an absent key"""
    return [table.get(k) for k in keys]


def batch_upsert(table, op, keys, values):
    """the pairs in order (store.rs:159-190); returns the action of every pair"""
    merge, changed = OPS[op]
    actions = []
    for k, v in zip(keys, values):
        old = table.get(k)
        if old is None:
            table[k] = v
            actions.append(INSERTED)
        else:
            m = merge(old, v)
            actions.append(MERGED if changed(m, old) else NO_CHANGE)
            table[k] = m
    return actions


def clone_table(table):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in table.items()}


def hll_of(node):
    """HyperLogLog::default() + add_u128(node)"""
    reg = np.zeros(64, dtype=np.uint8)
    hbo.hll_add(reg, node)
    return reg


def update_counters(prev_counters, next_counters, edges):
    """mapper.rs:91-118 for a batch of (from, to): the old counter of `from` (or the default), plus `from` itself, is upserted into
    `to` of the next table.  Returns (keys, actions)."""
    keys, values = [], []
    for f, t in edges:
        old = prev_counters.get(f)
        counter = np.zeros(64, dtype=np.uint8) if old is None else old.copy()
        hbo.hll_add(counter, f)
        keys.append(t)
        values.append(counter)
    return keys, batch_upsert(next_counters, HLL64, keys, values)


def update_centralities(prev_counters, next_counters, prev_centrality, next_centrality, nodes, round_):
    """mapper.rs:157-209; returns the number of distinct nodes set"""
    nodes = list(nodes)
    present = sorted({n for n in nodes if n in prev_counters and n in next_counters})
    if not present:
        return 0
    old_sizes = hbo.hll_sizes(np.stack([prev_counters[n] for n in present]))
    new_sizes = hbo.hll_sizes(np.stack([next_counters[n] for n in present]))
    new_values = {}
    for n, old_size, new_size in zip(present, old_sizes, new_sizes):
        d = max(int(new_size) - int(old_size), 0)  # saturating_sub
        if d == 0:
            continue
        new_values[n] = kahan_add(prev_centrality.get(n, KAHAN_DEFAULT), float(d) / float((round_ + 1) & M64))
    batch_set(next_centrality, new_values.keys(), new_values.values())
    return len(new_values)


def new_distances(old_distances, edges):
    """shortest_path/mapper.rs:66-81: destination -> the smallest old distance of a source + 1 over the batch's edges (from, to);
    old_distances: the batch_get of the sources as a dict (absent = no distance yet: the edge is skipped).  Keys in the order of
    first appearance (the reference's is a hash map's: every key occurs once, so the order does not matter)."""
    new = {}
    for f, t in edges:
        old = old_distances.get(f)
        if old is not None:
            d = old + 1
            if t not in new or d < new[t]:
                new[t] = d
    return new


def update_distances(prev_distances, next_distances, edges):
    """shortest_path/mapper.rs:57-88 for a batch of (from, to): the batch's own minimum per destination first, then one U64Min upsert
    per destination.  Returns (keys, actions)."""
    new = new_distances(prev_distances, edges)
    keys = list(new)
    return keys, batch_upsert(next_distances, U64_MIN, keys, [new[k] for k in keys])
