"""Host restatement of the finish of an AMPC job (include/hb_ampc.h: hbu_finish_centralities, hbu_top_centralities): the stored value
`f64::from(c) / divisor` (harmonic_centrality/coordinator.rs:204-211; divisor 1.0: approximated_harmonic_centrality/coordinator.rs:152-157),
the rank of store_harmonic - the position in the order (Reverse(SortableFloat(c)), NodeID), webgraph/centrality/mod.rs:92-103, where
SortableFloat is f64::total_cmp - and top_nodes (mod.rs:33-52).  Plain Python and numpy, no device: tests/test_ampc_finish_ref.py pins it
by hand-made cases, tests/test_ampc_finish.py compares the device with it."""
import numpy as np

M64 = (1 << 64) - 1


def quotients(values, divisor):
    """value / divisor in f64, one IEEE division each (values: floats; returns np.float64 array)"""
    with np.errstate(all="ignore"):
        return np.asarray(list(values), dtype=np.float64) / np.float64(divisor)


def bits(v):
    return int(np.float64(v).view(np.uint64))


def total_key(v):
    """f64::total_cmp as an integer key of the bit pattern: a < b under total_cmp iff total_key(a) < total_key(b)"""
    b = bits(v)
    return (b ^ M64) if b >> 63 else (b | (1 << 63))


def rank_order(ids, vals):
    """the indices of the entries in the order (value descending under total_cmp, id ascending)"""
    return sorted(range(len(ids)), key=lambda j: (-total_key(vals[j]), ids[j]))


def finish(model, divisor):
    """model: {id (int): value (float)}.  (ids, vals, ranks) in ascending id order, as hbu_finish_centralities returns them."""
    ids = sorted(model)
    vals = quotients([model[k] for k in ids], divisor)
    return ids, vals, ranks_of(ids, vals)


def ranks_of(ids, vals):
    ranks = [0] * len(ids)
    for pos, j in enumerate(rank_order(ids, vals)):
        ranks[j] = pos
    return ranks


def top(ids, vals, k):
    """the first min(k, len) (id, value) of the rank order: top_nodes"""
    return [(ids[j], vals[j]) for j in rank_order(ids, vals)[:k]]
