"""Host restatement of HarmonicNearestSeed (crates/core/src/entrypoint/centrality.rs:126-201) with the definitions of
include/hyperball.h: what hb_nearest_seed must compute, bit for bit.

literal() is the reference as written - dicts, and per node the backlinks sorted by (key[from], from), self links skipped, the first one
taken, one multiply; the rounds are a loop over copies of the dict.  numpy_form() is the same on arrays, for graphs too large for the
dicts; tests/test_nearest_seed.py shows the two equal on a small graph before it uses the second.  The graph is (ids, row_ptr, src) as
Context.graph() returns it: the in-list of sid v is src[row_ptr[v]:row_ptr[v + 1]], unique edges."""
import numpy as np

U64_MAX = (1 << 64) - 1
STAT_KEYS = ("with_original", "filled", "unknown_orig", "unknown_keys", "no_seed", "seed_without_value", "rounds_run", "results")


def id_ints(ids):
    return [(int(h) << 64) | int(l) for l, h in zip(ids["lo"].tolist(), ids["hi"].tolist())]


def literal(ids, row_ptr, src, orig, keys, discount, rounds=1):
    """orig: [(node, value)] (the original_centrality Db, in insertion order), keys: [(node, key)] -> (seeds {node: node}, values
    {node: f64}, stats dict)"""
    nodes = id_ints(ids)
    known = set(nodes)
    rp = [int(x) for x in row_ptr]
    backlinks = {v: [nodes[int(u)] for u in src[rp[i]:rp[i + 1]]] for i, v in enumerate(nodes)}
    original, key = {}, {}
    unknown_orig = unknown_keys = 0
    for node, value in orig:  # Db::insert: the last one wins
        if node in known:
            original[node] = float(value)
        else:
            unknown_orig += 1
    for node, k in keys:
        if node in known:
            key[node] = int(k)
        else:
            unknown_keys += 1
    seeds = {}
    for v in nodes:  # BacklinksQuery::new(v).with_limit(Limit(1)): ascending sort_score, self links skipped
        found = sorted((key.get(u, U64_MAX), u) for u in backlinks[v] if u != v)
        if found:
            seeds[v] = found[0][1]
    val = dict(original)
    filled = [0] * 16
    rounds_run = 0
    for r in range(1, max(int(rounds), 1) + 1):
        new = dict(val)
        count = 0
        for v in nodes:
            if v not in val and v in seeds and seeds[v] in val:
                new[v] = val[seeds[v]] * float(discount)  # one f64 multiply
                count += 1
        val = new
        filled[min(r - 1, 15)] += count
        rounds_run = r
        if not count:
            break
    stats = dict(with_original=len(original), filled=filled, unknown_orig=unknown_orig, unknown_keys=unknown_keys,
                 no_seed=sum(1 for v in nodes if v not in val and v not in seeds),
                 seed_without_value=sum(1 for v in nodes if v not in val and v in seeds), rounds_run=rounds_run, results=len(val))
    return seeds, val, stats


def top_order(values, k):
    """[(node, value)]: the first k rows of harmonic.csv - (Reverse(SortableFloat(c)), node_id): value descending, NodeID ascending"""
    return sorted(values.items(), key=lambda item: (-item[1], item[0]))[:k]


def numpy_form(ids, row_ptr, src, orig_sids, orig_vals, key_by_sid, discount, rounds=1):
    """the same on arrays, in sid space: orig_sids / orig_vals = the known entries of the orig list in order, key_by_sid = one uint64
    per node (U64_MAX = not listed) -> (seed sid per node or -1, value per node, has per node, filled list, rounds_run)"""
    n = len(ids)
    rp = np.asarray(row_ptr, dtype=np.int64)
    frm = np.asarray(src, dtype=np.int64)
    to = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = frm != to
    frm, to = frm[keep], to[keep]
    order = np.lexsort((frm, np.asarray(key_by_sid, dtype=np.uint64)[frm], to))  # by (to, key[from], from)
    frm, to = frm[order], to[order]
    first = np.ones(len(to), dtype=bool)
    first[1:] = to[1:] != to[:-1]
    seed = np.full(n, -1, dtype=np.int64)
    seed[to[first]] = frm[first]
    val = np.zeros(n, dtype=np.float64)
    has = np.zeros(n, dtype=bool)
    for s, v in zip(np.asarray(orig_sids).tolist(), np.asarray(orig_vals, dtype=np.float64).tolist()):
        val[s], has[s] = v, True
    filled, rounds_run = [0] * 16, 0
    for r in range(1, max(int(rounds), 1) + 1):
        take = ~has & (seed >= 0)
        take[take] = has[seed[take]]
        new = val.copy()
        new[take] = val[seed[take]] * np.float64(discount)
        val, has = new, has | take
        filled[min(r - 1, 15)] += int(take.sum())
        rounds_run = r
        if not take.any():
            break
    return seed, val, has, filled, rounds_run
