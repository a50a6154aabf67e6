"""Host restatement of scored_nodes of SimilarHostsFinder::find_similar_hosts (crates/core/src/similar_hosts.rs:54-272) with the
definitions of include/hyperball.h: what hb_similar_hosts must return, entry for entry and bit for bit.

literal() is the seven steps as written, with Python dicts, sets and sorted lists: the lists come from tests/links_ref.py and
tests/forwardlinks_ref.py (by import, unchanged), the BitVec - sixteen literal bloom words, a two-pointer intersection, math.sqrt - from
tests/inbound_similarity_ref.py.  layered() builds the test graphs: liked hosts, a layer of sources, a layer of targets."""
from tests import forwardlinks_ref as fref
from tests import graphs
from tests import inbound_similarity_ref as iref
from tests import links_ref as lref

LIST, PREFIX = 512, 128


def literal(ids, row_ptr, src, keys, liked, k):
    """keys: [(node, key)], liked: [node] in caller order (duplicates and unknown ids as given), k: the limit
    -> dict(nb, apply, bound, taken, candidates [(node, count)], top [(node, score)], and the stats counters forward_entries (the entries
    of the lists of step 3), distinct_targets (nodes with a count), gated / intersected (the pairs of step 6 by what the gate said))"""
    known = set(lref.id_ints(ids))
    N = len(liked)
    distinct = sorted({a for a in liked if a in known})
    in512 = dict(zip(distinct, ([u for u, _ in lst] for lst in lref.literal(ids, row_ptr, src, keys, distinct, LIST)[0])))  # step 1
    B = sorted({u for a in distinct for u in in512[a][:PREFIX]})  # step 2
    nb = len(B)
    count, forward_entries = {}, 0
    for lst in fref.literal(ids, row_ptr, src, keys, B, LIST)[0]:  # steps 3 and 4
        forward_entries += len(lst)
        for v, _ in lst:
            count[v] = count.get(v, 0) + 1
    apply, bound = nb > 32, (nb + 3) // 4
    rest = [(v, c) for v, c in count.items() if not apply or c <= bound]
    rest.sort(key=lambda e: (-e[1], e[0]))
    taken = rest[:256 if apply else 1024]
    candidates = [(v, c) for v, c in taken if v not in set(distinct)]  # only then
    cin = lref.literal(ids, row_ptr, src, keys, [v for v, _ in candidates], LIST)[0]  # step 5
    bv_c = {v: iref.BitVec(u for u, _ in lst) for (v, _), lst in zip(candidates, cin)}
    bv_a = {a: iref.BitVec(in512[a]) for a in distinct}
    empty = iref.BitVec()
    scored, gated, intersected = [], 0, 0
    for v, _ in candidates:  # step 6
        s = 0.0
        for a in liked:
            s += bv_a.get(a, empty).sim(bv_c[v])
            if a in bv_a and bv_a[a].ranks and bv_c[v].ranks:  # (a pair with an unknown entry or an empty list is neither gated nor intersected)
                if 4 * bv_a[a].intersect_ones(bv_c[v]) < max(bv_a[a].ones, bv_c[v].ones):
                    gated += 1
                else:
                    intersected += 1
        s = s / float(max(N, 1))
        scored.append((v, max(s, 0.0)))
    top = sorted(scored, key=lambda e: (-e[1], -e[0]))[:int(k)]  # step 7
    return dict(nb=nb, apply=apply, bound=bound, taken=len(taken), candidates=candidates, top=top, forward_entries=forward_entries,
                distinct_targets=len(count), gated=gated, intersected=intersected)


def layered(liked_in, source_out, extra=()):
    """liked_in: {liked host: [sources]}, source_out: {source: [targets]}, extra: [(from, to)] -> (ids, row_ptr, src) of the graph"""
    edges = [(u, a) for a, us in liked_in.items() for u in us] + [(b, v) for b, vs in source_out.items() for v in vs] + list(extra)
    return graphs.dense_from_tuples(edges)


# ---- the same on arrays, for graphs too large for the dicts ---------------------------------------------------------------------------
import math  # noqa: E402

import numpy as np  # noqa: E402


def numpy_state(ids, row_ptr, src):
    """what does not depend on keys or liked hosts: both CSRs and the bloom bit of every node"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    s = np.asarray(src, dtype=np.int64)
    out_ptr, dst = fref.out_csr(rp, s)
    with np.errstate(over="ignore"):
        bit = (np.asarray(ids["lo"], dtype=np.uint64) * np.uint64(iref.MUL)) & np.uint64(63)
    return dict(ids=ids, rp=rp, src=s, out_ptr=out_ptr, dst=dst, bit=bit.astype(np.int64), n=len(rp) - 1)


def _node(ids, sid):
    return (int(ids["hi"][sid]) << 64) | int(ids["lo"][sid])


def _sid_of(ids, node):
    lo, hi = 0, len(ids)
    while lo < hi:
        mid = (lo + hi) // 2
        if _node(ids, mid) < node:
            lo = mid + 1
        else:
            hi = mid
    return lo if lo < len(ids) and _node(ids, lo) == node else -1


def _best(lst, v, key, limit):
    lst = lst[lst != v]
    return lst[np.lexsort((lst, key[lst]))[:limit]]


def _mask(bits):
    m = 0
    for b in np.unique(bits).tolist():
        m |= 1 << b
    return m


def numpy_form(state, key_by_sid, liked, k):
    """literal() in sid space: key_by_sid = one uint64 per node (2^64 - 1 = not listed); the same dict, nodes as ints"""
    ids, rp, src, out_ptr, dst, bit, n = (state[f] for f in ("ids", "rp", "src", "out_ptr", "dst", "bit", "n"))
    key = np.asarray(key_by_sid, dtype=np.uint64)
    sids = [_sid_of(ids, a) for a in liked]
    distinct = sorted({s for s in sids if s >= 0})
    in512 = {a: _best(src[rp[a]:rp[a + 1]], a, key, LIST) for a in distinct}
    B = np.unique(np.concatenate([in512[a][:PREFIX] for a in distinct])) if distinct else np.zeros(0, dtype=np.int64)
    nb = len(B)
    count, forward_entries = np.zeros(n, dtype=np.int64), 0
    for b in B.tolist():
        fw = _best(dst[out_ptr[b]:out_ptr[b + 1]], b, key, LIST)
        forward_entries += len(fw)
        count[fw] += 1  # (unique edges: no index repeats inside one list)
    apply, bound = nb > 32, (nb + 3) // 4
    touched = np.flatnonzero(count)
    distinct_targets = len(touched)
    c = count[touched]
    keep = (c <= bound) if apply else np.ones(len(c), dtype=bool)
    touched, c = touched[keep], c[keep]
    order = np.lexsort((touched, -c))[:256 if apply else 1024]
    taken, tc = touched[order], c[order]
    stay = ~np.isin(taken, np.array(distinct, dtype=np.int64))
    cand, cc = taken[stay], tc[stay]
    vec = lambda lst: (np.sort(lst), _mask(bit[lst]))  # noqa: E731
    va = {a: vec(in512[a]) for a in distinct}
    scored, gated, intersected = [], 0, 0
    for v in cand.tolist():
        lc, mc = vec(_best(src[rp[v]:rp[v + 1]], v, key, LIST))
        s = 0.0
        for a in sids:
            if a < 0:
                continue
            la, ma = va[a]
            if not len(la) or not len(lc):
                continue
            if 4 * bin(ma & mc).count("1") < max(bin(ma).count("1"), bin(mc).count("1")):
                gated += 1
                continue
            intersected += 1
            s += float(len(np.intersect1d(la, lc, assume_unique=True))) / (math.sqrt(float(len(la))) * math.sqrt(float(len(lc))))
        scored.append((_node(ids, v), max(s / float(max(len(liked), 1)), 0.0)))
    top = sorted(scored, key=lambda e: (-e[1], -e[0]))[:int(k)]
    return dict(nb=nb, apply=apply, bound=bound, taken=len(taken), candidates=[(_node(ids, v), int(x)) for v, x in zip(cand.tolist(), cc.tolist())], top=top,
                forward_entries=forward_entries, distinct_targets=distinct_targets, gated=gated, intersected=intersected)


def sids_of_subset(all_ids, ids):
    """sid of every id of `ids`, an ascending subset of all_ids (both U128 arrays)"""
    n, k = len(all_ids), len(ids)
    hi = np.concatenate((all_ids["hi"], ids["hi"]))
    lo = np.concatenate((all_ids["lo"], ids["lo"]))
    tag = np.concatenate((np.zeros(n, dtype=np.int8), np.ones(k, dtype=np.int8)))
    order = np.lexsort((tag, lo, hi))
    sub = tag[order] == 1
    return (np.cumsum(~sub) - 1)[sub].astype(np.int64)
