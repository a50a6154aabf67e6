"""Host restatement of HostBacklinksQuery::new(node).with_limit(EdgeLimit::Limit(L)) (crates/core/src/webgraph/query/backlink.rs:
230-360) with the definitions of include/hyperball.h: what hb_backlinks must return, entry for entry.

literal() is the definition as written: per query the in-neighbours from the CSR by destination, the node itself dropped, sorted by
(key, id), cut at L.  numpy_form() is the same on arrays, for graphs too large for the lists; tests/test_links_ref.py shows the two
equal on a small graph before tests/test_links.py uses the second.  The graph is (ids, row_ptr, src) as Context.graph() returns it: the
in-list of sid v is src[row_ptr[v]:row_ptr[v + 1]], unique edges."""
import numpy as np

U64_MAX = (1 << 64) - 1


def id_ints(ids):
    return [(int(h) << 64) | int(l) for l, h in zip(ids["lo"].tolist(), ids["hi"].tolist())]


def literal(ids, row_ptr, src, keys, queries, limit, keep_self=False):
    """keys: [(node, key)] in list order (the last entry of a node wins, unknown nodes are counted), queries: [node]
    -> (lists [[(node, key)] per query], degrees [int per query], unknown keys, unknown queries)"""
    nodes = id_ints(ids)
    sid_of = {v: i for i, v in enumerate(nodes)}
    rp = [int(x) for x in row_ptr]
    key, unknown_keys = {}, 0
    for node, k in keys:
        if node in sid_of:
            key[node] = int(k)
        else:
            unknown_keys += 1
    lists, degrees, unknown = [], [], 0
    for q in queries:
        if q not in sid_of:
            unknown += 1
            lists.append([])
            degrees.append(0)
            continue
        i = sid_of[q]
        found = [nodes[int(u)] for u in src[rp[i]:rp[i + 1]]]
        if not keep_self:
            found = [u for u in found if u != q]  # LinksQuery.skip_self_links
        found = sorted((key.get(u, U64_MAX), u) for u in found)
        degrees.append(len(found))
        lists.append([(u, k) for k, u in found[:int(limit)]])
    return lists, degrees, unknown_keys, unknown


def numpy_form(row_ptr, src, key_by_sid, query_sids, limit, keep_self=False):
    """the same in sid space: key_by_sid = one uint64 per node (U64_MAX = not listed), query_sids = int array (every one a node)
    -> (offsets int64 [q + 1], list entries as sids int64, their keys uint64, degrees int64)"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    key = np.asarray(key_by_sid, dtype=np.uint64)
    q = np.asarray(query_sids, dtype=np.int64)
    lens = rp[q + 1] - rp[q]
    owner = np.repeat(np.arange(len(q), dtype=np.int64), lens)  # the query an entry belongs to
    start = np.repeat(rp[q] - np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
    frm = src[np.arange(len(owner), dtype=np.int64) + start]
    if not keep_self:
        keep = frm != q[owner]
        frm, owner = frm[keep], owner[keep]
    order = np.lexsort((frm, key[frm], owner))  # by (query, key[from], from)
    frm, owner = frm[order], owner[order]
    degrees = np.bincount(owner, minlength=len(q)).astype(np.int64)
    first = np.concatenate(([0], np.cumsum(degrees)[:-1]))
    pos = np.arange(len(owner), dtype=np.int64) - first[owner]
    take = pos < int(limit)
    kept = np.minimum(degrees, int(limit))
    offsets = np.concatenate(([0], np.cumsum(kept))).astype(np.int64)
    return offsets, frm[take], key[frm[take]], degrees
