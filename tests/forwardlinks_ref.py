"""Host restatement of HostForwardlinksQuery::new(node).with_limit(EdgeLimit::Limit(L)) (crates/core/src/webgraph/query/forwardlink.rs:
183-330) with the definitions of include/hyperball.h: what hb_forwardlinks must return, entry for entry.

literal() is the definition as written: per query the out-neighbours - every node whose in-list in the CSR by destination names the
queried node -, the node itself dropped, sorted by (key, id), cut at L.  numpy_form() transposes the CSR once (out_csr) and is then
tests/links_ref.py's numpy form on the transposed arrays: the two directions differ in nothing but the list they read.
tests/test_forwardlinks_ref.py shows the two equal before tests/test_forwardlinks.py uses the second.  The graph is (ids, row_ptr, src)
as Context.graph() returns it: the in-list of sid v is src[row_ptr[v]:row_ptr[v + 1]], unique edges."""
import numpy as np

from tests import links_ref as lref

U64_MAX = lref.U64_MAX
id_ints = lref.id_ints


def literal(ids, row_ptr, src, keys, queries, limit, keep_self=False):
    """keys: [(node, key)] in list order (the last entry of a node wins, unknown nodes are counted), queries: [node]
    -> (lists [[(node, key)] per query], degrees [int per query], unknown keys, unknown queries)"""
    nodes = id_ints(ids)
    known = set(nodes)
    rp = [int(x) for x in row_ptr]
    out = {v: [] for v in nodes}  # forward lists from the CSR by destination
    for i, v in enumerate(nodes):
        for u in src[rp[i]:rp[i + 1]]:
            out[nodes[int(u)]].append(v)
    key, unknown_keys = {}, 0
    for node, k in keys:
        if node in known:
            key[node] = int(k)
        else:
            unknown_keys += 1
    lists, degrees, unknown = [], [], 0
    for q in queries:
        if q not in known:
            unknown += 1
            lists.append([])
            degrees.append(0)
            continue
        found = out[q]
        if not keep_self:
            found = [v for v in found if v != q]  # LinksQuery.skip_self_links
        found = sorted((key.get(v, U64_MAX), v) for v in found)
        degrees.append(len(found))
        lists.append([(v, k) for k, v in found[:int(limit)]])
    return lists, degrees, unknown_keys, unknown


def out_csr(row_ptr, src):
    """the CSR by source of a CSR by destination: (out_ptr int64 [n + 1], dst int64), the out-list of sid u = dst[out_ptr[u]:out_ptr[u + 1]]"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    n = len(rp) - 1
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    order = np.lexsort((dst, src))
    out_ptr = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n)))).astype(np.int64)
    return out_ptr, dst[order]


def numpy_form(out_ptr, dst, key_by_sid, query_sids, limit, keep_self=False):
    """the same in sid space on the arrays of out_csr(): -> (offsets int64 [q + 1], list entries as sids int64, their keys uint64,
    degrees int64)"""
    return lref.numpy_form(out_ptr, dst, key_by_sid, query_sids, limit, keep_self)
