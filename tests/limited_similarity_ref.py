"""Host restatement of hb_inbound_similarity with a limit (include/hyperball.h): the Scorer of tests/inbound_similarity_ref.py, unchanged,
over BitVecs built from backlinks(v, limit) as tests/links_ref.py restates hb_backlinks - the in-neighbours u != v in the order
(key[u], NodeID u), the first min(limit, degree(v)) of them - for EVERY node, anchors included.

The literal form builds the lists with links_ref.literal and hands them to inbound_similarity_ref.BitVec / Scorer / counts.  The numpy
form cuts the CSR with links_ref.numpy_form and hands the cut graph to inbound_similarity_ref.numpy_scores / numpy_state (neither looks
at the order inside a list); tests/test_limited_similarity_ref.py shows the two equal before anything relies on the second.
limit == 0 is the whole mode: the graph as it is, self links included."""
import numpy as np

from tests import inbound_similarity_ref as sref
from tests import links_ref

U64_MAX = links_ref.U64_MAX
id_ints = sref.id_ints


def bitvecs(ids, row_ptr, src, keys, limit):
    """{id: BitVec of backlinks(id, limit)}; keys = [(node, key)] as links_ref.literal takes them"""
    if not limit:
        return sref.bitvecs(ids, row_ptr, src)
    ints = id_ints(ids)
    lists, _, _, _ = links_ref.literal(ids, row_ptr, src, keys, ints, limit)
    return {v: sref.BitVec(u for u, _ in lst) for v, lst in zip(ints, lists)}


def literal(ids, row_ptr, src, keys, limit, liked, disliked, normalized=False, self_score=1.0, bv=None):
    """float64 score of every node, ascending NodeID"""
    bv = bv if bv is not None else bitvecs(ids, row_ptr, src, keys, limit)
    return sref.literal(ids, row_ptr, src, liked, disliked, normalized, self_score, bv=bv)


def key_by_sid(ids, keys):
    """[(node, key)] -> one uint64 per node, U64_MAX = not listed (the last entry of a node wins)"""
    sid_of = {v: i for i, v in enumerate(id_ints(ids))}
    out = np.full(len(ids), U64_MAX, dtype=np.uint64)
    for node, k in keys:
        if node in sid_of:
            out[sid_of[node]] = k
    return out


def cut_graph(ids, row_ptr, src, keys_by_sid, limit):
    """(ids, row_ptr, src) with every in-list cut to backlinks(v, limit); keys_by_sid: uint64 per node or None (NodeID order)"""
    if not limit:
        return ids, np.asarray(row_ptr, dtype=np.int64), np.asarray(src, dtype=np.int64)
    n = len(ids)
    kb = np.full(n, U64_MAX, dtype=np.uint64) if keys_by_sid is None else np.asarray(keys_by_sid, dtype=np.uint64)
    offsets, frm, _, _ = links_ref.numpy_form(row_ptr, src, kb, np.arange(n, dtype=np.int64), limit)
    return ids, offsets, frm


def numpy_scores(cut, liked, disliked, normalized=False, self_score=1.0):
    return sref.numpy_scores(*cut, liked, disliked, normalized, self_score)


def numpy_export(cut, last):
    """what hb_debug_copy_similarity_batch shows after a limited call whose last batch holds the entries `last`:
    (counts (n, len(last)) uint32, bloom uint64, len uint32)"""
    ids, rp, s = cut
    n = len(ids)
    length, bloom, rows = sref.numpy_state(ids, rp, s)
    index = {v: i for i, v in enumerate(id_ints(ids))}
    counts = np.zeros((n, len(last)), dtype=np.uint32)
    for j, a in enumerate(last):
        i = index.get(a)
        if i is None or not len(s):
            continue
        ind = np.zeros(n, dtype=np.int64)
        ind[s[rp[i]:rp[i + 1]]] = 1
        counts[:, j] = np.bincount(rows, weights=ind[s], minlength=n).astype(np.uint32)
    return counts, bloom, length.astype(np.uint32)
