"""Host restatement of hb_score_hosts (include/hyperball.h): per request, inbound_similarity_ref.Scorer / lookup over the BitVecs of
limited_similarity_ref.bitvecs - Scorer::score of every node entry against the request's liked / disliked hosts, exactly as the lookup
route (hb_inbound_similarity + hb_similarity_lookup) is restated - plus the four pair classes the operator counts.

A request is a dict: nodes, and optionally liked, disliked, normalized, self_score (ids as Python ints).  The literal form works on a
{id: BitVec} table; the numpy form takes the cut graph of limited_similarity_ref.cut_graph and is what the larger graphs use
(tests/test_score_hosts_ref.py shows the two equal first)."""
import math

import numpy as np

from tests import inbound_similarity_ref as sref
from tests import limited_similarity_ref as lref

CLASSES = ("pairs_self", "pairs_empty", "pairs_gated", "pairs_intersected")
EMPTY = sref.BitVec()


def fields(req):
    return (list(req.get("liked", ())), list(req.get("disliked", ())), list(req["nodes"]), bool(req.get("normalized", False)),
            1.0 if req.get("self_score") is None else float(req["self_score"]))


def classify(a, va, v, vv):
    """the class of the pair (anchor a with BitVec va, node v with BitVec vv), in the order the header defines"""
    if a == v:
        return "pairs_self"
    if not va.ranks or not vv.ranks:
        return "pairs_empty"
    if 4 * va.intersect_ones(vv) < max(va.ones, vv.ones):
        return "pairs_gated"
    return "pairs_intersected"


def literal(bv, requests):
    """([float64 scores per request], stats): stats holds every integer counter of hb_score_stats except pieces and device_bytes"""
    out = []
    st = dict.fromkeys(CLASSES + ("requests", "anchors", "nodes", "unknown_anchors", "unknown_nodes", "pairs"), 0)
    known = set()
    for req in requests:
        liked, disliked, nodes, normalized, self_score = fields(req)
        out.append(sref.lookup(bv, liked, disliked, normalized, self_score, nodes))
        st["requests"] += 1
        st["anchors"] += len(liked) + len(disliked)
        st["nodes"] += len(nodes)
        st["unknown_anchors"] += sum(1 for a in liked + disliked if a not in bv)
        st["unknown_nodes"] += sum(1 for v in nodes if v not in bv)
        st["pairs"] += (len(liked) + len(disliked)) * len(nodes)
        known.update(x for x in liked + disliked + nodes if x in bv)
        for v in nodes:
            for a in liked + disliked:
                st[classify(a, bv.get(a, EMPTY), v, bv.get(v, EMPTY))] += 1
    st["distinct"] = len(known)
    return out, st


def tables(ids, row_ptr, src, keys, limit):
    return lref.bitvecs(ids, row_ptr, src, keys, limit)


def numpy_form(cut, requests):
    """the same from the cut graph (ids, row_ptr, src with every in-list cut to backlinks(v, limit)), pair by pair on the sorted cut
    lists: the work is the operator's own, (nodes x anchors) intersections, so a graph of any size can be checked"""
    ids, rp, s = cut
    rp = np.asarray(rp, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    index = {v: i for i, v in enumerate(sref.id_ints(ids))} if len(ids) < (1 << 16) else _Index(ids)
    length, bloom, _ = sref.numpy_state(ids, rp, s)
    ones = sref._popcount64(bloom)
    lists = {}

    def entries(i):
        if i not in lists:
            lists[i] = np.sort(s[rp[i]:rp[i + 1]])
        return lists[i]

    out = []
    st = dict.fromkeys(CLASSES + ("requests", "anchors", "nodes", "unknown_anchors", "unknown_nodes", "pairs"), 0)
    known = set()
    for req in requests:
        liked, disliked, nodes, normalized, self_score = fields(req)
        anchors = liked + disliked
        ai = [index.get(a, -1) for a in anchors]
        vi = [index.get(v, -1) for v in nodes]
        st["requests"] += 1
        st["anchors"] += len(anchors)
        st["nodes"] += len(nodes)
        st["unknown_anchors"] += sum(1 for i in ai if i < 0)
        st["unknown_nodes"] += sum(1 for i in vi if i < 0)
        st["pairs"] += len(anchors) * len(nodes)
        known.update(i for i in ai + vi if i >= 0)
        scores = []
        for v, i in zip(nodes, vi):
            sums = [0.0, 0.0]
            for k, (a, j) in enumerate(zip(anchors, ai)):
                if a == v:
                    st["pairs_self"] += 1
                    term = self_score
                elif i < 0 or j < 0 or not length[i] or not length[j]:
                    st["pairs_empty"] += 1
                    continue
                elif 4 * int(sref._popcount64(np.array([bloom[i] & bloom[j]], dtype=np.uint64))[0]) < max(int(ones[i]), int(ones[j])):
                    st["pairs_gated"] += 1
                    continue
                else:
                    st["pairs_intersected"] += 1
                    count = len(np.intersect1d(entries(i), entries(j), assume_unique=True))
                    term = float(count) / (math.sqrt(float(length[j])) * math.sqrt(float(length[i])))
                sums[0 if k < len(liked) else 1] += term
            x = float(len(disliked)) + (sums[0] - sums[1])
            if normalized:
                x = x / float(max(len(liked), 1))
            scores.append(max(x, 0.0))
        out.append(np.array(scores, dtype=np.float64))
    st["distinct"] = len(known)
    return out, st


class _Index:
    """id -> sid of a large graph by binary search on the ascending (hi, lo) words instead of a dict of every node"""

    def __init__(self, ids):
        self.hi = np.asarray(ids["hi"], dtype=np.uint64)
        self.lo = np.asarray(ids["lo"], dtype=np.uint64)

    def get(self, v, default=-1):
        hi, lo = np.uint64(v >> 64), np.uint64(v & sref.M64)
        a, b = int(np.searchsorted(self.hi, hi, "left")), int(np.searchsorted(self.hi, hi, "right"))
        i = a + int(np.searchsorted(self.lo[a:b], lo))
        return i if i < b and int(self.lo[i]) == int(lo) else default


def cut_for(ids, row_ptr, src, keys_by_sid, limit, requests):
    """a cut graph that holds the cut lists of the hosts the requests name and no other list: what numpy_form reads, at the cost of
    those hosts' in-lists instead of the whole graph's (limited_similarity_ref.cut_graph cuts every list)"""
    n = len(ids)
    index = _Index(ids)
    named = sorted({i for req in requests for k in ("liked", "disliked", "nodes") for i in (index.get(v) for v in req.get(k, ())) if i >= 0})
    kb = np.full(n, lref.U64_MAX, dtype=np.uint64) if keys_by_sid is None else np.asarray(keys_by_sid, dtype=np.uint64)
    offsets, frm, _, _ = lref.links_ref.numpy_form(row_ptr, src, kb, np.array(named, dtype=np.int64), limit)
    length = np.zeros(n, dtype=np.int64)
    length[named] = np.diff(offsets)
    return ids, np.concatenate(([0], np.cumsum(length))).astype(np.int64), frm
