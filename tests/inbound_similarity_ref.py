"""Host restatement of Scorer (crates/core/src/ranking/inbound_similarity.rs:61-138) over BitVec (ranking/bitvec_similarity.rs:22-189),
written as the reference writes it: sorted de-duplicated in-neighbour lists, a bloom of 16 u64 words, the two-pointer intersection,
`math.sqrt`, sequential float sums.  `numpy_scores` is the vectorised form for large graphs; tests/test_similarity_ref.py shows it equal
to the literal one, bit for bit, on the small cases before anything relies on it.

The in-neighbour set of a node is its whole in-list in the graph given here (include/hyperball.h names this difference from the
reference's 512 fetched backlinks)."""
import math

import numpy as np

MUL = 11400714819323198549
M64 = (1 << 64) - 1
NUM_BLOOMS = 16


def bloom_hash(item):
    """VeryJankyBloomFilter::hash (bitvec_similarity.rs:36-41) of the low 64 bits of an id: (word, bit)"""
    h = ((item & M64) * MUL) & M64
    return h % NUM_BLOOMS, h % 64


class BitVec:
    """BitVec::new (bitvec_similarity.rs:144-163)"""

    def __init__(self, ranks=()):
        self.ranks = sorted(set(int(r) for r in ranks))
        self.data = [0] * NUM_BLOOMS
        self.ones = 0
        for r in self.ranks:  # insert_u128 -> insert (:43-57)
            a, b = bloom_hash(r)
            if self.data[a] & (1 << b):
                continue
            self.data[a] |= 1 << b
            self.ones += 1
        self.sqrt_len = math.sqrt(float(len(self.ranks)))

    def intersect_ones(self, other):
        return sum(bin(a & b).count("1") for a, b in zip(self.data, other.data))

    def intersection_size(self, other):
        """Posting::intersection_size (:85-111)"""
        a, b = self.ranks, other.ranks
        i = j = count = 0
        while i < len(a) and j < len(b):
            if a[i] == b[j]:
                count += 1
                i += 1
                j += 1
            elif a[i] < b[j]:
                i += 1
            else:
                j += 1
        return count

    def sim(self, other):
        """BitVec::sim (:165-180)"""
        if self.sqrt_len == 0.0 or other.sqrt_len == 0.0:
            return 0.0
        max_ones = max(self.ones, other.ones)
        if float(self.intersect_ones(other)) / float(max_ones) < 0.25:
            return 0.0
        return float(self.intersection_size(other)) / (self.sqrt_len * other.sqrt_len)

    def fold(self):
        """the 16 words as one u64: word a only ever holds bits b with b % 16 == a, so OR loses nothing"""
        m = 0
        for w in self.data:
            m |= w
        return m


class Scorer:
    """Scorer::new / calculate_score / set_self_score (inbound_similarity.rs:71-137); liked / disliked: lists of (id, BitVec)"""

    def __init__(self, liked, disliked, normalized, self_score=1.0):
        self.liked, self.disliked, self.normalized, self.self_score = list(liked), list(disliked), bool(normalized), float(self_score)

    def _sim(self, anchor, node, inbound):  # NodeScorer::sim (:44-50)
        return self.self_score if anchor[0] == node else anchor[1].sim(inbound)

    def score(self, node, inbound):
        sl = 0.0
        for a in self.liked:
            sl += self._sim(a, node, inbound)
        sd = 0.0
        for a in self.disliked:
            sd += self._sim(a, node, inbound)
        s = float(len(self.disliked)) + (sl - sd)
        if self.normalized:
            s = s / float(max(len(self.liked), 1))
        return max(s, 0.0)


def id_ints(ids):
    return [(int(h) << 64) | int(l) for l, h in zip(ids["lo"].tolist(), ids["hi"].tolist())]


def bitvecs(ids, row_ptr, src):
    """{id: BitVec of its in-list} of a dense graph (ids U128 ascending, CSR of in-lists by index)"""
    ints = id_ints(ids)
    rp = [int(x) for x in row_ptr]
    s = [int(x) for x in src]
    return {v: BitVec(ints[u] for u in s[rp[i]:rp[i + 1]]) for i, v in enumerate(ints)}


def make_scorer(bv, liked, disliked, normalized, self_score=1.0):
    empty = BitVec()
    return Scorer([(a, bv.get(a, empty)) for a in liked], [(a, bv.get(a, empty)) for a in disliked], normalized, self_score)


def literal(ids, row_ptr, src, liked, disliked, normalized=False, self_score=1.0, bv=None):
    """float64 score of every node, ascending NodeID"""
    bv = bv if bv is not None else bitvecs(ids, row_ptr, src)
    sc = make_scorer(bv, liked, disliked, normalized, self_score)
    return np.array([sc.score(v, bv[v]) for v in id_ints(ids)], dtype=np.float64)


def lookup(bv, liked, disliked, normalized, self_score, ids):
    """Scorer::score of arbitrary ids (an id that is no node: BitVec::default())"""
    sc = make_scorer(bv, liked, disliked, normalized, self_score)
    empty = BitVec()
    return np.array([sc.score(v, bv.get(v, empty)) for v in ids], dtype=np.float64)


def counts(bv, ids, anchors):
    """(n, len(anchors)) exact intersection sizes; an anchor that is no node: 0"""
    ints = id_ints(ids)
    out = np.zeros((len(ints), len(anchors)), dtype=np.uint32)
    for j, a in enumerate(anchors):
        if a in bv:
            for i, v in enumerate(ints):
                out[i, j] = bv[v].intersection_size(bv[a])
    return out


def top_order(ids, scores, k, skip=()):
    """sorted_k(Reverse((SortableFloat(score), node))) (similar_hosts.rs:182-191): score descending, ties by NodeID descending"""
    skip = set(skip)
    items = [(float(s), v) for v, s in zip(id_ints(ids), scores) if v not in skip]
    items.sort(key=lambda t: (-t[0], -t[1]))
    return items[:k]


# ---- the vectorised form ---------------------------------------------------------------------------------------------------------------
def _popcount64(a):
    return np.unpackbits(np.ascontiguousarray(a, dtype=np.uint64).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def numpy_state(ids, row_ptr, src):
    """(len, bloom as one u64, row of every edge) of a dense graph"""
    n = len(ids)
    rp = np.asarray(row_ptr, dtype=np.int64)
    s = np.asarray(src, dtype=np.int64)
    length = np.diff(rp)
    with np.errstate(over="ignore"):
        pos = (np.asarray(ids["lo"], dtype=np.uint64) * np.uint64(MUL)) & np.uint64(63)
    bits = np.uint64(1) << pos[s]
    bloom = np.zeros(n, dtype=np.uint64)
    rows = np.repeat(np.arange(n, dtype=np.int64), length)
    if len(s):  # one OR per non-empty row: its segment ends where the next non-empty row begins
        bloom[length > 0] = np.bitwise_or.reduceat(bits, rp[:-1][length > 0])
    return length, bloom, rows


def numpy_scores(ids, row_ptr, src, liked, disliked, normalized=False, self_score=1.0, state=None):
    n = len(ids)
    rp = np.asarray(row_ptr, dtype=np.int64)
    s = np.asarray(src, dtype=np.int64)
    length, bloom, rows = state if state is not None else numpy_state(ids, row_ptr, src)
    index = {v: i for i, v in enumerate(id_ints(ids))}
    ones = _popcount64(bloom)
    sqrt_len = np.sqrt(length.astype(np.float64))

    def total(entries):
        acc = np.zeros(n, dtype=np.float64)
        for a in entries:  # sequentially, in entry order: adding a +0.0 term changes no bit of a sum that is never -0.0
            i = index.get(a)
            if i is None:
                continue
            ind = np.zeros(n, dtype=np.int64)
            ind[s[rp[i]:rp[i + 1]]] = 1
            inter = np.bincount(rows, weights=ind[s], minlength=n) if len(s) else np.zeros(n)
            gate = (length > 0) & (length[i] > 0) & (4 * _popcount64(bloom & bloom[i]) >= np.maximum(ones, ones[i]))
            with np.errstate(divide="ignore", invalid="ignore"):
                term = np.where(gate, inter.astype(np.float64) / (sqrt_len[i] * sqrt_len), 0.0)
            term[i] = self_score
            acc = acc + term
        return acc

    sc = float(len(disliked)) + (total(liked) - total(disliked))
    if normalized:
        sc = sc / float(max(len(liked), 1))
    return np.maximum(sc, 0.0) + 0.0
