"""Fan forests: graphs whose walk results have closed forms that do not depend on the order of any sum.

For a list of lengths Ks:

    r2 -> x -> r,   r -> h_K for every K,   h_K -> K leaves,   leaf i of h_K -> w(K, i) tips of its own

`diamond=True` replaces r -> h_K by r -> {a_K, b_K} -> h_K.  `flipped=True` hands out the same graph with every edge reversed, so
that the in-lists carry the lengths instead of the out-lists.

The plain fan is a tree: from every source sigma == 1 everywhere below it and delta_s(v) = the number of descendants of v, so every
coefficient (1 + delta) / sigma is a small integer and neighbouring leaves of a hub carry different ones (w is a hash, not i % 4).  In
the diamond flavour sigma == 2 from h_K down for the sources above the diamond; the coefficients are then half-integers.  Every sum
is an integer or half-integer far below 2^53: the same f64 in any summation shape.  A kernel that reads the wrong entry of a list, or
drops or doubles one, changes the answer; one that only adds in another order does not.

Node ids are index + 1 in this order: r2, x, r, [a_K, b_K per K], the hubs h_K (consecutive, in the order of Ks), the leaves hub by
hub, the tips leaf by leaf.  Every node has an edge, so the sid of a node in a loaded graph is its index here.  Plain Python and
numpy; tests/test_fans_ref.py checks the closed forms against the literal restatements on a small Ks."""
import numpy as np

# the smallest lengths that straddle every list-length switch and every step size of the walk kernels (4, 8, 16, 64, 256, 4096,
# a second and third 4096-entry segment) and the 16-entry tail of the 256 + 16 k lists
KS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 271, 272, 273, 4095, 4096, 4097, 8191, 8192, 8193, 12289)

CHAIN, MID, HUB, LEAF, TIP = 0, 1, 2, 3, 4
UNREACHED = 255


def w(K, i):
    """tips of leaf i of h_K: the top two bits of a 32-bit integer hash of (K, i) (no period of 4, 16, 64 or 4096 in i)"""
    m = np.uint64(0xFFFFFFFF)
    h = ((np.asarray(i, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761) + np.uint64(K) * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(30)).astype(np.int64)


class Fan:
    def __init__(self, Ks=KS, diamond=False):
        self.Ks = tuple(int(K) for K in Ks)
        self.diamond = bool(diamond)
        G = len(self.Ks)
        self.r2, self.x, self.r = 0, 1, 2
        nxt = 3
        self.mid = np.zeros((G, 2), dtype=np.int64)  # a_K, b_K (diamond only)
        if diamond:
            self.mid = nxt + np.arange(2 * G, dtype=np.int64).reshape(G, 2)
            nxt += 2 * G
        self.hub = nxt + np.arange(G, dtype=np.int64)
        nxt += G
        kinds = [np.full(3, CHAIN), np.full(2 * G if diamond else 0, MID), np.full(G, HUB)]
        groups = [np.full(3, -1), np.repeat(np.arange(G), 2) if diamond else np.zeros(0, dtype=np.int64), np.arange(G)]
        self.leaf_first = np.zeros(G, dtype=np.int64)
        tips = []
        for g, K in enumerate(self.Ks):
            self.leaf_first[g] = nxt
            nxt += K
            tips.append(w(K, np.arange(K)))
            kinds.append(np.full(K, LEAF))
            groups.append(np.full(K, g))
        self.tips_of_leaf = np.concatenate(tips) if tips else np.zeros(0, dtype=np.int64)  # per leaf, in leaf order
        first_leaf, n_leaves = int(self.leaf_first[0]) if G else nxt, len(self.tips_of_leaf)
        leaf_index = first_leaf + np.arange(n_leaves, dtype=np.int64)
        tip_leaf = np.repeat(leaf_index, self.tips_of_leaf)
        self.tip_first = nxt
        kinds.append(np.full(len(tip_leaf), TIP))
        groups.append(np.concatenate(groups[3:])[tip_leaf - first_leaf] if n_leaves else np.zeros(0, dtype=np.int64))
        self.n = nxt + len(tip_leaf)
        self.kind = np.concatenate(kinds).astype(np.int64)
        self.group = np.concatenate(groups).astype(np.int64)
        assert len(self.kind) == self.n == len(self.group)
        # the leaf a node hangs under: a leaf itself, its tips; -1 above
        self.leaf_of = np.full(self.n, -1, dtype=np.int64)
        self.leaf_of[leaf_index] = leaf_index
        self.leaf_of[self.tip_first:] = tip_leaf
        # depth below r2
        hub_depth = 4 if diamond else 3
        self.depth = np.zeros(self.n, dtype=np.int64)
        self.depth[[self.x, self.r]] = (1, 2)
        self.depth[self.kind == MID] = 3
        self.depth[self.kind == HUB] = hub_depth
        self.depth[self.kind == LEAF] = hub_depth + 1
        self.depth[self.kind == TIP] = hub_depth + 2
        # descendants, in closed form
        self.desc = np.zeros(self.n, dtype=np.int64)
        self.desc[leaf_index] = self.tips_of_leaf
        under_hub = np.array([K + int(t.sum()) for K, t in zip(self.Ks, tips)], dtype=np.int64)  # the leaves and their tips
        self.desc[self.hub] = under_hub
        if diamond:
            self.desc[self.mid] = (1 + under_hub)[:, None]
        self.desc[self.r] = int(((3 if diamond else 1) + under_hub).sum())
        self.desc[self.x] = self.desc[self.r] + 1
        self.desc[self.r2] = self.desc[self.r] + 2
        # edges, as node indices
        frm = [np.array([self.r2, self.x]), ]
        to = [np.array([self.x, self.r]), ]
        if diamond:
            frm += [np.full(2 * G, self.r), self.mid.reshape(-1)]
            to += [self.mid.reshape(-1), np.repeat(self.hub, 2)]
        else:
            frm.append(np.full(G, self.r))
            to.append(self.hub)
        frm += [np.repeat(self.hub, self.Ks), tip_leaf]
        to += [leaf_index, self.tip_first + np.arange(len(tip_leaf), dtype=np.int64)]
        self.frm = np.concatenate(frm).astype(np.int64)
        self.to = np.concatenate(to).astype(np.int64)

    # ---- the graph -------------------------------------------------------------------------------------------------------------------
    def hub_of(self, K):
        return int(self.hub[self.Ks.index(K)])

    def leaves(self, K):
        g = self.Ks.index(K)
        return np.arange(self.leaf_first[g], self.leaf_first[g] + K, dtype=np.int64)

    def edges(self, flipped=False):
        """(from, to) as arrays of node ids (index + 1)"""
        return (self.to + 1, self.frm + 1) if flipped else (self.frm + 1, self.to + 1)

    def tuples(self, flipped=False):
        f, t = self.edges(flipped)
        return list(zip(f.tolist(), t.tolist()))

    # ---- closed forms ----------------------------------------------------------------------------------------------------------------
    def subtree(self, s):
        """mask of s and everything s reaches"""
        k, m = self.kind[s], np.zeros(self.n, dtype=bool)
        if k == CHAIN:
            m = self.depth >= self.depth[s]
        elif k in (MID, HUB):
            m = (self.group == self.group[s]) & (self.kind >= HUB)
        elif k == LEAF:
            m = self.leaf_of == s
        m[s] = True
        return m

    def ancestors(self, t):
        """mask of t and everything that reaches t"""
        m = np.zeros(self.n, dtype=bool)
        m[t] = True
        k = self.kind[t]
        m[:3] = self.depth[:3] <= self.depth[t]  # r2, x, r: the chain down to t, all of it for a node below r
        if k >= HUB:
            m[self.hub[self.group[t]]] = True
            if self.diamond:
                m[self.mid[self.group[t]]] = True
        if k == TIP:
            m[self.leaf_of[t]] = True
        return m

    def dist_from(self, sources):
        """uint8 distance of every node from the nearest of `sources` along the edges; 255 = not reached"""
        d = np.full(self.n, UNREACHED, dtype=np.int64)
        for s in sources:
            m = self.subtree(s)
            d[m] = np.minimum(d[m], self.depth[m] - self.depth[s])
        return d.astype(np.uint8)

    def dist_to(self, targets):
        """the same against the edges (= along the edges of the flipped graph)"""
        d = np.full(self.n, UNREACHED, dtype=np.int64)
        for t in targets:
            m = self.ancestors(t)
            d[m] = np.minimum(d[m], self.depth[t] - self.depth[m])
        return d.astype(np.uint8)

    def brandes(self, s):
        """(dist int64 with -1 = unreached, sigma uint64, delta float64) of source s.  delta_s(v) counts the nodes below v, except
        that a_K / b_K each carry half of what hangs under h_K for a source above the diamond."""
        m = self.subtree(s)
        dist = np.where(m, self.depth - self.depth[s], -1)
        above = self.diamond and self.kind[s] == CHAIN
        sigma = np.where(m, 1, 0).astype(np.uint64)
        delta = np.where(m, self.desc, 0).astype(np.float64)
        if above:
            sigma[m & (self.kind >= HUB)] = 2
            mid = m & (self.kind == MID)
            delta[mid] = self.desc[mid].astype(np.float64) / 2.0  # (1 + what is under h_K) / 2, and desc of a_K is that numerator
        return dist, sigma, delta

    def sums(self, sources):
        """(sum over the sources s != v of delta_s(v) in ascending source order, mask of the results)"""
        total = np.zeros(self.n, dtype=np.float64)
        reached = np.zeros(self.n, dtype=bool)
        for s in sorted(set(int(s) for s in sources)):
            dist, _, delta = self.brandes(s)
            delta[s] = 0.0
            total += delta
            reached |= dist >= 0
        return total, reached
