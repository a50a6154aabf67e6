"""Host restatement of Betweenness::calculate (crates/core/src/webgraph/centrality/betweenness.rs:29-146) for the tests of hb_betweenness.

    literal(n, row_ptr, src, sources)   betweenness.rs:50-122 as written: queue, stack, predecessor lists, Python ints for sigma
    numpy(n, row_ptr, src, sources)     the same quantities level by level with numpy, for the larger cases

The graph is the library's reduced one: CSR by destination in ascending-NodeID (sid) indexing, as Context.graph() returns it.  Both
return a Result: per source (ascending sid) dist / sigma / delta arrays, sums[v] = sum of delta_s(v) over the sources s != v in
ascending order, the result set, and max_dist.  Nothing here saturates or stops at 254 levels: those are limits of the library.
"""
from collections import deque

import numpy as np

UNREACHED = 255


class Result:
    def __init__(self, n, sources):
        self.n = n
        self.sources = sorted(set(int(s) for s in sources))
        self.dist = []    # per source: int array, -1 = unreached
        self.sigma = []   # per source: list of Python ints / uint64 array
        self.delta = []   # per source: float64 array
        self.sums = np.zeros(n, dtype=np.float64)
        self.reached = np.zeros(n, dtype=bool)
        self.max_dist = 0

    def values(self, raw=False):
        """value per sid: sum / (S (S - 1)) as one f64 division (betweenness.rs:128-140); -1.0 = no result"""
        s = np.float64(len(self.sources))
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.sums if raw else self.sums / (s * (s - np.float64(1.0)))
        return np.where(self.reached, v, -1.0)


def out_lists(n, row_ptr, src):
    """out-neighbour CSR (ptr, idx) of the in-edge CSR; the out-neighbours of a node in ascending sid order"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    order = np.argsort(src, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ptr[1:])
    return ptr, dst[order]


def literal(n, row_ptr, src, sources):
    ptr, idx = out_lists(n, row_ptr, src)
    ptr, idx = ptr.tolist(), idx.tolist()
    res = Result(n, sources)
    centrality = {}
    for s in res.sources:
        centrality.setdefault(s, 0.0)
        stack = []
        predecessors = {}
        sigma = {s: 1}
        distances = {s: 0}
        q = deque([s])
        while q:
            v = q.popleft()
            stack.append(v)
            for w in idx[ptr[v]:ptr[v + 1]]:
                if w not in distances:
                    q.append(w)
                    distances[w] = distances[v] + 1
                if distances[w] == distances[v] + 1:
                    sigma[w] = sigma.get(w, 0) + sigma.get(v, 0)
                    predecessors.setdefault(w, []).append(v)
        res.max_dist = max(res.max_dist, max(distances.values()))
        delta = {}
        while stack:
            w = stack.pop()
            for v in predecessors.get(w, ()):
                delta[v] = delta.get(v, 0.0) + (float(sigma[v]) / float(sigma[w])) * (1.0 + delta.get(w, 0.0))
            if w != s:
                centrality[w] = centrality.get(w, 0.0) + delta.get(w, 0.0)
        res.dist.append(np.array([distances.get(v, -1) for v in range(n)], dtype=np.int64))
        res.sigma.append([sigma.get(v, 0) for v in range(n)])
        res.delta.append(np.array([delta.get(v, 0.0) for v in range(n)], dtype=np.float64))
    for v, c in centrality.items():
        res.sums[v] = c
        res.reached[v] = True
    return res


def _expand(ptr, idx, nodes):
    """the out-edges (u, w) of `nodes`, in node order"""
    counts = ptr[nodes + 1] - ptr[nodes]
    total = int(counts.sum())
    if not total:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    first = np.cumsum(counts) - counts
    pos = np.repeat(ptr[nodes] - first, counts) + np.arange(total, dtype=np.int64)
    return np.repeat(nodes, counts), idx[pos]


def numpy(n, row_ptr, src, sources):
    ptr, idx = out_lists(n, row_ptr, src)
    res = Result(n, sources)
    for s in res.sources:
        dist = np.full(n, -1, dtype=np.int64)
        sigma = np.zeros(n, dtype=np.uint64)
        delta = np.zeros(n, dtype=np.float64)
        dist[s] = 0
        sigma[s] = 1
        levels = [np.array([s], dtype=np.int64)]
        while len(levels[-1]):
            d = len(levels)
            u, w = _expand(ptr, idx, levels[-1])
            new = np.unique(w[dist[w] < 0])
            dist[new] = d
            on = dist[w] == d
            np.add.at(sigma, w[on], sigma[u[on]])
            levels.append(new)
        levels.pop()
        res.max_dist = max(res.max_dist, len(levels) - 1)
        for d in range(len(levels) - 1, 0, -1):
            u, w = _expand(ptr, idx, levels[d - 1])
            on = dist[w] == d
            u, w = u[on], w[on]
            np.add.at(delta, u, (sigma[u].astype(np.float64) / sigma[w].astype(np.float64)) * (1.0 + delta[w]))
        res.dist.append(dist)
        res.sigma.append(sigma)
        res.delta.append(delta)
        got = dist >= 0
        res.reached |= got
        add = delta.copy()
        add[s] = 0.0
        res.sums += add
    return res


def rtol(n, row_ptr, src, res):
    """The comparison rule of the GPU tests: 4 * 2^-53 * (L (D + 4) + S + 3) with L the deepest level, D the largest out-degree and S
    the source count - sums of non-negative terms, one rounding per operation along the longest chain, doubled for the restatement's
    own error and again for second-order terms."""
    outdeg = np.bincount(np.asarray(src, dtype=np.int64), minlength=n) if len(src) else np.zeros(1, dtype=np.int64)
    return 4.0 * 2.0 ** -53 * (res.max_dist * (int(outdeg.max()) + 4) + len(res.sources) + 3)
