"""Host restatement of ApproxHarmonic (crates/core/src/webgraph/centrality/approx_harmonic.rs:40-89) for the sampled-harmonic tests.

- dijkstra_multi: shortest_path.rs:57-103, literally (heap, early return when a POPPED cost exceeds max_dist);
- bfs_histogram: the same distances as a numpy bit-parallel BFS (512 sources per uint64 x 8 row), for graphs of C2 size;
- values: the definition of include/hyperball.h (f64 sum of c_d * w_d, d ascending, then through f32);
- f32_loop: the reference's own sequential f32 accumulation (approx_harmonic.rs:60-72);
- sample_sids: the seeded sampler (Floyd's algorithm driven by splitmix64).
"""
import heapq
import math

import numpy as np

MASK64 = (1 << 64) - 1


def dijkstra_multi(sources, out_edges, max_dist):
    """shortest_path.rs:57-103: {node: dist}; out_edges(v) -> iterable of targets."""
    distances = {}
    queue = []
    for s in sources:
        heapq.heappush(queue, (0, s))
        distances[s] = 0
    while queue:
        cost, v = heapq.heappop(queue)
        if cost > distances.get(v, 255):
            continue
        if max_dist is not None and cost > max_dist:
            return distances
        for t in out_edges(v):
            if cost + 1 < distances.get(t, 255):
                heapq.heappush(queue, (cost + 1, t))
                distances[t] = cost + 1
    return distances


def out_lists(n, row_ptr, src):
    """out-neighbour lists from a CSR by destination (sid indexing)."""
    out = [[] for _ in range(n)]
    for v in range(n):
        for k in range(int(row_ptr[v]), int(row_ptr[v + 1])):
            out[int(src[k])].append(v)
    return out


def dijkstra_histogram(n, row_ptr, src, sources, max_dist):
    """c_d(v), d = 1 .. max_dist + 1, as (n, max_dist + 1) uint16, from one dijkstra_multi per source."""
    out = out_lists(n, row_ptr, src)
    D = max_dist + 1
    hist = np.zeros((n, D), dtype=np.uint16)
    for s in sources:
        for v, d in dijkstra_multi([int(s)], lambda u: out[u], max_dist).items():
            if d == 0:
                continue  # approx_harmonic.rs:63
            assert d <= D
            hist[v, d - 1] += 1
    return hist


def bfs_histogram(n, row_ptr, src, sources, max_dist):
    """The same histogram by a bit-parallel BFS over the in-edge CSR, 512 sources per batch."""
    D = max_dist + 1
    hist = np.zeros((n, D), dtype=np.uint16)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    starts = row_ptr[:-1]
    nonempty = row_ptr[1:] > starts
    safe = np.minimum(starts, max(len(src) - 1, 0))
    sources = np.asarray(sources, dtype=np.int64)
    for b0 in range(0, len(sources), 512):
        batch = sources[b0:b0 + 512]
        cur = np.zeros((n, 8), dtype=np.uint64)
        for i, s in enumerate(batch):
            cur[s, i >> 6] |= np.uint64(1 << (i & 63))
        for d in range(1, D + 1):
            nxt = cur.copy()
            if len(src):
                for col in range(8):
                    g = cur[src, col]
                    red = np.bitwise_or.reduceat(g, safe)
                    red[~nonempty] = 0
                    nxt[:, col] |= red
            new = nxt & ~cur
            cnt = np.zeros(n, dtype=np.int64)
            for col in range(8):
                cnt += np.unpackbits(np.ascontiguousarray(new[:, col]).view(np.uint8).reshape(n, 8), axis=1).sum(axis=1, dtype=np.int64)
            hist[:, d - 1] += cnt.astype(np.uint16)
            if not cnt.any():
                break
            cur = nxt
    return hist


def weights(num_nodes, k_req, levels):
    """w_d = (1.0f / d) * norm, norm = N / (k * (N - 1)), all f32 (approx_harmonic.rs:57,69)."""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = f(num_nodes) / (f(k_req) * (f(num_nodes) - f(1.0)))
        return [f(f(1.0) / f(d)) * norm for d in range(1, levels + 1)]


def values(hist, num_nodes, k_req):
    """value(v) = (double)(float)S(v), S = sum over d ascending with c_d > 0 of (double)c_d * (double)w_d; NaN where no source reached v."""
    w = weights(num_nodes, k_req, hist.shape[1])
    out = np.full(hist.shape[0], np.nan)
    for v in np.nonzero(hist.sum(axis=1))[0]:
        s = 0.0
        for d in range(hist.shape[1]):
            c = int(hist[v, d])
            if c:
                s += float(c) * float(w[d])
        out[v] = float(np.float32(s))
    return out


def f32_loop(hist, num_nodes, k_req):
    """approx_harmonic.rs:60-72 sequentially: one f32 `+= (1.0 / dist) * norm` per (source, target) pair, in d order."""
    w = weights(num_nodes, k_req, hist.shape[1])
    out = np.full(hist.shape[0], np.nan)
    for v in np.nonzero(hist.sum(axis=1))[0]:
        acc = np.float32(0.0)
        for d in range(hist.shape[1]):
            for _ in range(int(hist[v, d])):
                acc = np.float32(acc + w[d])
        out[v] = float(acc)
    return out


def default_k(num_nodes, eps=0.3):
    """approx_harmonic.rs:49 with Rust's saturating cast."""
    if num_nodes <= 1:
        return 0
    return int(math.ceil(math.log2(float(num_nodes)) / (eps * eps)))


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, z ^ (z >> 31)


def sample_sids(n, row_ptr, src, seed, k):
    """Candidates = sids with an out-edge (ascending); Floyd: for i in C-K .. C-1, j = next() % (i + 1); sorted chosen sids."""
    outdeg = np.bincount(np.asarray(src, dtype=np.int64), minlength=n) if len(src) else np.zeros(n, dtype=np.int64)
    cand = np.nonzero(outdeg)[0]
    C = len(cand)
    K = min(k, C)
    chosen = set()
    state = seed & MASK64
    for i in range(C - K, C):
        state, r = splitmix64(state)
        j = r % (i + 1)
        chosen.add(i if j in chosen else j)
    return cand[sorted(chosen)]
