"""Host restatement of ShortestPaths (crates/core/src/webgraph/shortest_path.rs:26-227) for the distance tests.

- dijkstra: tests/sample_ref.dijkstra_multi (the literal heap version with the u8 rule `cost + 1 < 255` and the early return when a
  popped cost exceeds max_dist) over a CSR by destination in sid indexing: forward over the out-neighbour lists, reversed over the
  CSR rows themselves (the in-neighbours);
- bfs: the same map by a numpy frontier BFS, for graphs of C2 size.  tests/test_distances.py checks that the two agree on the small
  graphs before the C2 case trusts it.

Both return a uint8 array of n distances, 255 = absent from the reference's map.
"""
import numpy as np

from tests import sample_ref

UNREACHED = 255


def _to_array(n, dmap):
    out = np.full(n, UNREACHED, dtype=np.uint8)
    for v, d in dmap.items():
        assert 0 <= d < UNREACHED
        out[v] = d
    return out


def dijkstra(n, row_ptr, src, sources, reversed=False, max_dist=None):
    """sources: sids (unknown sources are the caller's business: they have no sid).  max_dist None = to exhaustion."""
    if reversed:
        rp = [int(x) for x in row_ptr]
        s = [int(x) for x in src]
        edges = lambda v: s[rp[v]:rp[v + 1]]
    else:
        out = sample_ref.out_lists(n, row_ptr, src)
        edges = lambda v: out[v]
    return _to_array(n, sample_ref.dijkstra_multi([int(x) for x in sources], edges, max_dist))


def bfs(n, row_ptr, src, sources, reversed=False, max_dist=None):
    """Frontier BFS with the same rules: level d = 1 .. min(max_dist + 1, 254); a node first seen at level d gets d."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    frm, to = (dst, src) if reversed else (src, dst)  # an edge carries the frontier from `frm` to `to`
    dist = np.full(n, UNREACHED, dtype=np.uint8)
    sources = np.asarray(sorted(set(int(x) for x in sources)), dtype=np.int64)
    if not len(sources):
        return dist
    dist[sources] = 0
    in_front = np.zeros(n, dtype=bool)
    in_front[sources] = True
    last = 254 if max_dist is None else min(int(max_dist) + 1, 254)
    for d in range(1, last + 1):
        hit = to[in_front[frm]]
        new = np.zeros(n, dtype=bool)
        new[hit] = True
        new &= dist == UNREACHED
        if not new.any():
            break
        dist[new] = d
        in_front = new
    return dist
