"""Mirror of the ShortestPaths trait (crates/core/src/webgraph/shortest_path.rs:26-227) on the GPU library (hb_distances).

    raw_distances(source)                          dijkstra_multi over forward links, to exhaustion
    raw_distances_with_max(source, max_dist)       ... returning when a cost above max_dist is popped
    raw_reversed_distances(source)                 the same over backlinks: the distance from every node TO the source
    raw_reversed_distances_with_max(source, max_dist)

Each returns {NodeID int: distance} like the reference's BTreeMap<NodeID, u8> (iteration order = ascending NodeID).  As in the
reference's raw maps, the source itself is always present with distance 0 - also when it is no node of the graph
(dijkstra_multi inserts it before it looks at any edge, shortest_path.rs:71-74).

distances() / reversed_distances() are the reference's Node-keyed forms: there every id goes through Id2NodeQuery and ids the graph
does not know are dropped (shortest_path.rs:106-120; webgraph/tests.rs:104-118), so an unknown source gives an EMPTY map.  Node names
are not part of the loaded graph, so these two return the same NodeID-keyed map, without the unknown source.

The graph follows every edge record (HB_FLAG_ALL_RELS), as the forward / backlink queries do.  The granularity argument of the trait
is the graph that was loaded: host-level records, or page-level ones (webgraph.load_webgraph(..., page_graph=True)).
"""
from . import _lib
from .harmonic import ids_from_ints, ids_to_ints


def _as_int(node):
    if isinstance(node, int):
        return node
    return (int(node["hi"]) << 64) | int(node["lo"])


class ShortestPaths:
    def __init__(self, ctx, owns_ctx=False):
        self.ctx = ctx
        self._owns = owns_ctx
        self.stats = {}

    @classmethod
    def from_graph(cls, graph, **ctx_kwargs):
        """graph: edge records as in harmonic.EdgeListGraph (host_edges() / host_nodes())."""
        flags = ctx_kwargs.pop("flags", 0) | _lib.HB_FLAG_ALL_RELS
        ctx = _lib.Context(flags=flags, **ctx_kwargs)
        try:
            ctx.load_edges(graph.host_edges(), graph.host_nodes())
        except Exception:
            ctx.close()
            raise
        return cls(ctx, owns_ctx=True)

    def close(self):
        if self._owns:
            self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _run(self, source, reversed, max_dist, keep_unknown_source):
        src = _as_int(source)
        ids, dist, self.stats = self.ctx.distances(ids_from_ints([src]), reversed=reversed, max_dist=max_dist)
        out = dict(zip(ids_to_ints(ids), dist.tolist()))
        if keep_unknown_source and self.stats["unknown_sources"]:
            out[src] = 0
            out = dict(sorted(out.items()))
        return out

    def raw_distances(self, source):
        return self._run(source, False, None, True)

    def raw_distances_with_max(self, source, max_dist):
        return self._run(source, False, max_dist, True)

    def raw_reversed_distances(self, source):
        return self._run(source, True, None, True)

    def raw_reversed_distances_with_max(self, source, max_dist):
        return self._run(source, True, max_dist, True)

    def distances(self, source):
        return self._run(source, False, None, False)

    def reversed_distances(self, source):
        return self._run(source, True, None, False)
