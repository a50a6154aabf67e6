"""Mirror of Betweenness (crates/core/src/webgraph/centrality/betweenness.rs:151-172) on the GPU library (hb_betweenness).

    Betweenness.calculate(graph)      Brandes' algorithm from every node of the graph (the reference takes up to 100 000 host nodes;
                                      a larger graph needs `sources`, see include/hyperball.h)
      .centrality                     {NodeID int: value}: sum of the dependencies over the sources / (S (S - 1)), ascending NodeID
      .max_dist                       the largest distance found from any source

The reference keys its map by Node (Id2NodeQuery per id, betweenness.rs:133-141); node names are not part of the loaded graph, so the
keys here are the NodeIDs.  The graph follows every edge record (HB_FLAG_ALL_RELS), as the ForwardlinksQuery of betweenness.rs:73-75
does.
"""
from . import _lib
from .harmonic import ids_from_ints, ids_to_ints


class Betweenness:
    def __init__(self, centrality, max_dist, stats=None):
        self.centrality = centrality
        self.max_dist = max_dist
        self.stats = stats or {}

    @classmethod
    def from_context(cls, ctx, sources=None, mode=None):
        """ctx: a Context with a loaded graph; sources: node ids as ints (None = every node)."""
        src = None if sources is None else ids_from_ints([int(s) for s in sources])
        ids, vals, st = ctx.betweenness(src, mode=mode)
        return cls(dict(zip(ids_to_ints(ids), vals.tolist())), int(st["max_dist"]), st)

    @classmethod
    def from_graph(cls, graph, sources=None, **ctx_kwargs):
        """graph: edge records as in harmonic.EdgeListGraph (host_edges() / host_nodes())."""
        flags = ctx_kwargs.pop("flags", 0) | _lib.HB_FLAG_ALL_RELS
        with _lib.Context(flags=flags, **ctx_kwargs) as ctx:
            ctx.load_edges(graph.host_edges(), graph.host_nodes())
            return cls.from_context(ctx, sources)

    @classmethod
    def calculate(cls, graph, **ctx_kwargs):
        return cls.from_graph(graph, **ctx_kwargs)
