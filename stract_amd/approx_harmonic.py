"""Mirror of ApproxHarmonic (crates/core/src/webgraph/centrality/approx_harmonic.rs:35-89) on the GPU library (hb_sampled_harmonic).

build() runs the sampled BFS on the page graph (every edge record followed: HB_FLAG_ALL_RELS, as ForwardlinksQuery does) and writes the
`harmonic` / `harmonic_rank` stores under `output` (the second store build_approx_harmonic writes).  The sample is seeded (the reference
draws it with thread_rng); `num_nodes` is the caller's estimate of N (the reference's HyperLogLog<2048> over page_nodes(),
approx_harmonic.rs:41-46) - None = the exact node count of the graph.
"""
import os

from . import _lib
from .harmonic import ids_to_ints


class ApproxHarmonic:
    def __init__(self, ids, vals, stats=None):
        self._ids = ids
        self._vals = vals
        self.stats = stats or {}
        self._map = None

    @classmethod
    def build(cls, graph, output, seed, num_nodes=None, **ctx_kwargs):
        """approx_harmonic.rs:40-89.  graph: page-level edge records (host_edges() / host_nodes() as in harmonic.EdgeListGraph)."""
        flags = ctx_kwargs.pop("flags", 0) | _lib.HB_FLAG_ALL_RELS
        with _lib.Context(flags=flags, **ctx_kwargs) as ctx:
            ctx.load_edges(graph.host_edges(), graph.host_nodes())
            st = ctx.sampled_harmonic(seed=seed, num_nodes=num_nodes or 0)
            ids, vals = ctx.results()
            if output is not None:
                os.makedirs(output, exist_ok=True)
                ctx.store_harmonic(str(output))
            return cls(ids, vals, st)

    def get(self, node):
        """approx_harmonic.rs:84: Some(centrality) or None."""
        if self._map is None:
            self._map = dict(zip(ids_to_ints(self._ids), self._vals.tolist()))
        if not isinstance(node, int):
            node = (int(node["hi"]) << 64) | int(node["lo"])
        return self._map.get(node)

    def iter(self):
        """approx_harmonic.rs:88: (NodeID, centrality) in ascending NodeID order."""
        return zip(ids_to_ints(self._ids), self._vals.tolist())

    def len(self):
        return len(self._vals)

    __len__ = len
