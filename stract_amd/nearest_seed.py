"""Mirror of HarmonicNearestSeed (crates/core/src/entrypoint/centrality.rs:126-201) on the GPU library (hb_nearest_seed).

harmonic_nearest_seed() loads the page graph (every edge record followed: HB_FLAG_ALL_RELS, as BacklinksQuery does), gives every node
without an original centrality discount_factor x the centrality of its first backlink's source, and writes the `harmonic` /
`harmonic_rank` stores under `output`.  `ranks` are the order keys of the backlinks: the harmonic rank of every node's host (a node that
is not listed has u64::MAX, as in the reference).  include/hyperball.h states the definitions and the defined differences.
"""
import os

import numpy as np

from . import _lib
from .harmonic import ids_from_ints, ids_to_ints


def _pairs(mapping, dtype):
    """dict {node int: value}, or an (ids, values) pair of arrays / sequences -> (U128 array, values array); None -> (None, None)"""
    if mapping is None:
        return None, None
    if isinstance(mapping, dict):
        keys = list(mapping.keys())
        return ids_from_ints(keys), np.array([mapping[k] for k in keys], dtype=dtype)
    ids, vals = mapping
    if len(ids) and not isinstance(ids, np.ndarray):
        ids = ids_from_ints([int(i) for i in ids])
    return np.ascontiguousarray(ids, dtype=_lib.U128), np.ascontiguousarray(vals, dtype=dtype)


class NearestSeed:
    """The result of one hb_nearest_seed call on a context that holds the graph."""

    def __init__(self, ctx, stats):
        self.ctx = ctx
        self.stats = stats

    @classmethod
    def run(cls, ctx, original=None, ranks=None, discount_factor=0.5, rounds=0, from_image=False):
        """original: {node: centrality} or (ids, vals), or from_image=True for the context's live result; ranks: {node: key} or (ids, keys)"""
        orig_ids, orig_vals = _pairs(original, np.float64)
        key_ids, keys = _pairs(ranks, np.uint64)
        return cls(ctx, ctx.nearest_seed(orig_ids, orig_vals, key_ids, keys, discount_factor=discount_factor, rounds=rounds, from_image=from_image))

    def arrays(self):
        """(ids ascending, values) of the nodes that have a value"""
        return self.ctx.nearest_seed_copy()

    def all(self):
        """one value per node in ascending-NodeID order, -1.0 = none"""
        return self.ctx.nearest_seed_all()

    def top(self, k):
        """the first k rows of harmonic.csv: (node ints, values), value descending, ties by NodeID ascending"""
        ids, vals = self.ctx.nearest_seed_top(k)
        return ids_to_ints(ids), vals

    def seeds(self):
        """{node: seed node} for every node that has a seed"""
        seed, has = self.ctx.nearest_seed_seeds()
        nodes = ids_to_ints(self.ctx.graph()[0])
        seeds = ids_to_ints(seed)
        return {v: s for v, s, h in zip(nodes, seeds, has.tolist()) if h}

    def store(self, output):
        """store_harmonic (centrality/mod.rs:72-114) of the pairs: rank = position by (value descending, NodeID ascending)"""
        ids, vals = self.arrays()
        order = np.lexsort((np.arange(len(vals)), -vals))  # (the ids ascend with the index)
        ranks = np.empty(len(vals), dtype=np.uint64)
        ranks[order] = np.arange(len(vals), dtype=np.uint64)
        os.makedirs(output, exist_ok=True)
        _lib.store_harmonic(str(output), ids, vals, ranks)


def harmonic_nearest_seed(graph, original, ranks=None, discount_factor=0.5, output=None, rounds=0, **ctx_kwargs):
    """centrality.rs:126-201.  graph: page-level edge records (host_edges() / host_nodes() as in harmonic.EdgeListGraph); original: the
    original_centrality pairs; ranks: the order keys.  -> (ids ascending, values, stats)."""
    flags = ctx_kwargs.pop("flags", 0) | _lib.HB_FLAG_ALL_RELS
    with _lib.Context(flags=flags, **ctx_kwargs) as ctx:
        ctx.load_edges(graph.host_edges(), graph.host_nodes())
        res = NearestSeed.run(ctx, original, ranks, discount_factor=discount_factor, rounds=rounds)
        ids, vals = res.arrays()
        if output is not None:
            res.store(output)
        return ids, vals, res.stats
