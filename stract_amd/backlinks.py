"""Mirror of HostBacklinksQuery::new(node).with_limit(EdgeLimit::Limit(L)) (crates/core/src/webgraph/query/backlink.rs:230-360) on the
GPU library (hb_links_set_keys / hb_backlinks).

set_link_keys() / set_link_keys_from_ranks() give the loaded graph its order keys - the harmonic rank of every host, which is what
sort_score orders one node's backlinks by - and build the dense order that stays on the device; host_backlinks() answers a batch of
queries (RemoteWebgraph::batch_search) with the first `limit` in-neighbours of every queried host in the order (key, NodeID).
include/hyperball.h states the definitions and the defined differences.
"""
import numpy as np

from . import _lib
from .harmonic import ids_from_ints


def _ids(nodes):
    """a U128 array, or a sequence of node ints -> U128 array"""
    if isinstance(nodes, np.ndarray) and nodes.dtype == _lib.U128:
        return np.ascontiguousarray(nodes)
    return ids_from_ints([int(v) for v in nodes])


def set_link_keys(ctx, ids, keys):
    """hb_links_set_keys with a list: ids (U128 array or node ints) and their uint64 keys; a node that is not listed has 2^64 - 1.
    -> the stats"""
    return ctx.links_set_keys(_ids(ids), np.ascontiguousarray(keys, dtype=np.uint64))


def set_link_keys_from_ranks(ctx):
    """hb_links_set_keys(HB_LINKS_KEYS_FROM_RANKS): key = the harmonic rank of the context's live result (hb_run / hb_sampled_harmonic)"""
    return ctx.links_set_keys(from_ranks=True)


def host_backlinks(ctx, nodes, limit, keep_self=False):
    """The first `limit` backlinks of every node of `nodes` (U128 array or node ints), best (key, NodeID) first.
    -> (offsets, ids, keys, degrees): the list of query i is ids[offsets[i]:offsets[i + 1]] with its keys beside it, degrees[i] the
    whole in-degree of the node (self link excluded unless keep_self)."""
    ctx.backlinks(_ids(nodes), limit, flags=_lib.HB_LINKS_KEEP_SELF if keep_self else 0)
    return ctx.links_copy()
