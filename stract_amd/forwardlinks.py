"""Mirror of HostForwardlinksQuery::new(node).with_limit(EdgeLimit::Limit(L)) (crates/core/src/webgraph/query/forwardlink.rs:183-330)
on the GPU library (hb_forwardlinks): the first `limit` out-neighbours of every queried host in the order (key, NodeID), the order
that backlinks.set_link_keys() / set_link_keys_from_ranks() gave the loaded graph.  include/hyperball.h states the definitions and the
defined differences.
"""
from . import _lib
from .backlinks import _ids, set_link_keys, set_link_keys_from_ranks  # noqa: F401  (one key set serves both directions)


def host_forwardlinks(ctx, nodes, limit, keep_self=False):
    """The first `limit` forward links of every node of `nodes` (U128 array or node ints), best (key, NodeID) first.
    -> (offsets, ids, keys, degrees): the list of query i is ids[offsets[i]:offsets[i + 1]] with its keys beside it, degrees[i] the
    whole out-degree of the node (self link excluded unless keep_self)."""
    ctx.forwardlinks(_ids(nodes), limit, flags=_lib.HB_LINKS_KEEP_SELF if keep_self else 0)
    return ctx.links_copy()
