"""Mirror of SimilarHostsFinder::find_similar_hosts (crates/core/src/similar_hosts.rs:54-272) on the GPU library (hb_similar_hosts).

The library answers scored_nodes - the co-citation candidates of the liked hosts, scored by the inbound similarity of their
512-backlink BitVecs, best first; this class does what stays with the caller: the reference's `orig_limit` / `limit + len + 30`
arithmetic, the removal of the liked hosts' root domains through a callback, and take(orig_limit).  The order keys are the ones
backlinks.set_link_keys() / set_link_keys_from_ranks() gave the loaded graph.  include/hyperball.h states the definitions."""
from . import _lib
from .backlinks import _ids


def _int(idrec):
    return (int(idrec["hi"]) << 64) | int(idrec["lo"])


class SimilarHostsFinder:
    def __init__(self, ctx, max_similar_hosts=1000):
        self.ctx = ctx
        self.max_similar_hosts = int(max_similar_hosts)
        self.stats = {}

    def find_similar_hosts(self, nodes, limit, domain_of=None):
        """nodes: the liked hosts (U128 array or node ints, in order); -> [(node int, score)] of at most `limit` hosts, best first.
        domain_of(node int) -> the host's root domain (anything hashable) or None; None for the argument = no filter.  As in the
        reference (similar_hosts.rs:211-218, 250-270) a host is dropped when its root domain is that of a LIKED host, or when it
        has none; two results of one other domain both stay."""
        ids = _ids(nodes)
        orig_limit = min(int(limit), self.max_similar_hosts)
        want = min(orig_limit + len(ids) + 30, 1024)  # (the library's range; the reference asks for limit + len + 30)
        if orig_limit < 1 or not len(ids):
            return []
        self.stats = self.ctx.similar_hosts(ids, want)
        got, scores = self.ctx.similar_copy()
        liked_domains = {domain_of(_int(v)) for v in ids} - {None} if domain_of is not None else set()
        out = []
        for v, s in zip(got, scores.tolist()):
            node = _int(v)
            if domain_of is not None:
                d = domain_of(node)
                if d is None or d in liked_domains:
                    continue
            out.append((node, s))
            if len(out) == orig_limit:
                break
        return out


def similar_flags(spread=False, no_shortcut=False):
    return (_lib.HB_LINKS_SPREAD_ORDS if spread else 0) | (_lib.HB_LINKS_NO_SHORTCUT if no_shortcut else 0)
