"""Mirror of the InboundScorer ranking stage (crates/core/src/ranking/pipeline/scorers/inbound_similarity.rs:38-54) on the GPU
library (hb_score_hosts).

    s = InboundScorer.new(ctx, liked, disliked, normalized=False, limit=512)    ctx: a Context with the host graph loaded
    s.set_self_score(x)                         Scorer::set_self_score
    s.compute(host_ids)                         the InboundSimilarity signal value of every page of a result list, by its host id
                                                (float64 array, caller order; the stage takes at most 300 pages)
    compute_many(ctx, searches, limit=512)      several searches in one device call: [(liked, disliked, host_ids)] -> [float64 array]

The searcher builds Scorer::new(webgraph, liked, disliked, false) for a query with host rankings (searcher/api/mod.rs:467-501) and fetches
one BitVec per UNIQUE host of the initial results from EdgeLimit::Limit(512) backlinks (:411-465, :199-216); the stage then calls
Scorer::score(host, inbound) per page.  Here the unique hosts of all searches of a call are looked up once on the device, and the work
is proportional to (result hosts + liked + disliked) x limit - no walk of the graph (stract_amd.inbound_similarity.Scorer scores every
host of the graph).  The lists follow the context's current key set (Context.links_set_keys).
"""
import numpy as np

from .harmonic import ids_from_ints


def _request(liked, disliked, hosts, normalized, self_score):
    return dict(liked=ids_from_ints([int(x) for x in liked]), disliked=ids_from_ints([int(x) for x in disliked]), nodes=ids_from_ints(hosts),
                normalized=bool(normalized), self_score=self_score)


def _unique(host_ids):
    hosts = [int(h) for h in host_ids]
    unique = sorted(set(hosts))
    place = {h: i for i, h in enumerate(unique)}
    return unique, np.array([place[h] for h in hosts], dtype=np.int64)


def compute_many(ctx, searches, limit=512, normalized=False, self_score=None):
    """searches: [(liked, disliked, host_ids)]; returns (one float64 array per search in the order of its host_ids, the stats)"""
    uniq = [_unique(hosts) for _, _, hosts in searches]
    stats = ctx.score_hosts([_request(liked, disliked, u, normalized, self_score) for (liked, disliked, _), (u, _) in zip(searches, uniq)], limit=limit)
    return [scores[where] for scores, (_, where) in zip(ctx.score_copy(), uniq)], stats


class InboundScorer:
    def __init__(self, ctx, liked, disliked, normalized=False, limit=512):
        self.ctx = ctx
        self.liked = [int(x) for x in liked]
        self.disliked = [int(x) for x in disliked]
        self.normalized = bool(normalized)
        self.limit = int(limit)
        self.self_score = None
        self.stats = None

    @classmethod
    def new(cls, ctx, liked, disliked, normalized=False, limit=512):
        return cls(ctx, liked, disliked, normalized, limit)

    def set_self_score(self, self_score):
        self.self_score = float(self_score)

    def compute(self, host_ids):
        (out,), self.stats = compute_many(self.ctx, [(self.liked, self.disliked, host_ids)], self.limit, self.normalized, self.self_score)
        return out
