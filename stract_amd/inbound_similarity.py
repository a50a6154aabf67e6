"""Mirror of Scorer (crates/core/src/ranking/inbound_similarity.rs:61-138) on the GPU library (hb_inbound_similarity).

    s = Scorer.new(ctx, liked, disliked, normalized, limit)   ctx: a Context with the host graph loaded; liked / disliked: NodeIDs as ints
    s.set_self_score(x)                                Scorer::set_self_score
    s.score(ids)                                       Scorer::score for the given hosts (float64 array; unknown hosts: empty BitVec)
    s.score_all()                                      (ids, scores) of every host of the graph, ascending NodeID
    s.top(k, skip_anchors=False)                       (ids, scores) of the k best hosts: score descending, ties by NodeID descending
                                                       (similar_hosts.rs:182-191; skip_anchors: :163)

The reference builds one BitVec per host it is asked about from at most 512 fetched backlinks (searcher/api/mod.rs:199-216:
EdgeLimit::Limit(512)); here every host of the loaded graph is scored at once.  limit=512 is the reference's value: every BitVec, the
anchors' included, then holds the 512 best backlinks in the order (key, NodeID) of the context's current key set (Context.links_set_keys),
self links skipped.  limit=0, the default, takes whole in-lists (include/hyperball.h names the differences).  The device call runs
lazily, once per setting.
"""
from .harmonic import ids_from_ints, ids_to_ints


class Scorer:
    def __init__(self, ctx, liked, disliked, normalized, limit=0):
        self.ctx = ctx
        self.liked = [int(x) for x in liked]
        self.disliked = [int(x) for x in disliked]
        self.normalized = bool(normalized)
        self.limit = int(limit)
        self.self_score = None
        self.mode = None
        self.stats = None

    @classmethod
    def new(cls, ctx, liked, disliked, normalized=False, limit=0):
        return cls(ctx, liked, disliked, normalized, limit)

    def set_self_score(self, self_score):
        self.self_score = float(self_score)
        self.stats = None

    def _run(self):
        if self.stats is None:
            self.stats = self.ctx.inbound_similarity(ids_from_ints(self.liked), ids_from_ints(self.disliked), normalized=self.normalized,
                                                     self_score=self.self_score, mode=self.mode, limit=self.limit)
        return self.stats

    def score(self, ids):
        self._run()
        return self.ctx.similarity_lookup(ids_from_ints([int(i) for i in ids]))

    def score_all(self):
        self._run()
        return ids_to_ints(self.ctx.graph()[0]), self.ctx.similarity_all()

    def top(self, k, skip_anchors=False):
        self._run()
        ids, vals = self.ctx.similarity_top(k, skip_anchors=skip_anchors)
        return ids_to_ints(ids), vals
