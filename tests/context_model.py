"""One model of a HyperBall context for the state tests (tests/test_context_state.py, tools/diff_fuzz.py --mode context): what
include/hyperball.h and DESIGN.md section 18 say a context holds - the loaded graph, run_open, rows, image, the resident key set, the
limit of the cached cut lists and, for every operator, whether its result is live - and one table of operations over every call family
of the context.  An operation has three members: draw(rng, world) -> args or None, model(world, args) (the state change, and the counts
of the conditions of DESIGN.md section 36), device(handles, world, args) (the call on the library, compared as the operator's own suite
compares it).

The model adds no arithmetic of its own.  Every expected value comes from what the sibling tests use: oracle/hbo.py for hb_run /
hb_begin / hb_step / hb_finish, and the helpers of tests/test_sampled_harmonic.py, test_distances.py, test_betweenness.py,
test_similarity.py, test_limited_similarity.py, test_nearest_seed.py, test_links.py, test_forwardlinks.py, test_similar_hosts.py and
test_score_hosts.py (each over its tests/*_ref.py) for the operators, with the argument draws of tests/operator_cases.py.  What the
sequences are after is what a call leaves for the NEXT one: holders that never shrink, the key set and its orders, the cached cut lists,
the row -> readers transpose, the result image, the shared rows.  So after every refusal, after every sixth operation and at the end
every reader of every operator is called, each C entry point in a call of its own: of a live result they must read byte for byte what
they read when it was made, of a result that is gone each of them, asked alone, must refuse with HB_ERR_INVALID.

`python -m tests.context_model --seeds ...` counts the conditions (a) .. (k) from the model alone (no library is loaded)."""
import argparse
import collections
import functools
import glob
import json
import os
import sys
import tempfile

import numpy as np

from tests import graphs
from tests import operator_cases as oc

COUNTS = (0, 1, 3, 17, 64, 65, 300)  # queries of a call: they fall as often as they rise
N_OPS = 72  # operations of one sequence
COMPARE_EVERY = 6
MAX_DROPPED, MAX_REFUSED = 0.05, 0.15
BORROWERS = ("sampled", "betweenness", "similarity")
NEWER = ("nearest_seed", "links_set_keys", "backlinks", "forwardlinks", "similar_hosts", "score_hosts")
OPERATORS = ("sampled", "distances", "betweenness", "similarity") + NEWER  # the ten; hb_inbound_similarity with limit 0 and with a cutting limit
KEY_READERS = ("backlinks", "forwardlinks", "similar_hosts", "score_hosts", "similarity_cut")  # they read the resident key set, in holders that only grow
CHAINS = [(b, n, d) for b in BORROWERS for n in NEWER for d in ("forth", "back")]  # (e): borrower, newer call, run - and the reverse
# the context of a sequence: seed % 6
VARIANTS = [("default", (), 0), ("no_sparse", ("NO_SPARSE",), 0), ("live_first", ("LIVE_FIRST",), 0), ("chunk8", (), 8),
            ("no_sparse_chunk16", ("NO_SPARSE",), 16), ("live_first_chunk4", ("LIVE_FIRST",), 4)]
assert all(c == 0 or c in oc.CHUNKS for _, _, c in VARIANTS)
NEED = {"a_fewer_queries": 10, "a_smaller_limit": 10, "c_reused": 4, "c_after_set_keys": 4, "c_other_limit": 4, "c_after_reload": 4,
        "d_ranks_hyperball": 3, "d_ranks_sampled": 3, "d_ranks_refused": 3, "d_image_hyperball": 3, "d_image_sampled": 3, "d_image_refused": 3,
        "f_smaller_after_all_ten": 3, "f_larger_after_smaller": 3, "g_forward_builds_transpose": 2, "g_forward_reuses_transpose": 2, "g_walk_reuses_forward_built": 2,
        "i_release_with_four_live": 5, "j_live_first": 2, "j_chunk": 2, "k_refusals": 40}
NEED.update({"b_" + op: 3 for op in KEY_READERS})
NEED.update({"e_%s_%s_%s" % c: 1 for c in CHAINS})
NEED.update({"h_" + op: 1 for op in OPERATORS})


def pick(rng, xs):
    xs = list(xs)
    return xs[int(rng.integers(0, len(xs)))]


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------
def _stars():
    """the first `stars` graph of operator_cases.draw_graph with 100 .. 400 hosts and a hub above the default chunk of 64"""
    for k in range(1000):
        _, tuples = oc.draw_graph(np.random.default_rng([36, k]), "stars")
        n = len({x for e in tuples for x in e})
        indeg = collections.Counter(t for _, t in tuples)
        if 100 <= n <= 400 and max(indeg.values()) > 70:
            return tuples
    raise AssertionError("no stars graph")


def _tuples(name):
    from tests import test_reload, test_state
    if name == "empty":
        return []
    if name == "stars":
        return _stars()
    if name == "lcg70":
        return test_state.TUPLES["lcg70"]() + [(5, 5)]
    if name == "lcg70_fringe":
        return test_state.TUPLES["lcg70_fringe_live"]()
    return test_reload._tuples({"lcg300": "A", "lcg300_fringe": "A_fringe"}[name]) + [(7, 7)]


GRAPH_NAMES = ("empty", "lcg70", "lcg70_fringe", "stars", "lcg300", "lcg300_fringe")


class Graph:
    """a graph of the pool: its tuples, its reduced form (ascending ids, in-lists) and what the references need of it, each made once"""

    def __init__(self, name):
        from tests import inbound_similarity_ref as sref
        self.name, self.tuples = name, _tuples(name)
        self.graph = self.ids, self.row_ptr, self.src = graphs.dense_from_tuples(self.tuples)
        self.n = len(self.ids)
        self.ints = sref.id_ints(self.ids)
        indeg = np.diff(np.asarray(self.row_ptr, dtype=np.int64))
        self.hubs = [int(x) for x in np.argsort(-indeg, kind="stable")[:2]] if self.n else []
        self.has_out = np.unique(np.asarray(self.src, dtype=np.int64)).tolist()

    def edges(self):
        from stract_amd import _lib
        from stract_amd.harmonic import EdgeListGraph
        return EdgeListGraph.from_tuples(self.tuples).host_edges() if self.tuples else np.zeros(0, dtype=_lib.EDGE)

    @functools.cached_property
    def fgraph(self):
        from tests import forwardlinks_ref as fref
        return (self.ids,) + fref.out_csr(self.row_ptr, self.src)

    @functools.cached_property
    def bv(self):
        from tests import inbound_similarity_ref as sref
        return sref.bitvecs(*self.graph)

    @functools.cached_property
    def trace(self):
        """the oracle's run: [(registers, kahan, sizes, values, keep) after 0, 1, .. T passes]; hb_step number T reports no change"""
        from oracle import hbo
        out = []
        while True:
            o = hbo.Dense(np.ascontiguousarray(self.ids["lo"]), self.row_ptr, self.src)
            has = True
            for _ in range(len(out)):
                has, _st = o.step(hbo.FRONTIER)
            vals, keep, _k = o.finish()
            out.append((o.registers(), o.kahan(), o.sizes(), vals, keep))
            o.close()
            if not has:
                return out

    @property
    def passes(self):
        return len(self.trace) - 1


@functools.lru_cache(maxsize=None)
def graph(name):
    return Graph(name)


# ---- the world ------------------------------------------------------------------------------------------------------------------------
class World:
    """what a context holds, as the header says it; and the counts of the conditions the sequences must reach"""

    def __init__(self, seed, variant):
        self.seed, self.variant = seed, variant
        self.g = None  # the loaded graph
        self.stream = None  # the graph whose records were appended and neither finalized nor discarded
        self.run_open, self.steps, self.converged = False, 0, False
        self.rows, self.image = "Nobody", None  # image: None, ("HyperBall", passes done) or ("Sampled",)
        self.keys = {}  # the resident key set {id: key}, empty = NodeID order; "ranks" = the ranks of the image it was set from
        self.cut_limit = None  # the limit of the cached cut lists
        self.live = {}  # operator -> what its readers need to know of the live result
        self.counts = collections.Counter()
        self.loads = 0
        self.chains = 0
        self.limited_before = False  # a cutting hb_inbound_similarity ran on an earlier graph
        self.open_runs_done = False
        self.h_pending = []  # the operators refused inside the open run: counted for (h) once that run is finished
        self.reset_load()

    def reset_load(self):
        self.max_queries, self.max_limit = {}, {}
        self.key_epoch, self.epoch_of = 0, {}
        self.ran = set()  # the operators that have run on this graph
        self.transpose_by = None  # NO_SPARSE: who built the row -> readers transpose of this load (ensure_transpose: the first of hb_distances,
        # hb_betweenness and a hb_forwardlinks with a known query; every later one of them reuses it)
        self.limited_here = False
        self.lists_dropped_by = None
        self.lnk_touched = False
        self.last_calls = []  # run and the ten operators in the order they were called on this graph, for (e)

    # -- what a call does, counted --------------------------------------------------------------------------------------------------
    def flags(self):
        from stract_amd import _lib
        f = _lib.HB_FLAG_ALL_RELS
        for name in self.variant[1]:
            f |= getattr(_lib, "HB_FLAG_" + name)
        return f

    def loaded(self, g):
        old = self.g
        if old is not None:
            if g.n < old.n and set(OPERATORS) <= self.ran:
                self.counts["f_smaller_after_all_ten"] += 1
            if g.n > old.n and self.loads >= 1:
                self.counts["f_larger_after_smaller"] += 1
            self.counts["reload_other" if g.name != old.name else "reload_same"] += 1
        self.limited_before = self.limited_before or self.limited_here
        self.g, self.stream = g, None
        self.run_open, self.steps, self.converged = False, 0, False
        self.rows, self.image, self.keys, self.cut_limit, self.live = "Nobody", None, {}, None, {}
        self.h_pending = []
        self.loads += 1
        self.reset_load()

    def called(self, name):
        """a successful call of `run` or of one of the ten operators"""
        op = "similarity" if name == "similarity_cut" else name
        self.ran.add(op)
        self.last_calls.append(op)
        t = tuple(self.last_calls[-3:])
        if len(t) == 3:
            if t[0] in BORROWERS and t[1] in NEWER and t[2] == "run":
                self.counts["e_%s_%s_forth" % t[:2]] += 1
            if t[0] == "run" and t[1] in NEWER and t[2] in BORROWERS:
                self.counts["e_%s_%s_back" % (t[2], t[1])] += 1

    def holder_call(self, name, queries, limit):
        """(a) a holder never shrinks: a call with fewer queries or a smaller limit than an earlier one of the same operator since the load;
        (b) hb_links_set_keys between two calls of a key-reading operator"""
        if queries < self.max_queries.get(name, 0):
            self.counts["a_fewer_queries"] += 1
        if limit < self.max_limit.get(name, 0):
            self.counts["a_smaller_limit"] += 1
        self.max_queries[name] = max(queries, self.max_queries.get(name, 0))
        self.max_limit[name] = max(limit, self.max_limit.get(name, 0))
        if name in self.epoch_of and self.epoch_of[name] < self.key_epoch:
            self.counts["b_" + name] += 1
        self.epoch_of[name] = self.key_epoch
        self.lnk_touched = True

    def transpose_used(self, who):
        """(g), in a HB_FLAG_NO_SPARSE context (any other has the sweep passes' transpose from the load on)"""
        if "NO_SPARSE" not in self.variant[1]:
            return
        if self.transpose_by is None:
            self.transpose_by = who
            self.counts["g_forward_builds_transpose"] += who == "forwardlinks"
        elif who == "forwardlinks":
            self.counts["g_forward_reuses_transpose"] += self.transpose_by != "forwardlinks"
        else:
            self.counts["g_walk_reuses_forward_built"] += self.transpose_by == "forwardlinks"

    def n_live(self):
        """the operators whose result is live (the sampled operator by its histogram; hb_backlinks / hb_forwardlinks share one result)"""
        return sum(1 for v in self.live.values() if v)

    def is_live(self, reader):
        if self.g is None:
            return False
        if reader == "image":
            return self.image is not None
        if reader == "state":
            return self.rows == "HyperBall"
        if reader in ("similarity_batch", "similarity_counts"):
            # bloom and len of the last call's lists: gone with the cut lists a limited call read them from (hb_links_set_keys); the counts
            # of its last batch lie in the shared rows
            sim = self.live.get("similarity")
            return bool(sim) and sim["limit"] in (0, self.cut_limit) and (reader == "similarity_batch" or self.rows == "Similarity")
        return bool(self.live.get(reader))


class Handles:
    """the device side of a world: the context, and every live result as the device returned it when it was made"""

    def __init__(self, factory, world):
        self.factory = factory
        self.kw = dict(flags=world.flags(), chunk=world.variant[2])
        self.ctx = factory(**self.kw)
        self.snap = {}
        self.image = None  # (ids, values, ranks) of the live image
        self.fresh = {}
        self.tmp = tempfile.TemporaryDirectory()
        self.stores = 0

    def close(self):
        self.ctx.close()
        self.tmp.cleanup()


def refused(fn, code=None):
    from stract_amd import _lib
    try:
        fn()
    except _lib.HyperballError as e:
        assert e.code == (_lib.HB_ERR_INVALID if code is None else code), e
        return
    raise AssertionError("a call that must be refused was accepted")


# ---- the readers: what a live result reads as, as bytes -------------------------------------------------------------------------------
def _bytes(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def _c(ctx, entry, *args):
    """one call of one C entry point"""
    ctx._check(getattr(ctx.lib, entry)(ctx.h, *args))


def _u64():
    import ctypes
    return ctypes.c_uint64(0)


def _ref(x):
    import ctypes
    return ctypes.byref(x)


def _z(shape, dtype):
    return np.zeros(shape, dtype=dtype)


def _count_copy_all(prefix, dtype, with_all=True):
    """the count / copy / all readers of hb_distance_*, hb_betweenness_*, hb_nearest_seed_*: `k` goes from the count to the copy"""
    from stract_amd import _lib
    P = _lib._ptr

    def count(ctx, w, s):
        k = _u64()
        _c(ctx, prefix + "_count", _ref(k))
        s["k"] = k.value
        return (np.array([k.value]),)

    def copy(ctx, w, s):
        k = s.get("k", 1)
        ids, vals = _z(k, _lib.U128), _z(k, dtype)
        _c(ctx, prefix + "_copy", P(ids), P(vals), k)
        return ids, vals

    def every(ctx, w, s):
        out = _z(ctx.n(), dtype)
        _c(ctx, prefix + "_all", P(out), len(out))
        return (out,)
    return [(prefix + "_count", count), (prefix + "_copy", copy), (prefix + "_all", every)]


def _top(entry, flags=()):
    from stract_amd import _lib
    P = _lib._ptr

    def top(ctx, w, s):
        k = min(5, s.get("k", 5))
        ids, vals, wrote = _z(k, _lib.U128), _z(k, np.float64), _u64()
        _c(ctx, entry, k, *flags, P(ids), P(vals), _ref(wrote))
        return ids[:wrote.value], vals[:wrote.value]
    return (entry, top)


def _readers():
    """result -> [(C entry, one call of it)]: EVERY reader of every operator, one call each, so that each can be asked on its own whether it
    refuses a result that is gone.  A call gets the state `s` of its group (the count a copy needs) and returns arrays."""
    from stract_amd import _lib
    P = _lib._ptr
    U128, f64, u64, u32, u8 = _lib.U128, np.float64, np.uint64, np.uint32, np.uint8

    def result_count(ctx, w, s):
        k = _u64()
        _c(ctx, "hb_result_count", _ref(k))
        s["k"] = k.value
        return (np.array([k.value]),)

    def result_copy(ctx, w, s):
        k = s.get("k", 1)
        ids, vals = _z(k, U128), _z(k, f64)
        _c(ctx, "hb_result_copy", P(ids), P(vals), k)
        return ids, vals

    def result_ranks(ctx, w, s):
        out = _z(s.get("k", 1), u64)
        _c(ctx, "hb_result_ranks", P(out), len(out))
        return (out,)

    def registers(ctx, w, s):
        out = _z((ctx.n(), 64), u8)
        _c(ctx, "hb_debug_copy_registers", P(out))
        return (out,)

    def kahan(ctx, w, s):
        a, b = _z(ctx.n(), f64), _z(ctx.n(), f64)
        _c(ctx, "hb_debug_copy_kahan", P(a), P(b))
        return a, b

    def sizes(ctx, w, s):
        out = _z(ctx.n(), u64)
        _c(ctx, "hb_debug_copy_sizes", P(out))
        return (out,)

    def state_hash(ctx, w, s):
        out = _z(2, u64)
        _c(ctx, "hb_debug_state_hash", P(out))
        return (out,)

    def histogram(ctx, w, s):
        out = _z((ctx.n(), (w.live.get("histogram") or {}).get("levels", 8)), np.uint16)
        _c(ctx, "hb_debug_sample_histogram", P(out))
        return (out,)

    def similarity_all(ctx, w, s):
        out = _z(ctx.n(), f64)
        _c(ctx, "hb_similarity_all", P(out), len(out))
        return (out,)

    def similarity_lookup(ctx, w, s):
        ids = _z(4, U128)  # three nodes (where the graph has them) and an id that is no node
        m = min(3, w.g.n) if w.g is not None else 0
        ids[:m] = w.g.ids[:m] if m else 0
        ids["hi"][m:] = np.uint64(1 << 36)
        out = _z(4, f64)
        _c(ctx, "hb_similarity_lookup", P(ids), 4, P(out))
        return (out,)

    def similarity_batch(counts):
        def read(ctx, w, s):
            n = ctx.n()
            c, bloom, length = _z((n, 16), u32), _z(n, u64), _z(n, u32)
            _c(ctx, "hb_debug_copy_similarity_batch", P(c) if counts else None, P(bloom), P(length))
            return c, bloom, length
        return read

    def seeds(ctx, w, s):
        seed, has = _z(ctx.n(), U128), _z(ctx.n(), u8)
        _c(ctx, "hb_nearest_seed_seeds", P(seed), P(has), len(has))
        return seed, has

    def links_count(ctx, w, s):
        q, e = _u64(), _u64()
        _c(ctx, "hb_links_count", _ref(q), _ref(e))
        s["q"], s["e"] = q.value, e.value
        return (np.array([q.value, e.value]),)

    def links_copy(ctx, w, s):
        q, e = s.get("q", 1), s.get("e", 1)
        off, deg, ids, keys = _z(q + 1, u64), _z(q, u64), _z(e, U128), _z(e, u64)
        _c(ctx, "hb_links_copy", P(off), P(deg), P(ids), P(keys), e)
        return off, deg, ids, keys

    def similar_count(ctx, w, s):
        k = _u64()
        _c(ctx, "hb_similar_count", _ref(k))
        s["k"] = k.value
        return (np.array([k.value]),)

    def similar_copy(ctx, w, s):
        k = s.get("k", 1)
        ids, scores = _z(k, U128), _z(k, f64)
        _c(ctx, "hb_similar_copy", P(ids), P(scores), k)
        return ids, scores

    def similar_candidates(ctx, w, s):
        wrote = _u64()
        if "k" in s:  # (its own size call first; asked about a result that is gone, the one call with room for one entry)
            _c(ctx, "hb_similar_candidates", None, None, 0, _ref(wrote))
        cap = wrote.value if "k" in s else 1
        ids, counts = _z(cap, U128), _z(cap, u64)
        _c(ctx, "hb_similar_candidates", P(ids), P(counts), cap, _ref(wrote))
        return ids[:wrote.value], counts[:wrote.value]

    def score_count(ctx, w, s):
        r, k = _u64(), _u64()
        _c(ctx, "hb_score_count", _ref(r), _ref(k))
        s["r"], s["k"] = r.value, k.value
        return (np.array([r.value, k.value]),)

    def score_copy(ctx, w, s):
        r, k = s.get("r", 1), s.get("k", 1)
        off, scores = _z(r + 1, u64), _z(k, f64)
        _c(ctx, "hb_score_copy", P(off), P(scores), k)
        return off, scores

    return {
        "image": [("hb_result_count", result_count), ("hb_result_copy", result_copy), ("hb_result_ranks", result_ranks), _top("hb_result_top")],
        "state": [("hb_debug_copy_registers", registers), ("hb_debug_copy_kahan", kahan), ("hb_debug_copy_sizes", sizes), ("hb_debug_state_hash", state_hash)],
        "histogram": [("hb_debug_sample_histogram", histogram)],
        "distances": _count_copy_all("hb_distance", u8),
        "betweenness": _count_copy_all("hb_betweenness", f64),
        "similarity": [("hb_similarity_all", similarity_all), _top("hb_similarity_top", (0,)), ("hb_similarity_lookup", similarity_lookup)],
        "similarity_batch": [("hb_debug_copy_similarity_batch (bloom, len)", similarity_batch(False))],
        "similarity_counts": [("hb_debug_copy_similarity_batch (counts)", similarity_batch(True))],
        "nearest_seed": _count_copy_all("hb_nearest_seed", f64) + [_top("hb_nearest_seed_top"), ("hb_nearest_seed_seeds", seeds)],
        "links": [("hb_links_count", links_count), ("hb_links_copy", links_copy)],
        "similar_hosts": [("hb_similar_count", similar_count), ("hb_similar_copy", similar_copy), ("hb_similar_candidates", similar_candidates)],
        "score_hosts": [("hb_score_count", score_count), ("hb_score_copy", score_copy)],
    }


READER_NAMES = ("image", "state", "histogram", "distances", "betweenness", "similarity", "similarity_batch", "similarity_counts", "nearest_seed", "links",
                "similar_hosts", "score_hosts")


def read_live(ctx, w, name):
    """every reader of a live result, in order, as bytes"""
    s, out = {}, ()
    for _entry, call in _readers()[name]:
        out += _bytes(*call(ctx, w, s))
    return out


def refuse_gone(ctx, w, name):
    """every reader of a result that is gone, each asked on its own: each must refuse with HB_ERR_INVALID"""
    for entry, call in _readers()[name]:
        try:
            refused(lambda: call(ctx, w, {}))
        except AssertionError as e:
            raise AssertionError("a result that is gone was served", name, entry) from e


def snapshot(w, h, *readers):
    for r in readers:
        if w.is_live(r):
            h.snap[r] = read_live(h.ctx, w, r)
    if "image" in readers and w.image is not None:
        h.image = h.ctx.results() + (h.ctx.ranks(),)


def compare_all(w, h):
    """every reader of every operator: a live result reads what the device returned when it was made, a result that is gone is refused
    by each of its readers"""
    if h is None:
        return
    for name in READER_NAMES:
        if w.is_live(name):
            assert read_live(h.ctx, w, name) == h.snap[name], ("a live result reads differently", name)
        else:
            refuse_gone(h.ctx, w, name)


# ---- the key set as the references take it ----------------------------------------------------------------------------------------------
def key_items(w, h):
    """[(id, key)] of the resident key set"""
    if w.keys == "ranks":
        from tests import links_ref as lref
        return list(zip(lref.id_ints(h.ranks_image[0]), h.ranks_image[2].tolist()))
    return sorted(w.keys.items())


def key_array(w, h):
    """the key of every sid, u64::MAX = not listed"""
    key = np.full(w.g.n, oc.U64_MAX, dtype=np.uint64)
    index = {v: i for i, v in enumerate(w.g.ints)}
    for v, k in key_items(w, h):
        key[index[v]] = k
    return key


# ---- load -----------------------------------------------------------------------------------------------------------------------------
def _load_graph(rng, w, smaller=False):
    """a reload draws another graph at least as often as the same one; smaller: mostly one with fewer hosts than the loaded one"""
    names = [n for n in GRAPH_NAMES if w.g is None or n != w.g.name]
    less = [n for n in names if w.g is not None and graph(n).n < w.g.n]
    if smaller and less and rng.random() < 0.7:
        return pick(rng, less)
    if w.g is not None and rng.random() < 0.3:
        return w.g.name
    return pick(rng, names)


def load_draw(rng, w, smaller=False):
    name = _load_graph(rng, w, smaller)
    how = pick(rng, ["edges", "dense", "append"]) if name != "empty" else pick(rng, ["edges", "append"])
    cuts = sorted(int(x) for x in rng.integers(0, len(graph(name).tuples) + 1, int(rng.integers(1, 3)))) if how == "append" else []
    return dict(graph=name, how=how, cuts=cuts)


def load_model(w, a):
    w.loaded(graph(a["graph"]))


def _check_loaded(w, h, a):
    ctx, g = h.ctx, w.g
    got = ctx.graph()
    assert all(np.array_equal(x, y) for x, y in zip(got, g.graph)), "the loaded graph"
    if "LIVE_FIRST" in w.variant[1] and "fringe" in g.name:
        live_first, n_live, _ = ctx.plan_live()
        assert live_first and 0 < n_live < g.n
    if g.name == "stars":
        assert ctx.plan()["nv"] > 0, "chunk trees exist"
    # device_bytes after a load: not above a fresh context with this graph (nothing of the earlier graph's operator states is still booked)
    key = (a["graph"], a["how"] if a["how"] != "append" else "edges")
    if key not in h.fresh:
        with h.factory(**h.kw) as other:
            _load(other, g, key[1], [])
            h.fresh[key] = other.stats()["device_bytes"]
    assert ctx.stats()["device_bytes"] <= h.fresh[key], ("device_bytes after the load", ctx.stats()["device_bytes"], h.fresh[key])
    h.snap, h.image = {}, None


def _load(ctx, g, how, cuts):
    if how == "dense":
        ctx.load_dense(*g.graph)
    elif how == "edges":
        ctx.load_edges(g.edges())
    else:
        for part in np.split(g.edges(), cuts):
            ctx.append_edges(part)
        ctx.finalize()


def load_device(h, w, a):
    _load(h.ctx, w.g, a["how"], a["cuts"])
    _check_loaded(w, h, a)


def append_draw(rng, w):
    name = _load_graph(rng, w)
    if name == "empty":
        name = "lcg70"
    return dict(graph=name, cuts=sorted(int(x) for x in rng.integers(0, len(graph(name).tuples) + 1, int(rng.integers(1, 3)))))


def append_model(w, a):
    """hb_append_edges touches the ingest stream alone (hb_api.hip): the loaded graph, rows, image, run_open and every live result stay"""
    w.stream = a["graph"]


def append_device(h, w, a):
    for part in np.split(graph(a["graph"]).edges(), a["cuts"]):
        h.ctx.append_edges(part)


def end_stream_draw(rng, w):
    return dict(how=pick(rng, ["finalize", "discard"]), graph=w.stream)


def end_stream_model(w, a):
    """hb_finalize is a load of the appended records; hb_discard_appended frees the stream and nothing else: the loaded graph and every
    live result stay as they are, and the next hb_append_edges starts an empty stream"""
    if a["how"] == "finalize":
        w.loaded(graph(a["graph"]))
    else:
        w.counts["discarded"] += 1
        w.stream = None


def end_stream_device(h, w, a):
    if a["how"] == "finalize":
        h.ctx.finalize()
        _check_loaded(w, h, dict(a, how="append"))
    else:
        h.ctx._check(h.ctx.lib.hb_discard_appended(h.ctx.h))
        if w.g is not None:
            assert all(np.array_equal(x, y) for x, y in zip(h.ctx.graph(), w.g.graph)), "the loaded graph after hb_discard_appended"


# ---- HyperBall ------------------------------------------------------------------------------------------------------------------------
def _check_state(w, h):
    """registers, Kahan words and sizes against the oracle after w.steps passes"""
    regs, (ks, ke), sizes, _, _ = w.g.trace[min(w.steps, w.g.passes)]
    ctx = h.ctx
    assert np.array_equal(ctx.registers(), regs), "registers"
    s, e = ctx.kahan()
    assert s.tobytes() == ks.tobytes() and e.tobytes() == ke.tobytes(), "Kahan words"
    if w.steps:
        assert np.array_equal(ctx.sizes(), sizes), "sizes"


def _check_image(w, h):
    """the result list against the oracle's after w.image[1] passes, bit for bit"""
    _, _, _, vals, keep = w.g.trace[w.image[1]]
    gids, gvals = h.ctx.results()
    assert np.array_equal(gids, w.g.ids[keep]) and gvals.tobytes() == vals[keep].tobytes(), "the result list"


def run_draw(rng, w):
    return {}


def run_model(w, a):
    w.run_open, w.steps, w.converged, w.rows, w.image = False, w.g.passes, True, "HyperBall", ("HyperBall", w.g.passes)
    w.h_pending = []
    w.called("run")


def run_device(h, w, a):
    st = h.ctx.run()
    assert st["passes"] == w.g.passes, ("passes", st["passes"], w.g.passes)
    _check_image(w, h)
    _check_state(w, h)
    snapshot(w, h, "image", "state")


def begin_draw(rng, w):
    return {}


def begin_model(w, a):
    w.run_open, w.steps, w.converged, w.rows, w.image = True, 0, False, "HyperBall", None
    w.h_pending = []


def begin_device(h, w, a):
    h.ctx.begin()
    _check_state(w, h)
    snapshot(w, h, "state")


def step_draw(rng, w):
    return dict(steps=int(rng.integers(1, 4)))


def step_model(w, a):
    a["has"] = []
    for _ in range(a["steps"]):
        if w.converged:
            break
        w.steps += 1
        w.converged = w.steps >= w.g.passes
        a["has"].append(not w.converged)


def step_device(h, w, a):
    got = [h.ctx.step() for _ in a["has"]]
    assert got == a["has"], ("has_changes", got, a["has"])
    _check_state(w, h)
    snapshot(w, h, "state")


def finish_draw(rng, w):
    return {}


def finish_model(w, a):
    if w.run_open:
        for op in w.h_pending:
            w.counts["h_" + op] += 1
        w.h_pending = []
    w.run_open, w.image = False, ("HyperBall", w.steps)


def finish_device(h, w, a):
    h.ctx.finish()
    _check_image(w, h)
    _check_state(w, h)
    snapshot(w, h, "image", "state")


def image_draw(rng, w):
    return dict(k=pick(rng, [0, 1, 3, 17, 1000]), store=bool(rng.random() < 0.5))


def image_model(w, a):
    pass


def image_device(h, w, a):
    """results, ranks, top(k) and store_harmonic against the image the model says is live (a sampled image counts)"""
    from oracle import hbo
    from stract_amd import _lib
    ctx = h.ctx
    ids, vals = ctx.results()
    ranks = ctx.ranks()
    assert read_live(ctx, w, "image") == h.snap["image"]
    if w.image[0] == "HyperBall":
        _check_image(w, h)
    assert np.array_equal(ranks, hbo.rank_results(vals)), "ranks"
    by_rank = np.argsort(ranks, kind="stable")
    tids, tvals = ctx.top(a["k"])
    kk = min(a["k"], len(vals))
    assert len(tvals) == kk and np.array_equal(tids, ids[by_rank[:kk]]) and tvals.tobytes() == vals[by_rank[:kk]].tobytes(), "top"
    if a["store"]:
        h.stores += 1
        dev, host = os.path.join(h.tmp.name, "dev%d" % h.stores), os.path.join(h.tmp.name, "host%d" % h.stores)
        ctx.store_harmonic(dev)
        _lib.store_harmonic(host, ids, vals, ranks)
        for db in ("harmonic", "harmonic_rank"):  # the files of tests/test_gpu.py's store comparison
            for ext in ("blobs", "bid", "ids", "blm"):
                fa, fb = glob.glob(os.path.join(dev, db, "*." + ext)), glob.glob(os.path.join(host, db, "*." + ext))
                assert len(fa) == len(fb) == (1 if len(ids) else 0), (db, ext)  # (an empty image - hb_finish right behind hb_begin - stores no segment)
                assert not fa or open(fa[0], "rb").read() == open(fb[0], "rb").read(), (db, ext)


# ---- the ten operators ------------------------------------------------------------------------------------------------------------------
def _count(rng, lo=0, hi=300):
    return pick(rng, [c for c in COUNTS if lo <= c <= hi])


def _sources(rng, g, count, pool=None):
    """`count` distinct known sids (as many as there are), the hubs among them"""
    pool = list(range(g.n)) if pool is None else pool
    sids = set(g.hubs[:1]) & set(pool)
    sids |= {pool[int(i)] for i in rng.integers(0, len(pool), count)}
    return sorted(sids)[:max(count, 1)]


def sampled_draw(rng, w):
    srcs = _sources(rng, w.g, _count(rng, 1, 65), w.g.has_out) if rng.random() < 0.7 else None
    return dict(sources=srcs, max_dist=int(pick(rng, [1, 7, 15])), seed=int(rng.integers(0, 1 << 30)), samples=int(pick(rng, [0, 3, 40])) if srcs is None else 0)


def sampled_model(w, a):
    w.rows, w.image = "Sampled", ("Sampled",)
    w.live["histogram"] = dict(levels=a["max_dist"] + 1)
    w.called("sampled")


def sampled_device(h, w, a):
    from tests import test_sampled_harmonic as th
    th._check(h.ctx, sources_sids=a["sources"], max_dist=a["max_dist"], seed=a["seed"], samples=a["samples"])
    snapshot(w, h, "image", "histogram")


def distances_draw(rng, w):
    return dict(sources=_sources(rng, w.g, _count(rng, 1)), reversed=bool(rng.integers(0, 2)), max_dist=pick(rng, [None, 0, 1, 7, 15, 200]),
                mode=pick(rng, [None, None, "top_down", "bottom_up"]))


def distances_model(w, a):
    w.transpose_used("distances")
    w.live["distances"] = True
    w.called("distances")


def distances_device(h, w, a):
    from tests import test_distances as td
    td._check(h.ctx, a["sources"], a["reversed"], a["max_dist"], modes=(a["mode"],), graph=w.g.graph)
    snapshot(w, h, "distances")


def betweenness_draw(rng, w):
    return dict(sources=_sources(rng, w.g, _count(rng, 1, 65)), mode=pick(rng, [None, None, "dense", "sparse"]))


def betweenness_model(w, a):
    w.transpose_used("betweenness")
    w.rows, w.live["betweenness"] = "Brandes", True
    w.called("betweenness")


def betweenness_device(h, w, a):
    from tests import test_betweenness as tb
    tb._check(h.ctx, a["sources"], modes=(a["mode"],), graph=w.g.graph)
    snapshot(w, h, "betweenness")


def similarity_draw(rng, w, cut=None):
    cut = rng.random() < 0.7 if cut is None else cut
    count = _count(rng, 1)
    liked = oc.draw_entries(rng, w.g.ints, count - count // 3)
    limit = 0
    if cut:  # the cached limit again, so that the lists are reused, as often as another one
        limit = w.cut_limit if w.cut_limit and rng.random() < 0.5 else int(pick(rng, oc.LIMITS))
    return dict(liked=liked, disliked=oc.draw_entries(rng, w.g.ints, count // 3), normalized=bool(rng.integers(0, 2)), self_score=pick(rng, [None, 0.25, 3.0]),
                mode=pick(rng, [None, None, "dense", "sparse"]), limit=limit)


def similarity_model(w, a):
    a["reused"] = False
    if a["limit"]:
        w.holder_call("similarity_cut", len(a["liked"]) + len(a["disliked"]), a["limit"])
        if w.cut_limit == a["limit"]:
            w.counts["c_reused"] += 1
            a["reused"] = True
        elif w.lists_dropped_by == "keys":
            w.counts["c_after_set_keys"] += 1
        elif w.cut_limit is not None:
            w.counts["c_other_limit"] += 1
        elif not w.limited_here and w.limited_before:
            w.counts["c_after_reload"] += 1
        w.cut_limit, w.limited_here, w.lists_dropped_by = a["limit"], True, None
    w.rows, w.live["similarity"] = "Similarity", dict(limit=a["limit"])
    w.called("similarity_cut" if a["limit"] else "similarity")


def similarity_device(h, w, a):
    ctx, g = h.ctx, w.g
    kw = dict(normalized=a["normalized"], self_score=a["self_score"], modes=(a["mode"],))
    if a["limit"]:
        from tests import test_limited_similarity as tl
        _, (st,), _ = tl._check(ctx, g.graph, key_items(w, h), a["limit"], a["liked"], a["disliked"], **kw)
        if a["reused"]:
            assert st["ms_lists"] == 0.0, "the cached cut lists were built again"
    else:
        from tests import test_similarity as ts
        ts._check(ctx, g.graph, g.bv, a["liked"], a["disliked"], **kw)
    snapshot(w, h, "similarity", "similarity_batch", "similarity_counts")


def nearest_seed_draw(rng, w):
    """an orig list or the live image; its own key list (it never reads the resident key set) or none"""
    from tests import nearest_seed_ref as nref
    g = w.g
    orig = None
    if w.image is None or w.run_open or rng.random() < 0.5:
        share = pick(rng, [0.02, 0.1, 0.5])
        orig = [(g.ints[int(x)], pick(rng, [0.0, float(rng.random()), float(rng.integers(0, 4)) / 4.0])) for x in rng.integers(0, max(g.n, 1), max(1, int(g.n * share)))] if g.n else []
        orig += [(oc.UNKNOWN + 1, 0.5)] + orig[:1]
    keys = []
    if rng.random() < 0.7:
        spread = int(pick(rng, [1, 3, 1 << 62]))
        keys = [(v, int(rng.integers(0, spread)) if rng.random() < 0.9 else nref.U64_MAX) for v in g.ints if rng.random() < 0.8]
        keys += [(oc.UNKNOWN + 2, 0)] + keys[:2]
    return dict(orig=orig, keys=keys, discount=pick(rng, [0.5, 0.3, 0.0, 1.0]), rounds=int(pick(rng, [0, 1, 2, 5, 255])))


def nearest_seed_model(w, a):
    if a["orig"] is None:
        w.counts["d_image_hyperball" if w.image[0] == "HyperBall" else "d_image_sampled"] += 1
    w.live["nearest_seed"] = True
    w.called("nearest_seed")


class _OriginalsFromTheImage:
    """a context whose hb_nearest_seed takes its originals from the live image: the helper hands it the list the image holds"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def nearest_seed(self, orig_ids, orig_vals, key_ids, keys, **kw):
        return self._ctx.nearest_seed(None, None, key_ids, keys, from_image=True, **kw)


def nearest_seed_device(h, w, a):
    from tests import links_ref as lref
    from tests import test_nearest_seed as tn
    ctx, g = h.ctx, w.g
    before = ctx.stats()["device_bytes"]
    if a["orig"] is None:
        orig = list(zip(lref.id_ints(h.image[0]), h.image[1].tolist()))
        _, _, st = tn._check(_OriginalsFromTheImage(ctx), g.graph, orig, a["keys"], a["discount"], a["rounds"]) if g.n else (0, 0, None)
        assert st is None or st["with_original"] == len(orig)
    elif g.n:
        _, _, st = tn._check(ctx, g.graph, a["orig"], a["keys"], a["discount"], a["rounds"])
    else:  # an empty graph: an empty result (tests/test_nearest_seed.py)
        st = tn._call(ctx, a["orig"], a["keys"], a["discount"], a["rounds"])
        assert st["unknown_orig"] == len(a["orig"]) and st["unknown_keys"] == len(a["keys"]) and st["results"] == 0 and ctx.nearest_seed_count() == 0
    if st is not None:  # the operator's state is all that the call books (tests/test_nearest_seed.py)
        assert ctx.stats()["device_bytes"] - before == st["device_bytes"] - h.snap.get("nearest_seed_bytes", 0), "device_bytes"
        h.snap["nearest_seed_bytes"] = st["device_bytes"]
    snapshot(w, h, "nearest_seed")


def set_keys_draw(rng, w):
    """a list (duplicates, unknown ids, u64::MAX = not listed), the ranks of the live image, or the empty list"""
    g = w.g
    u = rng.random()
    if w.image is not None and not w.run_open and u < 0.3:
        return dict(how="ranks", keys=None)
    if u < 0.45 or not g.n:
        return dict(how="list", keys=[] if g.n else [(oc.UNKNOWN + 5, 1)])
    key = oc._few_keys(rng, g.n)
    return dict(how="list", keys=oc._key_list(g.ints, key))


def set_keys_model(w, a):
    if a["how"] == "ranks":
        w.counts["d_ranks_hyperball" if w.image[0] == "HyperBall" else "d_ranks_sampled"] += 1
        w.keys = "ranks"
    else:
        w.keys = {v: k for v, k in a["keys"] if v < oc.UNKNOWN}
    if w.cut_limit is not None:
        w.lists_dropped_by = "keys"
    w.cut_limit = None
    w.key_epoch += 1
    w.lnk_touched = True
    w.called("links_set_keys")


def set_keys_device(h, w, a):
    from stract_amd.harmonic import ids_from_ints
    ctx = h.ctx
    if a["how"] == "ranks":
        h.ranks_image = h.image
        st = ctx.links_set_keys(from_ranks=True)
        assert st["listed"] == len(h.image[0]) and st["unknown_keys"] == 0
    elif not a["keys"]:
        st = ctx.links_set_keys()
        assert st["listed"] == 0
    else:
        sent = a["keys"] + a["keys"][:2] + ([(oc.UNKNOWN + 4, 3)] if w.g.n else [])  # duplicates (the same key again) and an unknown id
        st = ctx.links_set_keys(ids_from_ints([v for v, _ in sent]), np.array([k for _, k in sent], dtype=np.uint64))
        assert st["listed"] == len(w.keys) and st["unknown_keys"] == sum(1 for v, _ in sent if v >= oc.UNKNOWN)
    assert st["device_bytes"] > 0 or not w.g.n


def _links_draw(rng, w, picks):
    count = _count(rng)
    if count and w.g.n:
        qsids, ids = oc._queries(rng, w.g.graph, picks, min(count, 300))
    else:  # no query at all; on the empty graph every query is unknown
        from stract_amd.harmonic import ids_from_ints
        qsids = np.full(count, -1, dtype=np.int64)
        ids = ids_from_ints([oc.UNKNOWN + i for i in range(count)])
    return dict(qsids=[int(x) for x in qsids], _ids=ids, limit=int(pick(rng, oc.LIMITS)), slots=int(pick(rng, oc.SLOTS)))


def backlinks_draw(rng, w):
    return _links_draw(rng, w, w.g.hubs)


def forwardlinks_draw(rng, w):
    return _links_draw(rng, w, w.g.hubs + w.g.has_out[:2])


def backlinks_model(w, a, name="backlinks"):
    a["first"] = not w.lnk_touched
    w.holder_call(name, len(a["qsids"]), a["limit"])
    w.live["links"] = True
    w.called(name)


def forwardlinks_model(w, a):
    if any(q >= 0 for q in a["qsids"]):  # (links_top_rows runs for a call with a known query alone)
        w.transpose_used("forwardlinks")
    backlinks_model(w, a, "forwardlinks")


def _links_device(h, w, a, forward):
    ctx, g = h.ctx, w.g
    before = ctx.stats()["device_bytes"]
    if not g.n or not a["qsids"]:  # tests/test_links.py, test_forwardlinks.py: no query, and the empty graph
        st = (ctx.forwardlinks if forward else ctx.backlinks)(a["_ids"], a["limit"], slots_per_batch=a["slots"])
        off, ids, keys, deg = ctx.links_copy()
        q = len(a["qsids"])
        assert st["queries"] == st["unknown"] == q and st["entries"] == 0 and st["batches"] == 0 and off.tolist() == [0] * (q + 1)
        assert len(ids) == len(keys) == 0 and not deg.any() and ctx.links_count() == (q, 0)
    elif forward:
        from tests import test_forwardlinks as tf
        st, _ = tf._run(ctx, g.fgraph, key_array(w, h), a["qsids"], a["limit"], slots=a["slots"], query_ids=a["_ids"])
    else:
        from tests import test_links as tl
        st, _ = tl._run(ctx, g.graph, key_array(w, h), a["qsids"], a["limit"], slots=a["slots"], query_ids=a["_ids"])
        if a["first"]:  # nothing of the links state existed: what the call reports is what it booked (tests/test_links.py)
            assert ctx.stats()["device_bytes"] == before + st["device_bytes"], "device_bytes"
    snapshot(w, h, "links")


def backlinks_device(h, w, a):
    _links_device(h, w, a, False)


def forwardlinks_device(h, w, a):
    _links_device(h, w, a, True)


def similar_hosts_draw(rng, w):
    g = w.g
    count = _count(rng, 1)
    liked = oc.draw_liked(rng, g.ints, min(count, 200), g.hubs[:1])  # (at most 256 distinct liked hosts)
    liked += [liked[int(i)] for i in rng.integers(0, len(liked), max(0, count - 200))]  # the longest lists: the same hosts again
    return dict(liked=liked, k=int(pick(rng, oc.LIMITS)))


def similar_hosts_model(w, a):
    w.holder_call("similar_hosts", len(a["liked"]), a["k"])
    w.live["similar_hosts"] = True
    w.called("similar_hosts")


def similar_hosts_device(h, w, a):
    from tests import test_similar_hosts as ts
    ts._check(h.ctx, w.g.graph, key_items(w, h), a["liked"], a["k"])
    snapshot(w, h, "similar_hosts")


def score_hosts_draw(rng, w):
    g = w.g
    pool = oc.draw_shared_pool(rng, g.ints, g.hubs)

    def draw(k):
        return oc.draw_from_pool(rng, g.ints, pool, k)

    requests = [dict(liked=draw(int(rng.integers(0, 40))), disliked=draw(int(rng.integers(0, 20))), nodes=draw(_count(rng)), normalized=bool(rng.integers(0, 2)),
                     self_score=pick(rng, [None, 0.25, 3.0])) for _ in range(int(rng.integers(1, 4)))]
    if not any(r["nodes"] for r in requests):  # (a call that scores no host at all books nothing: its suite has no such call)
        requests[0]["nodes"] = draw(1)
    return dict(requests=requests, limit=int(pick(rng, oc.LIMITS)), slots=int(pick(rng, oc.SLOTS)), small=bool(rng.integers(0, 2)))


def score_hosts_model(w, a):
    w.holder_call("score_hosts", sum(len(r["nodes"]) for r in a["requests"]), a["limit"])
    w.live["score_hosts"] = True
    w.called("score_hosts")


def score_hosts_device(h, w, a):
    from tests import test_score_hosts as tsc
    tsc._check(h.ctx, tsc._cut(w.g.graph, key_items(w, h), a["limit"]), a["requests"], a["limit"], slots_per_batch=a["slots"], small_pieces=a["small"])
    snapshot(w, h, "score_hosts")


# ---- hb_release_cached_memory ---------------------------------------------------------------------------------------------------------
def release_draw(rng, w):
    return {}


def release_model(w, a):
    if w.n_live() >= 4:  # (every live result must still read the same afterwards: the full comparison follows)
        w.counts["i_release_with_four_live"] += 1


def release_device(h, w, a):
    from stract_amd import _lib
    import ctypes
    held = ctypes.c_uint64(0)
    assert h.ctx.lib.hb_release_cached_memory(ctypes.byref(held)) == _lib.HB_OK


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
LIMITED = ("backlinks", "forwardlinks", "similar_hosts", "score_hosts", "similarity")
REFUSALS = ["open_run", "open_run", "open_run", "ranks_without_image", "image_without_image", "ranks_without_image", "image_without_image", "step_without_run", "limit_1025", "max_dist_16", "reader_of_nothing",
            "debug_reader_after_borrower", "finish_without_rows"]


def refusal_draw(rng, w):
    """a call the library must refuse (the lists of the sibling suites), drawn until one fits the world"""
    for k in range(12):
        what = pick(rng, REFUSALS)
        if k == 0 and w.image is None and not w.run_open and rng.random() < 0.5:  # no image is the rarer state: its two refusals first
            what = pick(rng, ["ranks_without_image", "image_without_image"])
        a = dict(what=what)
        if what == "open_run":
            if not w.run_open:
                continue
            a["op"] = pick(rng, OPERATORS)
        elif w.run_open and what != "reader_of_nothing":
            continue
        elif what in ("ranks_without_image", "image_without_image"):
            if w.image is not None:
                continue
        elif what == "limit_1025":
            a["op"] = pick(rng, LIMITED)
        elif what == "reader_of_nothing":
            gone = [r for r in READER_NAMES if r not in ("state", "similarity_batch", "similarity_counts") and not w.is_live(r)]
            if not gone:
                continue
            a["reader"] = pick(rng, gone)
        elif what == "debug_reader_after_borrower":
            if w.rows in ("HyperBall", "Similarity"):
                continue
            a["reader"] = "similarity_counts" if w.live.get("similarity") and rng.random() < 0.5 else "state"
        elif what == "finish_without_rows":
            if w.rows == "HyperBall":
                continue
        return a
    return None


def refusal_model(w, a):
    w.counts["k_refusals"] += 1
    if a["what"] == "open_run":
        w.h_pending.append(a["op"])
    elif a["what"] == "ranks_without_image":
        w.counts["d_ranks_refused"] += 1
    elif a["what"] == "image_without_image":
        w.counts["d_image_refused"] += 1
    elif a["what"] == "max_dist_16":
        w.live["histogram"] = None  # the one thing a refused hb_sampled_harmonic drops: its own earlier histogram


def _smallest_call(ctx, op, limit=3):
    """the smallest well-formed call of an operator (its arguments are not what it is refused for)"""
    from stract_amd.harmonic import ids_from_ints
    one = ids_from_ints([1])
    return {"sampled": lambda: ctx.sampled_harmonic(sources=one), "distances": lambda: ctx.distances(one), "betweenness": lambda: ctx.betweenness(one),
            "similarity": lambda: ctx.inbound_similarity(one, limit=limit), "nearest_seed": lambda: ctx.nearest_seed(one, np.array([0.5])),
            "links_set_keys": lambda: ctx.links_set_keys(one, np.array([3], dtype=np.uint64)), "backlinks": lambda: ctx.backlinks(one, limit),
            "forwardlinks": lambda: ctx.forwardlinks(one, limit), "similar_hosts": lambda: ctx.similar_hosts(one, limit),
            "score_hosts": lambda: ctx.score_hosts([dict(liked=one, nodes=one)], limit=limit)}[op]


def refusal_device(h, w, a):
    from stract_amd import _lib
    ctx, what = h.ctx, a["what"]
    if what == "open_run":
        refused(_smallest_call(ctx, a["op"]))
    elif what == "ranks_without_image":
        refused(lambda: ctx.links_set_keys(from_ranks=True))
    elif what == "image_without_image":
        refused(lambda: ctx.nearest_seed(from_image=True))
    elif what == "step_without_run":
        refused(ctx.step)
    elif what == "limit_1025":
        refused(_smallest_call(ctx, a["op"], 1025))
    elif what == "max_dist_16":
        refused(lambda: ctx.sampled_harmonic(max_dist=16), _lib.HB_ERR_LIMIT)
    elif what == "finish_without_rows":
        refused(ctx.finish)
    else:
        refuse_gone(ctx, w, a["reader"])  # each reader of it on its own


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def _closed(w):
    return w.g is not None and not w.run_open


def _operator(w):
    return _closed(w) and w.g.n > 0


Op = collections.namedtuple("Op", "name weight when draw model device")
OPERATIONS = [
    # when(world): the calls that are legal in this state; what is illegal comes in through `refusal`, by the lists of the sibling suites
    Op("load", 5, lambda w: w.stream is None, load_draw, load_model, load_device),  # hb_load_edges, hb_load_dense, hb_append_edges .. hb_finalize
    Op("append", 4, lambda w: w.stream is None and w.g is not None, append_draw, append_model, append_device),
    Op("end_stream", 6, lambda w: w.stream is not None, end_stream_draw, end_stream_model, end_stream_device),  # hb_finalize, hb_discard_appended
    Op("run", 6, lambda w: _operator(w), run_draw, run_model, run_device),
    Op("begin", 6, lambda w: w.g is not None and w.g.n > 0, begin_draw, begin_model, begin_device),
    Op("step", 14, lambda w: w.run_open and not w.converged, step_draw, step_model, step_device),
    Op("finish", 10, lambda w: w.g is not None and w.g.n > 0 and w.rows == "HyperBall" and (w.run_open or w.image is not None), finish_draw, finish_model, finish_device),
    Op("image", 5, lambda w: w.g is not None and w.image is not None, image_draw, image_model, image_device),  # results, ranks, top, store_harmonic
    Op("sampled", 5, _operator, sampled_draw, sampled_model, sampled_device),
    Op("distances", 5, _operator, distances_draw, distances_model, distances_device),
    Op("betweenness", 4, _operator, betweenness_draw, betweenness_model, betweenness_device),
    Op("similarity", 9, _operator, similarity_draw, similarity_model, similarity_device),  # limit = 0 and a cutting limit
    Op("nearest_seed", 6, _closed, nearest_seed_draw, nearest_seed_model, nearest_seed_device),
    Op("links_set_keys", 8, _closed, set_keys_draw, set_keys_model, set_keys_device),
    Op("backlinks", 7, _closed, backlinks_draw, backlinks_model, backlinks_device),
    Op("forwardlinks", 7, _closed, forwardlinks_draw, forwardlinks_model, forwardlinks_device),
    Op("similar_hosts", 6, _operator, similar_hosts_draw, similar_hosts_model, similar_hosts_device),
    Op("score_hosts", 6, _operator, score_hosts_draw, score_hosts_model, score_hosts_device),
    Op("release_cached_memory", 4, lambda w: w.g is not None, release_draw, release_model, release_device),
    Op("refusal", 7, lambda w: w.g is not None, refusal_draw, refusal_model, refusal_device),
]
BY_NAME = {op.name: op for op in OPERATIONS}


def summary(name, a):
    """an operation as it is printed: the arguments without the long lists (the seed replays them)"""
    def short(v):
        if isinstance(v, (list, tuple)) and len(v) > 6:
            return "%d entries" % len(v)
        if isinstance(v, (list, tuple)):
            return [short(x) for x in v]
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items()}
        return v
    return [name, {k: short(v) for k, v in (a or {}).items() if not k.startswith("_")}]


def run(seed, factory=None, n_ops=N_OPS, log=None, variant=None):
    """One sequence.  factory: what makes a context (None: the model alone).  Returns the world with its counts; a failure raises
    AssertionError with the seed, the index of the operation and the operations so far."""
    variant = VARIANTS[seed % len(VARIANTS)] if variant is None else variant
    rng = np.random.default_rng(seed)
    w = World(seed, variant)
    h = Handles(factory, w) if factory is not None else None
    log = log if log is not None else []
    state = dict(drawn=0, dropped=0, refused=0)

    def fail(e, where=""):
        return AssertionError(json.dumps(dict(seed=seed, variant=variant[0], operation=len(log) - 1, failed=where + repr(e)[:600], operations=log), default=str))

    def compare_now():
        try:
            compare_all(w, h)
        except Exception as e:  # noqa: BLE001
            raise fail(e, "full comparison: ") from e

    def one(op, a):
        log.append(summary(op.name, a))
        try:
            op.model(w, a)
            if h is not None:
                op.device(h, w, a)
        except Exception as e:  # noqa: BLE001  (whatever it is, it is reported with the way to it)
            raise fail(e) from e
        state["drawn"] += 1
        if op.name == "refusal":
            state["refused"] += 1
        if op.name in ("refusal", "release_cached_memory") or state["drawn"] % COMPARE_EVERY == 0:
            compare_now()

    def draw_and_run(op, *extra):
        a = op.draw(rng, w, *extra)
        if a is None:
            state["drawn"] += 1
            state["dropped"] += 1
            return False
        one(op, a)
        return True

    def settle():
        """a loaded graph with hosts and no open run, by the calls that lead there"""
        if w.stream is not None:
            one(BY_NAME["end_stream"], dict(how="discard", graph=w.stream))
        if w.g.n == 0:
            one(BY_NAME["load"], dict(graph=pick(rng, GRAPH_NAMES[1:]), how="edges", cuts=[]))
        if w.run_open:
            close_run()

    def close_run():
        while not w.converged:
            one(BY_NAME["step"], dict(steps=1))
        one(BY_NAME["finish"], {})

    def chain():
        """(e): a borrower, one of the six newer calls and hb_run in a row, or the reverse; which of the 36: by the seed"""
        b, n, d = CHAINS[(seed * 3 + w.chains) % len(CHAINS)]
        w.chains += 1
        settle()
        for name in ((b, n, "run") if d == "forth" else ("run", n, b)):
            draw_and_run(BY_NAME[name])

    def refusals_in_an_open_run():
        """(h): two of the ten operators (by the seed, in turn) refused inside an open run, the full comparison after each, and the run then
        finished: its result is the oracle's"""
        settle()
        one(BY_NAME["begin"], {})
        one(BY_NAME["step"], dict(steps=1))
        for j in range(2):
            one(BY_NAME["refusal"], dict(what="open_run", op=OPERATORS[(2 * seed + j) % len(OPERATORS)]))
        close_run()
        w.open_runs_done = True

    try:
        compare_now()  # nothing is loaded: nothing answers
        one(BY_NAME["load"], dict(graph=pick(rng, GRAPH_NAMES[1:]), how=pick(rng, ["edges", "dense"]), cuts=[]))
        # (d): no image yet - HB_LINKS_KEYS_FROM_RANKS or HB_SEED_FROM_IMAGE is refused for want of one
        one(BY_NAME["refusal"], dict(what=("ranks_without_image", "image_without_image")[seed % 2]))
        while state["drawn"] < n_ops:
            # upkeep, read from the world alone: once every one of the ten operators has run on this graph, another graph is loaded
            if w.stream is None and set(OPERATORS) <= w.ran and rng.random() < 0.5:
                draw_and_run(BY_NAME["load"], True)
                continue
            if w.chains < 3 and state["drawn"] >= (w.chains + 1) * n_ops // 5:  # three chains, spread over the sequence
                chain()
                continue
            if not w.open_runs_done and state["drawn"] >= 4 * n_ops // 5:
                refusals_in_an_open_run()
                continue
            table = [op for op in OPERATIONS if op.when(w)]
            # an operator that has not run on this graph yet is three times as likely
            # (inside an open run the ten operators come as refusals alone: twice as likely there)
            weights = np.array([op.weight * (3 if op.name in OPERATORS and op.name not in w.ran else 2 if op.name == "refusal" and w.run_open else 1)
                                for op in table], dtype=np.float64)
            draw_and_run(table[int(rng.choice(len(table), p=weights / weights.sum()))])
        if w.run_open:  # an open run is finished, and correctly
            close_run()
        compare_now()
    finally:
        if h is not None:
            h.close()
    w.counts["operations"], w.counts["dropped"], w.counts["refused"], w.counts["loads"] = state["drawn"], state["dropped"], state["refused"], w.loads
    w.counts["j_live_first"] = int("LIVE_FIRST" in variant[1])
    w.counts["j_chunk"] = int(variant[2] != 0)
    return w


def totals(worlds):
    total = collections.Counter()
    for w in worlds:
        total.update(w.counts)
    return total


def unmet(worlds):
    """the conditions of NEED the seed list misses, and the sequences that break a cap"""
    total = totals(worlds)
    bad = ["%s: %d < %d" % (k, total[k], n) for k, n in NEED.items() if total[k] < n]
    if total["reload_other"] < total["reload_same"]:
        bad.append("a reload draws the same graph more often than another")
    for w in worlds:
        c = w.counts
        if c["dropped"] >= MAX_DROPPED * c["operations"]:
            bad.append("seed %d: dropped %d of %d" % (w.seed, c["dropped"], c["operations"]))
        if c["refused"] >= MAX_REFUSED * c["operations"]:
            bad.append("seed %d: refused %d of %d" % (w.seed, c["refused"], c["operations"]))
    return bad


def main():
    from stract_amd import _lib
    ap = argparse.ArgumentParser(description="the counts (a) .. (k) of a seed list, from the model alone")
    ap.add_argument("--seeds", type=int, nargs="+", required=True)
    ap.add_argument("--ops", type=int, default=N_OPS)
    a = ap.parse_args()
    worlds = [run(s, None, a.ops) for s in a.seeds]
    for s, w in zip(a.seeds, worlds):
        print(json.dumps(dict(seed=s, variant=w.variant[0], **{k: w.counts[k] for k in ("operations", "dropped", "refused", "reload_other", "reload_same", "discarded")})))
    total = totals(worlds)
    print(json.dumps(dict(total={k: total[k] for k in NEED}, unmet=unmet(worlds))))
    assert _lib._lib is None and _lib._lib_exp is None, "the model alone loads no library"
    sys.exit(1 if unmet(worlds) else 0)


if __name__ == "__main__":
    main()
