"""Who holds the shared device rows, and which result is live: hb_run, hb_sampled_harmonic, hb_distances,
hb_betweenness and hb_inbound_similarity in every order on ONE context.  Three of the four operators borrow the HyperBall rows
(d_regs / d_part / d_bits / the sweep scratch) and hb_sampled_harmonic also writes the result image; hb_distances borrows nothing.

Comparison rule: every call's result is compared bit for bit with the same call on a fresh context, and that fresh result is compared
with the CPU references by the sibling tests' own helpers (oracle/hbo.py, tests/sample_ref.py, distance_ref.py, betweenness_ref.py,
inbound_similarity_ref.py).  The graphs are the smallest on which all five calls give non-empty results."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib
from stract_amd.harmonic import EdgeListGraph, ids_from_ints
from tests import distance_ref as dref
from tests import graphs
from tests import inbound_similarity_ref as sref
from tests import sample_ref
from tests import test_betweenness as tb
from tests import test_distances as td
from tests import test_sampled_harmonic as ts
from tests import test_similarity as tsim

pytestmark = pytest.mark.gpu

# lcg70_fringe_live: lcg70 and nine hosts without an in-link that link into it, on a context with the live-first device order forced on
# (DESIGN.md section 32): the borrowed rows of the dead hosts lie behind the last row the passes visit from pass 1 on
TUPLES = {"lcg70": lambda: graphs.lcg_graph(n=70, m=300, seed=3), "fixture": lambda: list(graphs.FIXTURE),
          "lcg70_fringe_live": lambda: graphs.lcg_graph(n=70, m=300, seed=3) + [(101 + d, 1 + (7 * d + k) % 70) for d in range(9) for k in (0, 31)]}
FLAGS = {"lcg70_fringe_live": _lib.HB_FLAG_LIVE_FIRST}
NAMES = tuple(TUPLES)
CALLS = ("run", "sampled", "distances", "betweenness", "similarity")
BORROWERS = ("sampled", "betweenness", "similarity")  # they write the shared rows; hb_distances works in buffers of its own


class Case:
    """a graph, the arguments of the five calls on it and the oracle's HyperBall run"""

    def __init__(self, name):
        self.name = name
        self.edges = EdgeListGraph.from_tuples(TUPLES[name]()).host_edges()
        self.graph = self.ids, self.row_ptr, self.src = graphs.dense_from_tuples(TUPLES[name]())
        has_out = np.unique(np.asarray(self.src, dtype=np.int64))
        self.walk = has_out[[0, len(has_out) // 2, -1]].tolist()  # sids with an out-edge: the sampled and the Brandes sources
        self.forward = has_out[[1, -2]].tolist()
        ints = sref.id_ints(self.ids)
        self.liked, self.disliked = ints[::max(1, len(ints) // 5)][:5], ints[1:2]
        self.bv = sref.bitvecs(*self.graph)
        o = hbo.Dense(np.ascontiguousarray(self.ids["lo"]), self.row_ptr, self.src)
        self.passes = o.run()
        self.vals, self.keep, _ = o.finish()

    def load(self, factory):
        ctx = factory(flags=_lib.HB_FLAG_ALL_RELS | FLAGS.get(self.name, 0))
        ctx.load_edges(self.edges)
        live_first, n_live, _ = ctx.plan_live()
        assert live_first == (self.name in FLAGS) and (not live_first or 0 < n_live <= len(self.ids) - 9)
        return ctx

    def call(self, ctx, which):
        """the call `which` with this case's arguments"""
        if which == "run":
            ctx.run()
        elif which == "sampled":
            ctx.sampled_harmonic(sources=self.ids[self.walk])
        elif which == "distances":
            ctx.distances(self.ids[self.forward])
        elif which == "betweenness":
            ctx.betweenness(self.ids[self.walk])
        else:
            ctx.inbound_similarity(ids_from_ints(self.liked), ids_from_ints(self.disliked))

    def check(self, ctx, which):
        """the same call through the sibling test's helper: compared with the CPU reference"""
        if which == "run":
            st = ctx.run()
            gids, gvals = ctx.results()
            assert st["passes"] == self.passes and self.keep.any()
            assert np.array_equal(gids, self.ids[self.keep]) and np.array_equal(gvals.view(np.uint64), self.vals[self.keep].view(np.uint64))
        elif which == "sampled":
            _, h_ref = ts._check(ctx, sources_sids=self.walk)
            assert h_ref.any()
        elif which == "distances":
            assert td._check(ctx, self.forward, modes=(None,), ref=dref.bfs)["reached"] > len(self.forward)
        elif which == "betweenness":
            res, _ = tb._check(ctx, self.walk, modes=(None,))
            assert res.reached.sum() > len(self.walk)
        else:
            want, _ = tsim._check(ctx, ctx.graph(), self.bv, self.liked, self.disliked, modes=(None,))
            assert want.any()


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _read(ctx, which):
    """what the call `which` left to read, as bytes"""
    if which in ("run", "sampled"):
        out = ctx.results() + ((ctx.sample_histogram(),) if which == "sampled" else ())
    else:
        out = ({"distances": ctx.distance_all, "betweenness": ctx.betweenness_all, "similarity": ctx.similarity_all}[which](),)
    return tuple(a.tobytes() for a in out)


_FRESH = {}


def _fresh(factory, name, which):
    """the result of `which` on a context that has done nothing else - computed once, and checked there against the CPU reference"""
    if (name, which) not in _FRESH:
        case = _case(name)
        with case.load(factory) as ctx:
            case.call(ctx, which)
            got = _read(ctx, which)
            case.check(ctx, which)
            assert _read(ctx, which) == got
        _FRESH[name, which] = got
    return _FRESH[name, which]


def _refused(fn, code=_lib.HB_ERR_INVALID):
    with pytest.raises(_lib.HyperballError) as e:
        fn()
    assert e.value.code == code


def _histogram(ctx, levels=8):
    """hb_debug_sample_histogram itself (Context.sample_histogram refuses on its own when the last Python call failed)"""
    out = np.zeros((ctx.n(), levels), dtype=np.uint16)
    ctx._check(ctx.lib.hb_debug_sample_histogram(ctx.h, _lib._ptr(out)))
    return out


def _state(ctx):
    return ctx.registers().tobytes(), tuple(a.tobytes() for a in ctx.kahan()), ctx.sizes().tobytes(), ctx.state_hash()


REFUSALS = {  # refused by hb_sampled_harmonic after its entry: (keyword arguments, error code)
    "max_dist": (lambda case: dict(max_dist=16), _lib.HB_ERR_LIMIT),
    "unknown_source": (lambda case: dict(sources=np.concatenate([case.ids[:1], ids_from_ints([1 << 100])])), _lib.HB_ERR_INVALID),
    "samples": (lambda case: dict(samples=65536), _lib.HB_ERR_LIMIT),
}


# (1) a refused hb_sampled_harmonic changes nothing but the sampled histogram's validity: the finished run stays finished
@pytest.mark.parametrize("refusal", list(REFUSALS))
@pytest.mark.parametrize("name", NAMES)
def test_refused_sampled_call_leaves_the_finished_run_alone(gpu_ctx_factory, name, refusal):
    case = _case(name)
    kwargs, code = REFUSALS[refusal]
    with case.load(gpu_ctx_factory) as ctx:
        ctx.run()
        h0, r0 = ctx.state_hash(), _read(ctx, "run")
        assert r0 == _fresh(gpu_ctx_factory, name, "run")
        _refused(lambda: ctx.sampled_harmonic(**kwargs(case)), code)
        _refused(ctx.step)  # no run is open
        assert ctx.state_hash() == h0
        assert _read(ctx, "run") == r0  # a refused call leaves the result image alone
        for which in ("distances", "betweenness", "similarity"):
            case.check(ctx, which)
            assert _read(ctx, which) == _fresh(gpu_ctx_factory, name, which)
        # ... and the same refusal on top of a sampled result: the values stay, the histogram is dropped at the call's entry
        case.call(ctx, "sampled")
        s0 = _read(ctx, "sampled")
        _refused(lambda: ctx.sampled_harmonic(**kwargs(case)), code)
        assert tuple(a.tobytes() for a in ctx.results()) == s0[:2]
        _refused(lambda: _histogram(ctx))


# (2) all 25 ordered pairs (A, B): B's result does not depend on what A left behind
@pytest.mark.parametrize("first", CALLS)
@pytest.mark.parametrize("name", NAMES)
def test_every_ordered_pair_of_calls(gpu_ctx_factory, name, first):
    case = _case(name)
    for second in CALLS:
        with case.load(gpu_ctx_factory) as ctx:
            case.call(ctx, first)
            assert _read(ctx, first) == _fresh(gpu_ctx_factory, name, first), (first, second)
            case.call(ctx, second)
            assert _read(ctx, second) == _fresh(gpu_ctx_factory, name, second), (first, second)


# (3) what follows a finished run: no step; the HyperBall state answers while nobody has written the rows
@pytest.mark.parametrize("op", CALLS[1:])
@pytest.mark.parametrize("name", NAMES)
def test_after_a_finished_run(gpu_ctx_factory, name, op):
    case = _case(name)
    with case.load(gpu_ctx_factory) as ctx:
        ctx.run()
        s0, r0 = _state(ctx), _read(ctx, "run")
        case.call(ctx, op)
        _refused(ctx.step)
        if op in BORROWERS:
            for fn in (ctx.registers, ctx.kahan, ctx.sizes, ctx.state_hash, ctx.finish):
                _refused(fn)
        else:
            assert _state(ctx) == s0
            ctx.finish()  # (a second hb_finish: the same image again)
            assert _state(ctx) == s0 and _read(ctx, "run") == r0
        assert _read(ctx, op) == _fresh(gpu_ctx_factory, name, op)
        ctx.run()
        assert _state(ctx) == s0 and _read(ctx, "run") == r0


# (4) the counts of the last similarity batch lie in the shared rows: they are served until somebody else writes those rows
@pytest.mark.parametrize("then", ["distances", "betweenness", "sampled", "begin"])
@pytest.mark.parametrize("name", NAMES)
def test_similarity_batch_export(gpu_ctx_factory, name, then):
    case = _case(name)
    with case.load(gpu_ctx_factory) as ctx:
        case.call(ctx, "similarity")
        counts, bloom, length = ctx.debug_similarity_batch()
        assert counts.any() and np.array_equal(counts[:, :len(case.liked) + 1], sref.counts(case.bv, case.ids, case.liked + case.disliked))
        if then == "begin":
            ctx.begin()
        else:
            case.call(ctx, then)
        if then == "distances":
            again = ctx.debug_similarity_batch()
            assert all(np.array_equal(a, b) for a, b in zip(again, (counts, bloom, length)))
        else:
            _refused(ctx.debug_similarity_batch)
            bloom2, length2 = np.zeros_like(bloom), np.zeros_like(length)  # bloom / len alone are the operator's own
            ctx._check(ctx.lib.hb_debug_copy_similarity_batch(ctx.h, None, _lib._ptr(bloom2), _lib._ptr(length2)))
            assert np.array_equal(bloom2, bloom) and np.array_equal(length2, length)
        assert _read(ctx, "similarity") == _fresh(gpu_ctx_factory, name, "similarity")


# (5) the sampled histogram lives in a buffer of its own: it outlives hb_begin / hb_run; a refused call and a reload drop it
@pytest.mark.parametrize("name", NAMES)
def test_sample_histogram_lifetime(gpu_ctx_factory, name):
    case = _case(name)
    h_ref = sample_ref.dijkstra_histogram(len(case.ids), case.row_ptr, case.src, case.walk, 7)
    with case.load(gpu_ctx_factory) as ctx:
        case.call(ctx, "sampled")
        assert np.array_equal(ctx.sample_histogram(), h_ref)
        ctx.begin()
        assert np.array_equal(ctx.sample_histogram(), h_ref)  # (an open run)
        ctx.finish()
        ctx.run()
        assert np.array_equal(ctx.sample_histogram(), h_ref)
        _refused(lambda: ctx.sampled_harmonic(max_dist=16), _lib.HB_ERR_LIMIT)
        _refused(lambda: _histogram(ctx))
        case.call(ctx, "sampled")
        assert np.array_equal(_histogram(ctx), h_ref)
        ctx.load_edges(case.edges)
        _refused(lambda: _histogram(ctx))
        for fn in (ctx.results, ctx.distance_count, ctx.betweenness_count, ctx.similarity_all, ctx.state_hash, ctx.step, ctx.finish):
            _refused(fn)  # nothing of the first load answers, and nobody holds the rows
