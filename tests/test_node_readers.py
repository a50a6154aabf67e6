"""The reader contract of the three node-valued operators - hb_distances, hb_betweenness, hb_nearest_seed - and of the two _top readers
(hb_nearest_seed_top, hb_similarity_top) at the C boundary: every call goes through ctx.lib.hb_* with ctx.h, one entry point at a time.

What is pinned: the refusal texts before a result exists and after a reload; hb_*_copy with a cap below the count (a prefix, and nothing
past it: sentinel-filled buffers), with one or both outputs NULL; hb_*_all with cap < n and out == NULL; hb_distance_all and
hb_distance_copy each as the first reader after hb_distances (the compaction of the distances is made by whoever asks first); the _top
readers at k = 0, 1, results, results + 5 (n + 5) and with NULL outputs; the empty graph and a single node.

Every expected value is exact and comes from the host restatements the operators' own suites use (tests/distance_ref.py,
betweenness_ref.py, nearest_seed_ref.py, inbound_similarity_ref.py).  The large graph is a flipped fan of tests/fans.py with 590 nodes
(590 % 32 == 14): the hubs of 65 and 127 leaves have chunk trees under the default chunk, so device rows are not sids, and the inputs
leave nodes without a value (0 < count < n) in every operator.  It is a tree: every betweenness sum is a small integer, the same f64 in
any summation order."""
import ctypes

import numpy as np
import pytest

from stract_amd import _lib
from stract_amd.harmonic import EdgeListGraph, ids_from_ints
from tests import betweenness_ref as bref
from tests import distance_ref as dref
from tests import fans
from tests import inbound_similarity_ref as sref
from tests import nearest_seed_ref as nref

pytestmark = pytest.mark.gpu

KS = (0, 1, 3, 5, 17, 65, 127)
OPS = ("distance", "betweenness", "nearest_seed")
# the refusal of every reader while there is no result, as the library words it
REFUSAL = {
    "hb_distance_count": "hb_distance_count: no distances (call hb_distances)",
    "hb_distance_copy": "hb_distance_copy: no distances (call hb_distances)",
    "hb_distance_all": "hb_distance_all: no distances (call hb_distances)",
    "hb_betweenness_count": "hb_betweenness_count: no betweenness result (call hb_betweenness)",
    "hb_betweenness_copy": "hb_betweenness_copy: no betweenness result (call hb_betweenness)",
    "hb_betweenness_all": "hb_betweenness_all: no betweenness result (call hb_betweenness)",
    "hb_nearest_seed_count": "hb_nearest_seed_count: no nearest-seed result (call hb_nearest_seed)",
    "hb_nearest_seed_copy": "hb_nearest_seed_copy: no nearest-seed result (call hb_nearest_seed)",
    "hb_nearest_seed_all": "hb_nearest_seed_all: no nearest-seed result (call hb_nearest_seed)",
    "hb_nearest_seed_top": "hb_nearest_seed_top: no nearest-seed result (call hb_nearest_seed)",
    "hb_nearest_seed_seeds": "hb_nearest_seed_seeds: no nearest-seed result (call hb_nearest_seed)",
    "hb_similarity_top": "hb_similarity_top: no similarity result (call hb_inbound_similarity)",
}
DTYPE = {"distance": np.uint8, "betweenness": np.float64, "nearest_seed": np.float64}
FILL = {"distance": 255, "betweenness": -1.0, "nearest_seed": -1.0}
OUT_NAME = {"distance": "dist", "betweenness": "vals", "nearest_seed": "vals"}
SENTINEL = 0xA5


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _fn(ctx, op, what):
    return getattr(ctx.lib, "hb_%s_%s" % (op, what))


def _err(ctx):
    return (ctx.lib.hb_last_error(ctx.h) or b"").decode()


def _refused(ctx, rc, text):
    assert rc == _lib.HB_ERR_INVALID and _err(ctx) == text, (rc, _err(ctx), text)


def _count(ctx, op):
    k = ctypes.c_uint64(12345)
    assert _fn(ctx, op, "count")(ctx.h, ctypes.byref(k)) == _lib.HB_OK, _err(ctx)
    return k.value


def _copy(ctx, op, cap, ids=True, vals=True, size=None):
    """hb_<op>_copy into sentinel-filled buffers of `size` entries -> (rc, ids bytes or None, vals bytes or None)"""
    size = cap if size is None else size
    a = np.full(max(size, 1) * 16, SENTINEL, dtype=np.uint8) if ids else None
    b = np.full(max(size, 1) * np.dtype(DTYPE[op]).itemsize, SENTINEL, dtype=np.uint8) if vals else None
    rc = _fn(ctx, op, "copy")(ctx.h, _p(a), _p(b), cap)
    return rc, a, b


def _all(ctx, op, n):
    out = np.full(max(n, 1), FILL[op], dtype=DTYPE[op])
    assert _fn(ctx, op, "all")(ctx.h, _p(out), n) == _lib.HB_OK, _err(ctx)
    return out[:n]


def _same(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


# ---- the graphs, their inputs and the expected values ---------------------------------------------------------------------------------
class Case:
    """a graph, the inputs of the four operators on it, and per operator the expected value of every sid (FILL = none)"""

    def __init__(self, name):
        self.name = name
        if name == "empty":
            self.tuples = []
            self.dist_sources, self.bc_sources, self.orig, self.keys, self.liked, self.disliked = [7], [7], [(7, 0.5)], [(8, 1)], [7], [8]
        elif name == "single":
            self.tuples = [(1, 1)]
            self.dist_sources, self.bc_sources, self.orig, self.keys, self.liked, self.disliked = [1], [1], [(1, 2.5)], [], [1], []
        else:
            fan = fans.Fan(Ks=KS)
            assert fan.n == 590
            self.tuples = fan.tuples(flipped=True)  # tip -> leaf -> hub -> r -> x -> r2: the hubs' in-lists carry the lengths
            node = lambda v: int(v) + 1
            leaves127, leaves65, leaves17 = fan.leaves(127), fan.leaves(65), fan.leaves(17)
            tips = np.arange(fan.tip_first, fan.n)
            # reversed distances: everything that reaches the hub of 127 (through its chunk tree) or one leaf of 17
            self.dist_sources = [node(fan.hub_of(127)), node(leaves17[3])]
            # betweenness from tips and leaves: the sources and their ancestors are results, everything else is not
            self.bc_sources = [node(tips[0]), node(tips[len(tips) // 2]), node(leaves65[64]), node(leaves127[100]), node(fan.hub_of(3)), node(tips[-1])]
            # nearest seed: originals on every third tip, a few leaves and one hub, with ties in the values; keys that reverse the order of some leaves
            self.orig = [(node(t), 1.0 + (i % 4)) for i, t in enumerate(tips[::3])] + [(node(l), 8.0) for l in leaves127[::10]] + [(node(fan.hub_of(5)), 3.0)]
            self.keys = [(node(l), 1000 - i) for i, l in enumerate(leaves65)] + [(node(t), 5) for t in tips[::7]]
            self.liked = [node(fan.hub_of(65)), node(leaves127[5]), node(fan.hub_of(65))]
            self.disliked = [node(fan.hub_of(3))]

    def load(self, factory):
        ctx = factory(flags=_lib.HB_FLAG_ALL_RELS)
        ctx.load_edges(EdgeListGraph.from_tuples(self.tuples).host_edges() if self.tuples else np.zeros(0, dtype=_lib.EDGE))
        return ctx

    def prepare(self, ctx):
        """the graph as the context holds it, and the restatements' answers (made once)"""
        if hasattr(self, "want"):
            return
        self.ids, self.row_ptr, self.src = ctx.graph()
        self.n = n = len(self.ids)
        self.nodes = sref.id_ints(self.ids)
        sid = {v: i for i, v in enumerate(self.nodes)}
        self.want = {}
        if n:
            self.want["distance"] = dref.dijkstra(n, self.row_ptr, self.src, [sid[v] for v in self.dist_sources if v in sid], reversed=True)
            self.want["betweenness"] = bref.literal(n, self.row_ptr, self.src, [sid[v] for v in self.bc_sources if v in sid]).values(raw=True)
            _, vals, _ = nref.literal(self.ids, self.row_ptr, self.src, self.orig, self.keys, 0.5, 3)
            self.ns_vals = vals
            self.want["nearest_seed"] = np.array([vals.get(v, -1.0) for v in self.nodes], dtype=np.float64)
            self.scores = sref.literal(self.ids, self.row_ptr, self.src, self.liked, self.disliked)
        else:
            self.want = {op: np.zeros(0, dtype=DTYPE[op]) for op in OPS}
            self.ns_vals, self.scores = {}, np.zeros(0, dtype=np.float64)

    def run(self, ctx, op):
        """the operator through the wrapper (its options are not what this file is about); returns its stats"""
        if op == "distance":
            return ctx._distances(ids_from_ints(self.dist_sources), True, None, None, 0)
        if op == "betweenness":
            return ctx._betweenness(ids_from_ints(self.bc_sources), True, None)
        if op == "similarity":
            return ctx.inbound_similarity(ids_from_ints(self.liked), ids_from_ints(self.disliked))
        return ctx.nearest_seed(ids_from_ints([v for v, _ in self.orig]), np.array([x for _, x in self.orig], dtype=np.float64),
                                ids_from_ints([v for v, _ in self.keys]), np.array([k for _, k in self.keys], dtype=np.uint64), discount_factor=0.5, rounds=3)

    def full(self, op):
        """the full answer of hb_<op>_copy: (ids, values) of the sids that have a value"""
        keep = self.want[op] != FILL[op]
        return np.ascontiguousarray(self.ids[keep]), np.ascontiguousarray(self.want[op][keep])


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module")
def ran(gpu_ctx_factory):
    """ran(graph) -> (case, context): the graph loaded and all four operators run once, for the tests that only read"""
    cache = {}

    def get(name):
        if name not in cache:
            case = _case(name)
            ctx = case.load(gpu_ctx_factory)
            case.prepare(ctx)
            for op in OPS + ("similarity",):
                case.run(ctx, op)
            cache[name] = (case, ctx)
        return cache[name]

    yield get
    for _, ctx in cache.values():
        ctx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _every_reader_refuses(ctx, n):
    """every reader, asked alone with valid arguments, says that there is no result"""
    k = ctypes.c_uint64(0)
    w = ctypes.c_uint64(77)
    ids = np.zeros(n + 8, dtype=_lib.U128)
    for op in OPS:
        vals = np.zeros(n + 8, dtype=DTYPE[op])
        _refused(ctx, _fn(ctx, op, "count")(ctx.h, ctypes.byref(k)), REFUSAL["hb_%s_count" % op])
        _refused(ctx, _fn(ctx, op, "copy")(ctx.h, _p(ids), _p(vals), n), REFUSAL["hb_%s_copy" % op])
        _refused(ctx, _fn(ctx, op, "all")(ctx.h, _p(vals), n), REFUSAL["hb_%s_all" % op])
    vals = np.zeros(n + 8, dtype=np.float64)
    _refused(ctx, ctx.lib.hb_nearest_seed_top(ctx.h, 3, _p(ids), _p(vals), ctypes.byref(w)), REFUSAL["hb_nearest_seed_top"])
    assert w.value == 0  # (zeroed before the refusal)
    w = ctypes.c_uint64(77)
    _refused(ctx, ctx.lib.hb_similarity_top(ctx.h, 3, 0, _p(ids), _p(vals), ctypes.byref(w)), REFUSAL["hb_similarity_top"])
    assert w.value == 0
    has = np.zeros(n + 8, dtype=np.uint8)
    _refused(ctx, ctx.lib.hb_nearest_seed_seeds(ctx.h, _p(ids), _p(has), n), REFUSAL["hb_nearest_seed_seeds"])


@pytest.mark.parametrize("graph", ("single", "fan"))
def test_readers_refuse_before_any_operator_call_and_after_a_reload(gpu_ctx_factory, graph):
    case = _case(graph)
    with case.load(gpu_ctx_factory) as ctx:
        case.prepare(ctx)
        _every_reader_refuses(ctx, case.n)
        for op in OPS + ("similarity",):
            case.run(ctx, op)
        for op in OPS:
            assert _count(ctx, op) == len(case.full(op)[0])
        other = _case("single" if graph == "fan" else "fan")
        ctx.load_edges(EdgeListGraph.from_tuples(other.tuples).host_edges())  # another graph: every result is gone
        _every_reader_refuses(ctx, max(case.n, 590))


def test_readers_refuse_without_a_graph(gpu_ctx_factory):
    with gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS) as ctx:
        _every_reader_refuses(ctx, 0)


# ---- hb_*_copy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("graph", ("single", "fan"))
def test_copy_writes_the_prefix_and_nothing_else(ran, graph, op):
    case, ctx = ran(graph)
    ids, vals = case.full(op)
    count = _count(ctx, op)
    assert count == len(ids)
    if graph == "fan":
        assert 0 < count < case.n
    isz, vsz = 16, np.dtype(DTYPE[op]).itemsize
    for cap in sorted({count, count + 3, max(count - 1, 0), min(1, count), 0}):
        rc, a, b = _copy(ctx, op, cap, size=count + 4)
        assert rc == _lib.HB_OK, _err(ctx)
        k = min(cap, count)
        assert _same(a[:k * isz], ids[:k]) and _same(b[:k * vsz], vals[:k]), (cap, k)
        assert (a[k * isz:] == SENTINEL).all() and (b[k * vsz:] == SENTINEL).all(), cap  # nothing behind the prefix


@pytest.mark.parametrize("op", OPS)
def test_copy_with_null_outputs(ran, op):
    case, ctx = ran("fan")
    ids, vals = case.full(op)
    count = len(ids)
    for cap in (count, count - 1):
        rc, a, b = _copy(ctx, op, cap, ids=False)
        assert rc == _lib.HB_OK and a is None and _same(b[:cap * np.dtype(DTYPE[op]).itemsize], vals[:cap]), _err(ctx)
        rc, a, b = _copy(ctx, op, cap, vals=False)
        assert rc == _lib.HB_OK and b is None and _same(a[:cap * 16], ids[:cap]), _err(ctx)
        rc, a, b = _copy(ctx, op, cap, ids=False, vals=False)
        assert rc == _lib.HB_OK, _err(ctx)


# ---- hb_*_all -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("graph", ("single", "fan"))
def test_all(ran, graph, op):
    case, ctx = ran(graph)
    n = case.n
    assert _same(_all(ctx, op, n), case.want[op])
    out = np.full(n + 5, FILL[op], dtype=DTYPE[op])  # a larger cap: n values, the rest untouched
    marker = out.copy()
    assert _fn(ctx, op, "all")(ctx.h, _p(out), n + 5) == _lib.HB_OK, _err(ctx)
    assert _same(out[:n], case.want[op]) and _same(out[n:], marker[n:])
    before = out.copy()
    _refused(ctx, _fn(ctx, op, "all")(ctx.h, _p(out), n - 1), "hb_%s_all: cap < n" % op)
    _refused(ctx, _fn(ctx, op, "all")(ctx.h, None, n), "hb_%s_all: %s == NULL" % (op, OUT_NAME[op]))
    _refused(ctx, _fn(ctx, op, "count")(ctx.h, None), "hb_%s_count: count == NULL" % op)
    assert _same(out, before)


# ---- the distances' compaction, from both doors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ("all", "copy", "copy_of_nothing"))
def test_distance_readers_in_either_order(gpu_ctx_factory, first):
    case = _case("fan")
    with case.load(gpu_ctx_factory) as ctx:
        case.prepare(ctx)
        ids, vals = case.full("distance")
        for round_ in range(2):  # (the second call finds the buffers of the first)
            st = case.run(ctx, "distance")
            assert st["reached"] == len(ids)
            if first == "all":
                assert _same(_all(ctx, "distance", case.n), case.want["distance"])
            elif first == "copy_of_nothing":  # k == 0 and two NULL outputs leave the device alone; the next reader compacts
                assert _copy(ctx, "distance", 0)[0] == _lib.HB_OK and _copy(ctx, "distance", len(ids), ids=False, vals=False)[0] == _lib.HB_OK
            rc, a, b = _copy(ctx, "distance", len(ids))
            assert rc == _lib.HB_OK and _same(a, ids) and _same(b, vals), _err(ctx)
            assert _same(_all(ctx, "distance", case.n), case.want["distance"])
            assert _count(ctx, "distance") == len(ids)


# ---- the _top readers -----------------------------------------------------------------------------------------------------------------
def _top(ctx, which, k, ids=True, vals=True, size=None):
    size = (k if size is None else size) + 1
    a = np.full(size * 16, SENTINEL, dtype=np.uint8) if ids else None
    b = np.full(size * 8, SENTINEL, dtype=np.uint8) if vals else None
    w = ctypes.c_uint64(99)
    if which == "nearest_seed":
        rc = ctx.lib.hb_nearest_seed_top(ctx.h, k, _p(a), _p(b), ctypes.byref(w))
    else:
        rc = ctx.lib.hb_similarity_top(ctx.h, k, 0, _p(a), _p(b), ctypes.byref(w))
    assert rc == _lib.HB_OK, _err(ctx)
    return w.value, a, b


def _top_want(case, which, k):
    """(ids, values) in the order of the operator's own suite: nearest seed by NodeID ascending among equals, similarity descending"""
    if which == "nearest_seed":
        order = nref.top_order(case.ns_vals, k)
        return ids_from_ints([v for v, _ in order]), np.array([x for _, x in order], dtype=np.float64)
    order = sref.top_order(case.ids, case.scores, k)
    return ids_from_ints([v for _, v in order]), np.array([s for s, _ in order], dtype=np.float64)


@pytest.mark.parametrize("which", ("nearest_seed", "similarity"))
@pytest.mark.parametrize("graph", ("single", "fan"))
def test_top(ran, graph, which):
    case, ctx = ran(graph)
    results = len(case.ns_vals) if which == "nearest_seed" else case.n
    if graph == "fan":
        vals = list(case.ns_vals.values()) if which == "nearest_seed" else case.scores.tolist()
        assert len(set(vals)) < len(vals)  # ties: the order among equals is checked
    ks = [0, 1, results, results + 5] + ([case.n + 5] if which == "similarity" else [])
    for k in ks:
        got, a, b = _top(ctx, which, k, size=max(ks))
        assert got == min(k, results), (k, got)
        want_ids, want_vals = _top_want(case, which, k)
        assert len(want_ids) == got
        assert _same(a[:got * 16], want_ids) and _same(b[:got * 8], want_vals), k
        assert (a[got * 16:] == SENTINEL).all() and (b[got * 8:] == SENTINEL).all(), k
    # one output NULL, both NULL, written == NULL
    k = min(7, results)
    want_ids, want_vals = _top_want(case, which, k)
    got, a, b = _top(ctx, which, k, ids=False)
    assert got == k and _same(b[:k * 8], want_vals)
    got, a, b = _top(ctx, which, k, vals=False)
    assert got == k and _same(a[:k * 16], want_ids)
    assert _top(ctx, which, k, ids=False, vals=False)[0] == k
    buf = np.zeros(k + 1, dtype=_lib.U128)
    if which == "nearest_seed":
        assert ctx.lib.hb_nearest_seed_top(ctx.h, k, _p(buf), None, None) == _lib.HB_OK
    else:
        assert ctx.lib.hb_similarity_top(ctx.h, k, 0, _p(buf), None, None) == _lib.HB_OK
    assert _same(buf[:k], want_ids)


# ---- the empty graph ------------------------------------------------------------------------------------------------------------------
def test_empty_graph(ran):
    case, ctx = ran("empty")  # (every operator call has succeeded)
    assert case.n == 0
    for op in OPS:
        assert _count(ctx, op) == 0
        rc, a, b = _copy(ctx, op, 0)
        assert rc == _lib.HB_OK and (a == SENTINEL).all() and (b == SENTINEL).all()
        assert _copy(ctx, op, 5)[0] == _lib.HB_OK and _copy(ctx, op, 0, ids=False, vals=False)[0] == _lib.HB_OK
        out = np.full(1, FILL[op], dtype=DTYPE[op])
        assert _fn(ctx, op, "all")(ctx.h, _p(out), 0) == _lib.HB_OK and out[0] == FILL[op]
        _refused(ctx, _fn(ctx, op, "all")(ctx.h, None, 0), "hb_%s_all: %s == NULL" % (op, OUT_NAME[op]))
    for which in ("nearest_seed", "similarity"):
        for k in (0, 1, 5):
            got, a, b = _top(ctx, which, k)
            assert got == 0 and (a == SENTINEL).all() and (b == SENTINEL).all()
    seed, has = np.full(16, SENTINEL, dtype=np.uint8), np.full(1, SENTINEL, dtype=np.uint8)
    assert ctx.lib.hb_nearest_seed_seeds(ctx.h, _p(seed), _p(has), 0) == _lib.HB_OK and (seed == SENTINEL).all() and has[0] == SENTINEL
