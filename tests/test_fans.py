"""The walks at their list-length thresholds, with exact answers: hb_distances, hb_betweenness, hb_inbound_similarity and
hb_sampled_harmonic on the fan forests of tests/fans.py, whose lists end at, just under and just over every step and every switch of
the kernels (lane / wave / grid in bfs_push_kernel, quad / wave in bfs_pull_kernel, quad / bc_wave_sum / 4096-entry segments in
bc_back_node_kernel, the 8 / 4 / 256 / 64 entry steps of walk_gather, sim_bloom_kernel and sim_seed_*).

Comparison rule: EVERYTHING is exact.  The expected values are closed forms (tests/test_fans_ref.py checks them against the literal
restatements) whose sums are integers or half-integers far below 2^53, the same f64 in any summation order: floats are compared on
their bits.  A wrong bit is an entry read twice, skipped or taken from the wrong place - not rounding."""
import numpy as np
import pytest

from stract_amd import _lib
from tests import distance_ref as dref
from tests import fans
from tests import inbound_similarity_ref as sref
from tests import sample_ref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF  # no row (padding)
SEGMENT = 4096     # kBcSegment = kBfsHeavy
BC_MODES = (None, "dense", "sparse")
DIST_MODES = (None, "top_down", "bottom_up")
_FANS = {}


def _fan(diamond=False):
    if diamond not in _FANS:
        _FANS[diamond] = fans.Fan(diamond=diamond)
    return _FANS[diamond]


def _ids(nodes):
    """node indices of a fan as NodeIDs (index + 1)"""
    out = np.zeros(len(nodes), dtype=_lib.U128)
    out["lo"] = np.asarray(nodes, dtype=np.uint64) + np.uint64(1)
    return out


@pytest.fixture(scope="module")
def loaded(gpu_ctx_factory):
    """loaded(diamond, flipped, chunk, flags) -> (fan, context, graph): every variant is loaded once for the whole module"""
    cache = {}

    def get(diamond=False, flipped=False, chunk=0, flags=0):
        key = (diamond, flipped, chunk, flags)
        if key not in cache:
            fan = _fan(diamond)
            f, t = fan.edges(flipped)
            e = np.zeros(len(f), dtype=_lib.EDGE)
            e["from"]["lo"], e["to"]["lo"] = f, t
            ctx = gpu_ctx_factory(flags=_lib.HB_FLAG_ALL_RELS | flags, chunk=chunk)
            ctx.load_edges(e)
            graph = ctx.graph()
            assert np.array_equal(graph[0]["lo"], np.arange(1, fan.n + 1, dtype=np.uint64)) and not graph[0]["hi"].any()  # sid == node index
            cache[key] = (fan, ctx, graph)
        return cache[key]

    yield get
    for _, ctx, _ in cache.values():
        ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_exact(got, want, what):
    """bit for bit; where the expected division is 0 / 0 a NaN of either sign"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero((_bits(got) != _bits(want)) & ~nan)
    assert not len(bad), (what, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- the layout -----------------------------------------------------------------------------------------------------------------------
def _lists(plan):
    """per work row (node rows first, then the virtual rows): (reader-list length, reader-list start in out_rows, source-list length)"""
    rows_total = plan["n_pad"] + plan["nv"]
    src = plan["src"]
    readers = np.bincount(src[src != NONE].astype(np.int64), minlength=rows_total)
    start = np.cumsum(readers) - readers
    return readers, start, np.diff(plan["row_ptr"].astype(np.int64))


def _assert_layout(plan, want_lengths):
    """conditions on the INPUT: the reader lists of the node rows straddle the switches of bc_back_node_kernel and share segments"""
    n_pad = plan["n_pad"]
    readers, start, _ = _lists(plan)
    readers, start = readers[:n_pad], start[:n_pad]
    heavy = np.flatnonzero(readers > SEGMENT)
    assert len(heavy) >= 2                                    # (a) lists the grid sums
    assert (start[heavy] % SEGMENT != 0).any()                # (b) one that begins inside a segment
    first_seg, last_seg = start[heavy] // SEGMENT, (start[heavy] + readers[heavy] - 1) // SEGMENT
    assert np.intersect1d(first_seg, last_seg).size > 0       # (c) a segment where one heavy list ends and another begins ...
    shared = [(a, b) for a in heavy for b in heavy if a != b and (start[a] + readers[a] - 1) // SEGMENT == start[b] // SEGMENT]
    assert shared, "no two heavy rows share a segment"        # ... two different rows: both slots of that segment are in use
    for length in want_lengths:                               # (d) lists exactly at and one over each switch
        assert (readers == length).any(), length


@pytest.mark.parametrize("diamond", [False, True])
def test_layout_conditions(loaded, diamond):
    fan, ctx, _ = loaded(diamond)
    plan = ctx.plan()
    _assert_layout(plan, (4, 5, 8, 9, 16, 17, 64, 65, 256, 257, 272, 273, 4095, 4096, 4097, 8192, 8193, 12289))
    # the hubs' reader lists ARE the lengths of the family, whatever row the planner gave them
    row_of = np.full(fan.n, -1, dtype=np.int64)
    order = plan["order"]
    row_of[order[order != NONE].astype(np.int64)] = np.flatnonzero(order != NONE)
    assert (row_of >= 0).all()
    readers, _, _ = _lists(plan)
    assert np.array_equal(readers[row_of[fan.hub]], np.array(fan.Ks))
    # flipped: the in-lists carry the lengths, through chunk trees with ragged last chunks
    for chunk in (0, 4):
        _, fctx, fgraph = loaded(diamond, flipped=True, chunk=chunk)
        assert np.array_equal(np.diff(fgraph[1].astype(np.int64))[fan.hub], np.array(fan.Ks))
        fplan = fctx.plan()
        _, _, sources = _lists(fplan)
        assert fplan["nv"] > 0 and len(set(sources[fplan["n_pad"]:].tolist())) > 1  # chunk rows of more than one length


# ---- betweenness ----------------------------------------------------------------------------------------------------------------------
def _source_sets(fan):
    chain = [fan.r2, fan.x, fan.r]  # a hub is at three different depths for three lanes of one batch
    return {"chain": chain, "r": [fan.r], "two_batches": chain + [fan.hub_of(K) for K in (256, 257, 4096, 4097, 8193, 12289)]}


@pytest.mark.parametrize("which", ["chain", "r", "two_batches"])
@pytest.mark.parametrize("diamond", [False, True])
def test_betweenness(loaded, diamond, which):
    fan, ctx, _ = loaded(diamond)
    sources = sorted(_source_sets(fan)[which])
    S = len(sources)
    total, reached = fan.sums(sources)
    with np.errstate(divide="ignore", invalid="ignore"):
        normalized = total / (np.float64(S) * (np.float64(S) - np.float64(1.0)))  # one f64 division of the exact sum
    max_dist = max(int(fan.brandes(s)[0].max()) for s in sources)
    first = (S - 1) // 8 * 8
    for mode in BC_MODES:
        for raw in (True, False):
            what = "%s, %s, %s" % (which, mode, "raw" if raw else "normalized")
            want = total if raw else normalized
            got_ids, got_vals, st = ctx.betweenness(_ids(sources), raw=raw, mode=mode)
            assert np.array_equal(got_ids["lo"], np.flatnonzero(reached).astype(np.uint64) + np.uint64(1)), what
            _assert_exact(got_vals, want[reached], "values (%s)" % what)
            _assert_exact(ctx.betweenness_all(), np.where(reached, want, -1.0), "all values (%s)" % what)
            assert st["sources"] == S and st["batches"] == (S + 7) // 8 and st["max_dist"] == max_dist and st["results"] == int(reached.sum())
            assert st["unknown_sources"] == 0 and sum(st["levels_mode"]) == st["levels_forward"]
            if mode == "dense":
                assert st["levels_mode"][1] == 0 and st["levels_mode"][2] == 0
            if mode == "sparse":
                assert st["levels_mode"][0] == 0
            dist, sigma, delta = ctx.debug_betweenness_batch()  # the last batch
            for lane in range(8):
                if first + lane >= S:
                    assert (dist[:, lane] == 255).all() and not sigma[:, lane].any() and not _bits(delta[:, lane]).any(), what
                    continue
                d, sg, dl = fan.brandes(sources[first + lane])
                assert np.array_equal(dist[:, lane], np.where(d < 0, 255, d).astype(np.uint8)), (what, lane)
                assert np.array_equal(sigma[:, lane], sg), (what, lane)
                _assert_exact(delta[:, lane], dl, "delta of source %d (%s)" % (sources[first + lane], what))


# ---- distances ------------------------------------------------------------------------------------------------------------------------
def _inspected_top_down(plan, dist, reversed):
    """entries a forced top-down run reads: the whole push list of every reached node row and of every virtual row that relays"""
    n_pad, rows_total = plan["n_pad"], plan["n_pad"] + plan["nv"]
    row_ptr, src, order = plan["row_ptr"].astype(np.int64), plan["src"].astype(np.int64), plan["order"]
    readers, _, sources = _lists(plan)
    pushes = np.zeros(rows_total, dtype=bool)
    real = order != NONE
    pushes[:n_pad][real] = dist[order[real].astype(np.int64)] != dref.UNREACHED
    row = np.repeat(np.arange(rows_total), sources)  # the row of every entry: entry `src` feeds `row`
    keep = src != NONE
    frm, to = (row[keep], src[keep]) if reversed else (src[keep], row[keep])
    while True:  # a virtual row relays when a pushing row marks it
        marked = np.zeros(rows_total, dtype=bool)
        marked[to[pushes[frm]]] = True
        marked[:n_pad] = False
        if not (marked & ~pushes).any():
            break
        pushes |= marked
    return int((sources if reversed else readers)[pushes].sum())


def _distances(ctx, graph, plan, sources, reversed, want_closed, modes=DIST_MODES):
    ids, row_ptr, src = graph
    want = dref.bfs(len(ids), row_ptr, src, sources, reversed=reversed)
    assert np.array_equal(want, want_closed), (sources, reversed)
    keep = want != dref.UNREACHED
    for mode in modes:
        got_ids, got_dist, st = ctx.distances(_ids(sources), reversed=reversed, mode=mode)
        assert np.array_equal(ctx.distance_all(), want), (sources, reversed, mode)
        assert np.array_equal(got_ids, ids[keep]) and np.array_equal(got_dist, want[keep]), (sources, reversed, mode)
        assert st["reached"] == int(keep.sum()) == sum(st["frontier"]) and st["max_distance"] == int(want[keep].max())
        if mode == "top_down":  # pull stops at its first hit, push reads every entry: the counter is a function of the input
            assert not any(st["step"])
            assert st["edges_inspected"] == _inspected_top_down(plan, want, reversed), (sources, reversed)
        if mode == "bottom_up":
            assert all(st["step"][1:])


def _tips(fan):
    """a handful of tips: under three leaves (the lowest, a middle and the highest node id; the planner decides where in the hub's
    list they lie) of hubs at and over the switches, and the tip with the highest node id"""
    picks = []
    for K in (9, 257, 4096, 4097, 12289):
        for leaf in fan.leaves(K)[[0, K // 2, K - 1]]:
            mine = np.flatnonzero(fan.leaf_of[fan.tip_first:] == leaf)
            if len(mine):
                picks.append(fan.tip_first + int(mine[-1]))
    assert len(picks) >= 8
    return sorted(set(picks + [fan.n - 1]))


@pytest.mark.parametrize("diamond", [False, True])
def test_distances_on_the_fan(loaded, diamond):
    fan, ctx, graph = loaded(diamond)
    plan = ctx.plan()
    _distances(ctx, graph, plan, [fan.r2], False, fan.dist_from([fan.r2]))
    _distances(ctx, graph, plan, [fan.hub_of(4097), fan.hub_of(9), fan.x], False, fan.dist_from([fan.hub_of(4097), fan.hub_of(9), fan.x]))
    tips = _tips(fan)
    _distances(ctx, graph, plan, tips, True, fan.dist_to(tips))
    _distances(ctx, graph, plan, tips[:1], True, fan.dist_to(tips[:1]))


@pytest.mark.parametrize("chunk", [0, 4])
def test_distances_on_the_flipped_fan(loaded, chunk):
    fan, ctx, graph = loaded(False, flipped=True, chunk=chunk)
    plan = ctx.plan()
    tips = _tips(fan)
    _distances(ctx, graph, plan, tips, False, fan.dist_to(tips))  # along the flipped edges = against the fan's
    _distances(ctx, graph, plan, [fan.r2], True, fan.dist_from([fan.r2]))
    leaves = [int(fan.leaves(K)[-1]) for K in (256, 257, 4097)]  # (the leaf with the highest node id, wherever the planner put it)
    _distances(ctx, graph, plan, leaves, False, fan.dist_to(leaves), modes=(None, "top_down"))


# A bottom-up level needs ONE entry of a list only when that entry is the list's sole visited row: one leaf per hub is the source, chosen
# by its POSITION in the list the hub scans.  The positions come from the plan, not from the leaf numbers (the planner permutes rows).
PULL_KS = (255, 256, 257, 271, 4095, 4096, 4097)  # quad up to kBfsLongPull = 256, the whole wave above, 64 entries per step
LONG_PULL = 256


def _row_of(fan, plan):
    order = plan["order"]
    row_of = np.full(fan.n, -1, dtype=np.int64)
    row_of[order[order != NONE].astype(np.int64)] = np.flatnonzero(order != NONE)
    assert (row_of >= 0).all()
    return row_of


def _pull_positions(K):
    """entries of a K-entry list where a scan in steps of 4 or 64 can lose one: both ends, the last lane of the first 64-entry step and
    the first of the second, the first and last lane of the last full step, the first entry of the ragged tail"""
    full = K // 64 * 64
    return {"first": 0, "lane 63": 63, "second step": 64, "last full step": full - 64, "end of last full step": full - 1,
            "tail": min(full, K - 1), "last": K - 1}


@pytest.mark.parametrize("where", ["first", "lane 63", "second step", "last full step", "end of last full step", "tail", "last"])
def test_sole_hit_of_a_pulled_reader_list(loaded, where):
    """reversed, bottom-up on the fan: h_K scans its K readers (out_rows, ascending reader rows: the sorted transposition of
    hb_plan.hip) for its only visited leaf - by its quad for K <= 256, by the whole wave above"""
    fan, ctx, graph = loaded(False)
    plan = ctx.plan()
    row_of = _row_of(fan, plan)
    _, _, sources_len = _lists(plan)
    src = plan["src"]
    entry_row = np.repeat(np.arange(plan["n_pad"] + plan["nv"]), sources_len)  # the reader of every entry, ascending
    leaves = []
    for K in PULL_KS:
        readers = entry_row[src == row_of[fan.hub_of(K)]]
        pos = _pull_positions(K)[where]
        assert len(readers) == K and 0 <= pos < K and (np.diff(readers) > 0).all()
        assert np.array_equal(np.sort(plan["order"][readers].astype(np.int64)), fan.leaves(K))  # node rows, the leaves of h_K
        leaf = int(plan["order"][readers[pos]])
        assert np.flatnonzero(readers == row_of[leaf]).tolist() == [pos]  # the position, asserted
        leaves.append(leaf)
    assert sum(K > LONG_PULL for K in PULL_KS) >= 5 and sum(K <= LONG_PULL for K in PULL_KS) >= 2
    want = fan.dist_to(leaves)
    assert all(want[fan.hub_of(K)] == 1 for K in PULL_KS) and int((want == 0).sum()) == len(PULL_KS)  # one visited reader per hub
    _distances(ctx, graph, plan, leaves, True, want, modes=("bottom_up", None))


def _tree_entry(plan, row, upper, lowest):
    """follow the chunk tree below `row`: entry `upper` of every list of virtual rows, entry `lowest` of the list of node rows it ends
    in; -> (that node row, the length of that last list)"""
    n_pad, row_ptr, src = plan["n_pad"], plan["row_ptr"].astype(np.int64), plan["src"]
    while True:
        entries = src[row_ptr[row]:row_ptr[row + 1]]
        entries = entries[entries != NONE].astype(np.int64)
        assert len(entries)
        if (entries < n_pad).all():
            return int(entries[lowest]), len(entries)
        assert (entries >= n_pad).all()
        row = int(entries[upper])


@pytest.mark.parametrize("chunk", [0, 4])
def test_sole_hit_of_a_pulled_chunk_tree(loaded, chunk):
    """forward, bottom-up on the flipped fan: the chunk rows under h_K scan their entries, then h_K its chunk rows, for the only visited
    leaf - the first and the last entry of the first and of the last (ragged) chunk"""
    fan, ctx, graph = loaded(False, flipped=True, chunk=chunk)
    plan = ctx.plan()
    row_of = _row_of(fan, plan)
    ragged = False
    for upper in (0, -1):
        for lowest in (0, -1):
            leaves = []
            for K in PULL_KS:
                hub = row_of[fan.hub_of(K)]
                row, length = _tree_entry(plan, hub, upper, lowest)
                leaf = int(plan["order"][row])
                assert leaf in fan.leaves(K)
                leaves.append(leaf)
                ragged |= length != _tree_entry(plan, hub, 0, 0)[1]
            assert len(set(leaves)) == len(PULL_KS)
            _distances(ctx, graph, plan, leaves, False, fan.dist_to(leaves), modes=("bottom_up", None))
    assert ragged  # some last chunk is shorter than the first


# ---- inbound similarity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 4])
def test_inbound_similarity_on_the_flipped_fan(loaded, chunk):
    fan, ctx, graph = loaded(False, flipped=True, chunk=chunk)
    hubs = [int(h) for h, K in zip(fan.hub, fan.Ks) if K >= 1]
    assert len(hubs) > 16  # two batches
    length, bloom, _ = sref.numpy_state(*graph)
    assert np.array_equal(length[fan.hub], np.array(fan.Ks))
    K_of = dict(zip(fan.hub.tolist(), fan.Ks))
    # three orders of the same anchors: every hub is in the last batch - the one whose counts can be read back - of one of them
    for liked in (hubs, hubs[16:] + hubs[:16], hubs[10:] + hubs[:10]):
        last = liked[16:]
        anchors = [h + 1 for h in liked]
        want = sref.numpy_scores(*graph, anchors, [])
        # every node of the flipped fan has one out-link: in-lists are disjoint, |in(v) & in(h_K)| = K for v = h_K and 0 elsewhere
        want_counts = np.zeros((fan.n, 16), dtype=np.uint32)
        for slot, h in enumerate(last):
            want_counts[h, slot] = K_of[h]
        for mode in BC_MODES:
            st = ctx.inbound_similarity(_ids(liked), mode=mode)
            assert st["liked"] == len(liked) and st["unknown"] == 0 and st["batches"] == 2
            _assert_exact(ctx.similarity_all(), want, "scores (%s)" % mode)
            counts, dev_bloom, dev_len = ctx.debug_similarity_batch()
            assert np.array_equal(counts, want_counts), (mode, np.argwhere(counts != want_counts)[:5])
            assert np.array_equal(dev_len, length.astype(np.uint32)) and np.array_equal(dev_bloom, bloom), mode
    # the vectorised bloom is the literal fold (sixteen words OR-ed) on the lists at the switches
    ints = sref.id_ints(graph[0])
    rp, s = graph[1].astype(np.int64), graph[2]
    for K in (1, 9, 64, 65, 257, 4097):
        h = fan.hub_of(K)
        assert sref.BitVec(ints[u] for u in s[rp[h]:rp[h + 1]].tolist()).fold() == int(bloom[h])
    # both lists, normalized: a leaf and a hub liked, a hub disliked
    liked, disliked = [int(fan.leaves(4097)[4096]), hubs[3]], [fan.hub_of(4096)]
    want = sref.numpy_scores(*graph, [v + 1 for v in liked], [v + 1 for v in disliked], True)
    ctx.inbound_similarity(_ids(liked), _ids(disliked), normalized=True)
    _assert_exact(ctx.similarity_all(), want, "scores, liked and disliked")


# ---- sampled harmonic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 4])
def test_sampled_harmonic_on_the_flipped_fan(loaded, chunk):
    fan, ctx, graph = loaded(False, flipped=True, chunk=chunk)
    ids, row_ptr, src = graph
    tips = _tips(fan)
    for sources in ([fan.r2] + [fan.hub_of(K) for K in (257, 4097, 12289)],
                    tips + [int(fan.leaves(K)[-1]) for K in (8, 9, 256, 257, 4096, 4097)]):  # (highest node id of each hub) the in-lists carry what the leaves send
        st = ctx.sampled_harmonic(max_dist=7, sources=_ids(sorted(sources)))
        assert st["sources"] == len(sources)
        assert np.array_equal(ctx.sample_histogram(), sample_ref.dijkstra_histogram(len(ids), row_ptr, src, sorted(sources), 7))
