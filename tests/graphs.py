"""Shared test graphs (mirrors of the reference's fixtures + synthetic generators)."""
import numpy as np

from stract_amd import _lib
from stract_amd.harmonic import EdgeListGraph

# the reference fixture, crates/core/src/webgraph/centrality/harmonic.rs:323-341
#   A->B, B->C, A->C, C->A, D->C
A, B, C, D = 1, 2, 3, 4
FIXTURE = [(A, B), (B, C), (A, C), (C, A), (D, C)]
TAG = 1 << 13                # RelFlags::TAG, webpage/html/links.rs:130
SAME_ICANN_DOMAIN = 1 << 21  # links.rs:139
NOFOLLOW = 1 << 8


def fixture_graph(flags=0, extra=()):
    return EdgeListGraph.from_tuples([(f, t, flags) for f, t in FIXTURE] + list(extra))


def host_fixture():
    """harmonic.rs:358-458: twelve A.com->A.com page links collapse to one host self-loop;
    C.com->B.com, D.com->B.com."""
    a, b, c, d = 0xA0, 0xB0, 0xC0, 0xD0
    return EdgeListGraph.from_tuples([(a, a)] * 12 + [(c, b), (d, b)]), (a, b, c, d)


def lcg_graph(n=200, m=1200, seed=12345):
    """ids 1..n, m unique non-self edges from a 64-bit LCG."""
    x = seed
    edges = set()
    while len(edges) < m:
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        f = (x >> 33) % n + 1
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        t = (x >> 33) % n + 1
        if f != t:
            edges.add((f, t))
    return sorted(edges)


def dense_from_tuples(tuples):
    """(ids U128 ascending, row_ptr, src) of a clean tuple list (unique, no flags)."""
    nodes = sorted({x for e in tuples for x in e[:2]})
    index = {v: i for i, v in enumerate(nodes)}
    rows = [[] for _ in nodes]
    for f, t in sorted(set((e[0], e[1]) for e in tuples)):
        rows[index[t]].append(index[f])
    row_ptr = np.zeros(len(nodes) + 1, dtype=np.uint64)
    for i, r in enumerate(rows):
        row_ptr[i + 1] = row_ptr[i] + len(r)
    src = np.array([s for r in rows for s in sorted(r)], dtype=np.uint32)
    ids = np.zeros(len(nodes), dtype=_lib.U128)
    for i, v in enumerate(nodes):
        ids[i]["lo"] = v & 0xFFFFFFFFFFFFFFFF
        ids[i]["hi"] = v >> 64
    return ids, row_ptr, src


def random_registers(rng, count, kind="mixed"):
    """Random 64-register blocks covering every branch of HyperLogLog::size."""
    regs = np.zeros((count, 64), dtype=np.uint8)
    for i in range(count):
        k = kind if kind != "mixed" else ("sparse", "small", "mid", "large", "wide")[i % 5]
        if k == "sparse":      # many zero registers -> linear counting
            nz = rng.integers(1, 40)
            pos = rng.choice(64, nz, replace=False)
            regs[i, pos] = rng.integers(1, 6, nz)
        elif k == "small":     # e <= 320 -> bias table
            regs[i] = rng.integers(0, 4, 64)
        elif k == "mid":
            regs[i] = rng.integers(1, 8, 64)
        elif k == "large":
            regs[i] = rng.integers(8, 30, 64)
        else:                  # extreme register values incl. > 47 (sequential f64 fold)
            regs[i] = rng.integers(0, 66, 64)
    return regs


def random_graph(rng, kind=None):
    """Small random graphs of several shapes (as unique (from, to) int tuples, ids 1..n)."""
    kind = kind or ("uniform", "stars", "chains", "dense_core", "bipartite")[int(rng.integers(0, 5))]
    n = int(rng.integers(2, 600))
    edges = set()
    if kind == "uniform":
        for _ in range(int(rng.integers(0, 6 * n))):
            edges.add((int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))))
    elif kind == "stars":      # a few destinations with very many sources (deep chunk trees at small chunk sizes)
        for h in range(1, int(rng.integers(1, 5)) + 1):
            for s in rng.choice(np.arange(1, n + 1), size=int(rng.integers(1, n)), replace=False):
                edges.add((int(s), h))
        for _ in range(n):
            edges.add((int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))))
    elif kind == "chains":     # long diameter: many frontier / sparse passes
        for i in range(1, n):
            edges.add((i, i + 1))
        for _ in range(n // 4):
            edges.add((int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))))
    elif kind == "dense_core":
        core = max(2, n // 10)
        for a in range(1, core + 1):
            for b in range(1, core + 1):
                if rng.random() < 0.5:
                    edges.add((a, b))
        for v in range(core + 1, n + 1):
            edges.add((v, int(rng.integers(1, core + 1))))
            edges.add((int(rng.integers(1, core + 1)), v))
    else:                      # sources-only nodes -> destination-only nodes
        half = max(1, n // 2)
        for _ in range(4 * n):
            edges.add((int(rng.integers(1, half + 1)), int(rng.integers(half + 1, n + 2))))
    return kind, sorted(edges)


def dead_fringe_graph(rng):
    """("dead_fringe", tuples): a strongly connected live part - hosts 1 .. n_live on a ring, a random chord each - and n_dead hosts behind
    them that only link into it, so none of them has an in-link.  n_live lies on either side of a multiple of 64 and n_dead around 64
    (the row tiles of the live-first device order); host 1 is fed by every third live host and every second dead
    one, so its list is long enough for a chunk tree and ends in dead sources under that order."""
    n_live = 64 * int(rng.integers(1, 9)) + int(rng.integers(-1, 2))
    n_dead = int(rng.choice([1, 63, 64, 65, 200]))
    e = set()
    for v in range(1, n_live + 1):
        e.add((v, v % n_live + 1))
        e.add((v, int(rng.integers(1, n_live + 1))))
        if v % 3 == 0:
            e.add((v, 1))
    for d in range(n_live + 1, n_live + n_dead + 1):
        for t in rng.integers(1, n_live + 1, int(rng.integers(1, 4))).tolist():
            e.add((d, int(t)))
        if d % 2 == 0:
            e.add((d, 1))
    return "dead_fringe", sorted((a, b) for a, b in e if a != b)


def tailed_graph(core=300, core_edges=1500, chain=120, seed=7, branch=3):
    """A graph that reaches the reference's sqrt(n) tail (harmonic.rs:244-252): an LCG core whose node 1 feeds a
    chain of `chain` hosts with a few side branches.  Ids are salted so that bloom slots are not trivially distinct.
    Returns host-level tuples (from, to, 0)."""
    salt = 0x9E3779B97F4A7C15
    def nid(k):
        return ((k * salt) & 0xFFFFFFFFFFFFFFFF) | (k << 64)
    e = [(nid(f), nid(t), 0) for f, t in lcg_graph(core, core_edges, seed)]
    first = core + 1
    e.append((nid(1), nid(first), 0))
    for k in range(chain - 1):
        e.append((nid(first + k), nid(first + k + 1), 0))
        if branch and k % branch == 0:
            e.append((nid(first + k), nid(first + chain + k), 0))  # a leaf hanging off the chain
    return e


# ---- crafted ids: any (register index, register value) of HyperLogLog<64>::add ---------------------------------------------------
HLL_MUL = 11400714819323198549        # FastHasher (hyperloglog.rs:4311-4313): one wrapping multiplication; odd, so invertible mod 2^64
HLL_MUL_INV = pow(HLL_MUL, -1, 1 << 64)
EXTREME_VALUES = (40, 47, 48, 51, 55, 58, 65)  # 47 | 48: either side of the estimator's `big` switch; 58: the largest counted value; 65: hash << 6 == 0


def crafted_id_low(index, value, low_bits=0):
    """The low 64 id bits whose hash sets register `index` (0..63) to `value` (1..58, or 65: the bits below the index are all zero).
    value <= 58: hash = index << 58 | 1 << (58 - value) | low_bits mod 2^(58 - value); 59..64 cannot occur (add shifts the hash left by
    six before it counts leading zeros) and 0 is no value of add.  Distinct NodeIDs with the same low half differ in the high half."""
    if not 0 <= index < 64:
        raise ValueError("register index %r" % (index,))
    if value == 65:
        h = index << 58
    elif 1 <= value <= 58:
        h = index << 58 | 1 << (58 - value) | (low_bits % (1 << (58 - value)))
    else:
        raise ValueError("register value %r: add() gives 1..58 or 65" % (value,))
    return (h * HLL_MUL_INV) % (1 << 64)


def extreme_register_graph(seed=1, chain=40, sinks=208, filler=0):
    """A graph of about 1000 nodes whose counters hold registers of 40..58 and 65 from pass 0 on, as (ids, row_ptr, src) in the shape
    dense_from_tuples returns.  Real ids are xxh3 hashes: a register of 58 has odds of about 2^-52 per id, so these are built
    (crafted_id_low).  The high half of an id is the node's place in the node order; the device order sorts by out-degree and then by
    that place, so nodes of one out-degree lie in the order written here.

      sources   one crafted node per register index and value of EXTREME_VALUES (448 nodes, no in-edges)
      sat       fed by the 64 sources of value 65: every register 65, sum = 2^-59, e ~ 1.7e21 > 2^64: size() saturates
      sinks     `sinks` ordinary nodes fed by one crafted source for each of k register indices, kinds taken in turn so that the 16 rows of a
                tile mix them: k = 64 with values up to 58 (big, no zero register), k = 64 with values 40 / 47 only (not big), k in 30..63
                (zero registers, but too few for linear counting: the sum decides), k in 20..29 (decided by the zero count)
      hub       fed by every crafted source and by 200 ordinary nodes: virtual rows with big registers at every chunk size
      hub2      fed by 100 of those ordinary nodes, every sink and every chain node: virtual rows whose big registers arrive after pass 0
      chain     `chain` ordinary nodes behind eight of the sinks; sat enters it half way, three chain nodes (the last one among them) link
                back into sinks that feed the chain's head: a second wave of (saturated) counters walks the chain.  One node changes per pass and wave, so the
                bitmap, sweep and tail passes all move counters with registers above 47.
      filler    (the wide form only) `filler` ordinary nodes without in-edges that feed one drain node, spread evenly between the sinks.  They
                have a sink's out-degree, so the device order keeps them there: with more 64-row tiles than workgroups a workgroup's
                deferred epilogue holds four pending tiles per flush, and the sinks fall into all four (flush_slots).

    No test built on this graph tries to show that the estimator's f64 fold depends on its order.  Where every register is at least 30
    the fold is exact in any order (64 terms within 41 bits); where a register above 47 meets zero registers the last bits of the sum
    can depend on the order, but such a sum is far from any estimate whose integer part could flip, so no size would show it.  What
    the graph does reach: the multiset of registers that arrives at the fold, the hand-over of the folded size to the lane that owns
    the row, saturation at 2^64 - 1, and Kahan terms of about 2^64."""
    rng = np.random.default_rng(seed)
    place = [0]

    def node(low):
        place[0] += 1
        return (place[0] << 64) | low

    def ordinary():
        return node(place[0] + 1)  # small integers: no register above about 25

    source = {(j, v): node(crafted_id_low(j, v, int(rng.integers(0, 1 << 62)))) for j in range(64) for v in EXTREME_VALUES}
    feeders = [ordinary() for _ in range(200)]
    hub, hub2, sat = ordinary(), ordinary(), ordinary()
    e = [(source[j, 65], sat) for j in range(64)]
    e += [(s, hub) for s in source.values()] + [(f, hub) for f in feeders] + [(f, hub2) for f in feeders[:100]]
    sink = []
    drain = ordinary() if filler else None
    for i in range(sinks):
        kind = i % 8
        v = ordinary()
        sink.append(v)
        e += [(ordinary(), drain) for _ in range(filler // sinks)]
        if kind in (0, 2, 4, 6):    # every index, some value above 47
            idx, vals = range(64), [int(x) for x in rng.choice(EXTREME_VALUES[:6], 64)]
            vals[int(rng.integers(0, 64))] = EXTREME_VALUES[2 + (i // 8) % 4]
        elif kind == 1:             # every index, nothing above 47
            idx, vals = range(64), [int(x) for x in rng.choice(EXTREME_VALUES[:2], 64)]
        elif kind in (3, 7):        # 1..34 zero registers: size() needs the sum
            idx = rng.choice(64, int(rng.integers(30, 64)), replace=False).tolist()
            vals = [int(x) for x in rng.choice(EXTREME_VALUES, len(idx))]
        else:                       # >= 35 zero registers: linear counting
            idx = rng.choice(64, int(rng.integers(20, 30)), replace=False).tolist()
            vals = [int(x) for x in rng.choice(EXTREME_VALUES, len(idx))]
        e += [(source[int(j), x], v) for j, x in zip(idx, vals)] + [(v, hub2)]
    links = [ordinary() for _ in range(chain)]
    e += [(a, b) for a, b in zip(links, links[1:])] + [(c, hub2) for c in links]
    e += [(sink[i], links[0]) for i in (3, 5, 13, 21, 27, 45, 77, 101)]   # kinds 3 and 5: zero registers reach the chain's head
    e.append((sat, links[chain // 2]))
    e += [(links[chain // 8], sink[5]), (links[chain // 3], sink[21]), (links[chain - 1], sink[77])]
    return dense_from_tuples(e)


class ExtremeReference:
    """extreme_register_graph with the oracle's state after every pass (computed once, read-only), and the conditions the graph is built
    for, asserted on the oracle alone."""

    def __init__(self, seed=1):
        from oracle import hbo
        self.ids, self.row_ptr, self.src = extreme_register_graph(seed)
        o = hbo.Dense(np.ascontiguousarray(self.ids["lo"]), self.row_ptr, self.src)
        self.initial = (o.registers(), o.sizes())
        self.passes = []  # per pass: has_changes, stats, registers, Kahan sum, Kahan err, sizes, state hash, rows with a register > 47 that changed
        before, has = self.initial[0], True
        while has:
            has, st = o.step(hbo.FRONTIER)
            regs = o.registers()
            ks, ke = o.kahan()
            moved_big = int((((regs != before).any(axis=1)) & ((regs > 47).any(axis=1))).sum())
            self.passes.append(dict(has=has, st=st, regs=regs, ks=ks, ke=ke, sizes=o.sizes(), hash=o.state_hash(), moved_big=moved_big))
            before = regs
        self.T = len(self.passes)
        self.vals, self.keep, self.k = o.finish()
        self.final_hash = o.state_hash()
        for a in (self.ids, self.row_ptr, self.src, self.vals, self.keep, *self.initial):
            a.setflags(write=False)
        for p in self.passes:
            for a in (p["regs"], p["ks"], p["ke"], p["sizes"]):
                a.setflags(write=False)
        self.check()

    def check(self):
        SAT = (1 << 64) - 1
        first, later = self.passes[0], self.passes[min(7, self.T - 1)]
        regs = first["regs"]
        assert sorted(set(regs[regs > 47].tolist())) == [48, 51, 55, 58, 65]
        assert not np.isin(self.passes[-1]["regs"], np.arange(59, 65)).any()
        big, full = (regs > 47).any(axis=1), (regs != 0).all(axis=1)
        assert int((big & full).sum()) >= 100
        sat0, sat7 = int((first["sizes"] == SAT).sum()), int((later["sizes"] == SAT).sum())
        assert sat0 >= 1 and sat7 > sat0, (sat0, sat7)
        assert max(float(p["ks"].max()) for p in self.passes) >= 2.0 ** 63
        assert 40 <= self.T <= 50, self.T
        from stract_amd import _lib
        plan = _lib.host_plan(self.row_ptr, self.src)
        assert plan["nv"] > 0  # virtual rows at the default chunk size
        # four or more 16-row tiles of the default device order hold a counter of each kind, and as many mix big and other rows
        kind = row_kinds(regs, self.row_ptr)
        tiles = [set(kind[rows].tolist()) for rows in tile_rows(plan["order"], len(kind))]
        assert sum({BIG_FULL, SMALL_FULL, BY_SUM, BY_ZERO_COUNT} <= s for s in tiles) >= 4, tiles
        assert sum(BIG_FULL in s and len(s - {BIG_FULL}) > 0 for s in tiles) >= 4
        # with the interpreter's two workgroups (few_blocks) the slots 1, 2 and 3 of a four-tile flush hold big and other rows (slot 0 is
        # the one every launch with a single tile per workgroup uses)
        slots = flush_slots(plan["order"], kind, 2)
        assert all({BIG_FULL, SMALL_FULL, BY_SUM, BY_ZERO_COUNT} <= slots[k] for k in (1, 2, 3)), slots


TILE_ROWS = 16                    # rows of one wave's tile: one quad per row
LINEAR_COUNTING_ZEROS = 35        # 64 ln(64 / v) <= 40 from v = 35 zero registers on: size() is decided by the zero count
NO_SOURCES, BIG_FULL, SMALL_FULL, BY_SUM, BY_ZERO_COUNT = -1, 0, 1, 2, 3


def row_kinds(regs, row_ptr):
    """Per node, what its counter asks of the epilogue: a register above 47 and no zero register / no zero register and nothing above
    47 / zero registers but the sum decides / the zero count decides / (no sources: pass 0 leaves the row as it is)."""
    zeros = (regs == 0).sum(axis=1)
    kind = np.where(zeros == 0, np.where((regs > 47).any(axis=1), BIG_FULL, SMALL_FULL), np.where(zeros < LINEAR_COUNTING_ZEROS, BY_SUM, BY_ZERO_COUNT))
    kind[np.diff(row_ptr) == 0] = NO_SOURCES
    return kind


def tile_rows(order, n):
    """The nodes of every 16-row tile of a device order (padding rows left out)."""
    return [order[t:t + TILE_ROWS][order[t:t + TILE_ROWS] < n] for t in range(0, len(order), TILE_ROWS)]


def flush_slots(order, kind, workgroups):
    """Kinds of the rows in each of the four pending-tile slots of the deferred epilogue (hb_kernels.hip.h flush_pending), when the
    dense node-row launch has `workgroups` workgroups: workgroup b runs the 64-row tiles b, b + workgroups, ... and flushes after every
    fourth, so tile t lies in slot (t div workgroups) mod 4.  With at least as many workgroups as tiles only slot 0 is ever used."""
    slots = [set(), set(), set(), set()]
    for t, rows in enumerate(tile_rows(order, len(kind))):
        slots[(t * TILE_ROWS // 64 // workgroups) % 4] |= set(kind[rows].tolist())
    return slots


_EXTREME = {}


def extreme_reference(seed=1):
    if seed not in _EXTREME:
        _EXTREME[seed] = ExtremeReference(seed)
    return _EXTREME[seed]
