"""CPU-side checks: the C-ABI library loads and exports every symbol include/hyperball.h
declares, fails loudly without a device, and its host logic (ingest semantics, planner)
is correct.  No compute calls on a GPU here."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import hbo
from stract_amd import _lib, dist, synth
from stract_amd.harmonic import EdgeListGraph, HarmonicCentrality
from tests import graphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_all_exported():
    hdr = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include"))))
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hb[wu]?_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    # and the Python binding covers exactly the declared set
    assert declared == set(_lib.SYMBOLS)
    assert _lib.load().hb_abi_version() == 6


def test_experiment_switch_names_agree_with_the_python_binding():
    """Every HB_X_* switch of stract_amd/csrc/hb_experiments.h exists in _lib with the same value, and vice versa; each is one bit of
    hb_options.tune[1] above the low byte (the gather unroll), and no two share a bit."""
    text = open(os.path.join(ROOT, "stract_amd", "csrc", "hb_experiments.h")).read()
    header = {name: int(value, 16) for name, value in re.findall(r"^\s*(HB_X_[A-Z0-9_]+)\s*=\s*(0x[0-9A-Fa-f]+)u?\s*,", text, flags=re.M)}
    assert len(header) >= 17, sorted(header)
    binding = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith("HB_X_")}
    assert header == binding
    seen = 0
    for name, value in sorted(header.items()):
        assert value & (value - 1) == 0 and 0xFF < value <= 0xFFFFFFFF, (name, hex(value))
        assert not seen & value, "%s shares its bit with another switch" % name
        seen |= value
        assert _lib.needs_experiments_build((0, value)), name


def test_headers_are_plain_c99_and_struct_sizes_agree(tmp_path):
    """What a cgo / bindgen / JNI binding compiles is C, not C++: every header under include/ must pass a strict C99 compiler on its own,
    and the struct sizes the C compiler sees are the ones the Python binding (and INTEGRATION.md's Rust shim) assume."""
    import subprocess
    names = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    for name in names:  # each header alone: it must include what it needs
        src = tmp_path / ("only_" + name[:-2] + ".c")
        src.write_text('#include "%s"\nint main(void) { return 0; }\n' % name)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "o.o")])
    src = tmp_path / "sizes.c"
    src.write_text("".join('#include "%s"\n' % n for n in names) + '#include <stdio.h>\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(hb_options), sizeof(hb_stats), sizeof(hb_pass_stats), sizeof(hb_edge), sizeof(hb_u128)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [ctypes.sizeof(_lib.HbOptions), ctypes.sizeof(_lib.HbStats), ctypes.sizeof(_lib.HbPassStats), _lib.EDGE.itemsize, _lib.U128.itemsize], got


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_lib.HbOptions) == 4 * 7 + 128 + 32
    assert _lib.EDGE.itemsize == 40 and _lib.U128.itemsize == 16
    assert ctypes.sizeof(_lib.HbStats) == 29 * 8  # ABI 5: + result_stages, result_list, pipelined_passes, tail_kernel_passes
    assert ctypes.sizeof(_lib.HbPassStats) == 4 * 8 + 6 * 4


@pytest.mark.skipif(_lib.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_no_device_fails_loudly():
    with pytest.raises(_lib.HyperballError) as ei:
        _lib.Context()
    assert ei.value.code == _lib.HB_ERR_NO_DEVICE
    with pytest.raises(_lib.HyperballError):
        HarmonicCentrality.calculate(graphs.fixture_graph())


def test_null_ctx_is_rejected():
    lib = _lib.load()
    assert lib.hb_run(None, None) == _lib.HB_ERR_INVALID
    assert lib.hb_load_edges(None, None, 0, None, 0) == _lib.HB_ERR_INVALID
    lib.hb_destroy(None)  # no-op


def _reference_semantics_python(edges):
    """Plain-Python statement of store.rs:297-357 + harmonic.rs:131 for small inputs."""
    key = lambda r: ((int(r["from"]["hi"]) << 64) | int(r["from"]["lo"]), (int(r["to"]["hi"]) << 64) | int(r["to"]["lo"]))
    nodes = sorted({x for r in edges for x in key(r)})
    seen, kept = set(), []
    for r in edges:
        k = key(r)
        if k in seen:
            continue
        seen.add(k)
        if int(r["rel_flags"]) & 0x6FED00:
            continue
        kept.append(k)
    return nodes, len(seen), sorted(kept, key=lambda k: (k[1], k[0]))


def test_ingest_semantics_small():
    A, B, C, D = 5, (1 << 100) + 3, 7, (1 << 64)
    e = EdgeListGraph.from_tuples([(A, B, 0), (A, B, 1 << 8), (B, C, 1 << 13), (B, C, 0), (C, C, 0), (D, A, 1 << 21),
                                   (C, A, 1 << 12), (A, C, 0)]).host_edges()
    ids, row_ptr, src, mu = _lib.host_ingest(e)
    nodes, n_unique, kept = _reference_semantics_python(e)
    got_ids = [(int(h) << 64) | int(l) for l, h in zip(ids["lo"], ids["hi"])]
    assert got_ids == nodes                      # numeric u128 order; D only via a flagged edge
    assert mu == n_unique == 6
    got = [(got_ids[s], got_ids[v]) for v in range(len(ids)) for s in src[row_ptr[v]:row_ptr[v + 1]]]
    assert got == kept
    assert (B, C) not in kept and (C, A) in kept  # flagged-first stays lost; harmless flag bit 12 kept


def test_ingest_matches_python_on_salted_rmat():
    g = synth.RmatGraph(9, 3000)
    e = g.edges(salt=1, salt_seed=3)
    ids, row_ptr, src, mu = _lib.host_ingest(e)
    nodes, n_unique, kept = _reference_semantics_python(e)
    got_ids = [(int(h) << 64) | int(l) for l, h in zip(ids["lo"], ids["hi"])]
    assert got_ids == nodes and mu == n_unique
    got = [(got_ids[s], got_ids[v]) for v in range(len(ids)) for s in src[row_ptr[v]:row_ptr[v + 1]]]
    assert got == kept
    # explicit node list (graph.host_nodes()) gives the same reduction, any order, duplicates ok
    shuffled = np.concatenate([ids[::-1], ids[:5]])
    ids2, rp2, src2, mu2 = _lib.host_ingest(e, shuffled)
    assert np.array_equal(ids2, ids) and np.array_equal(rp2, row_ptr) and np.array_equal(src2, src)


def test_ingest_edge_cases():
    ids, row_ptr, src, mu = _lib.host_ingest(np.zeros(0, dtype=_lib.EDGE))
    assert len(ids) == 0 and row_ptr.tolist() == [0] and len(src) == 0 and mu == 0
    # records whose endpoint is not in the supplied node set are ignored (harmonic.rs:135)
    e = EdgeListGraph.from_tuples([(1, 2), (2, 3), (9, 1)]).host_edges()
    ids, row_ptr, src, mu = _lib.host_ingest(e, graphs.dense_from_tuples([(1, 2), (2, 3)])[0])
    assert len(ids) == 3 and len(src) == 2


def _expand(plan, row, n_pad):
    out = []
    for s in plan["src"][int(plan["row_ptr"][row]):int(plan["row_ptr"][row + 1])]:
        out.extend(_expand(plan, int(s), n_pad) if s >= n_pad else [int(s)])
    return out


@pytest.mark.parametrize("chunk,flags,tune", [(4, 0, ()), (16, 0, ()), (64, 0, ()), (8, _lib.HB_FLAG_NO_REORDER, ()),
                                              (16, 0, (0, 0, 0, 6, 4)), (64, 0, (0, 0, 0, 5, 8, 16)),
                                              (32, 0, (0, 0, 0, 1)), (16, _lib.HB_FLAG_NO_XCD_MAP, (0, 0, 0, 6, 4)),
                                              (8, 0, (0, 0, 0, 4, 2))])
def test_planner_invariants(chunk, flags, tune):
    # tune[3] = log2 of the hottest source band (1 = banding off), tune[4] = min sources before a band
    # cut, tune[5] = largest row that is not split
    g = synth.RmatGraph(12, 40_000)
    plan = _lib.host_plan(g.row_ptr, g.src, flags, chunk, tune)
    n, n_pad = g.n, plan["n_pad"]
    order = plan["order"].astype(np.int64)
    assert sorted(order.tolist()) == list(range(n))          # a permutation
    if flags & _lib.HB_FLAG_NO_REORDER:
        assert np.array_equal(order, np.arange(n))
    else:
        outdeg = np.bincount(g.src, minlength=n)
        assert np.all(np.diff(outdeg[order]) <= 0)            # hottest sources first
    dev_of = np.zeros(n, np.int64)
    dev_of[order] = np.arange(n)
    lens = np.diff(plan["row_ptr"].astype(np.int64))
    assert lens.max() <= chunk                                # no work row longer than chunk
    lb = plan["level_begin"].astype(np.int64)
    assert lb[0] == n_pad and np.all(lb % 64 == 0) and np.all(np.diff(lb) > 0) and lb[-1] == n_pad + plan["nv"]
    # level discipline: level-1 rows read real nodes, level-l rows read level l-1 only,
    # real rows read either only real nodes or only virtual rows
    for l in range(len(lb) - 1):
        for row in range(lb[l], lb[l + 1]):
            s = plan["src"][int(plan["row_ptr"][row]):int(plan["row_ptr"][row + 1])]
            if len(s) == 0:
                continue
            if l == 0:
                assert s.max() < n
            else:
                assert s.min() >= lb[l - 1] and s.max() < lb[l]
    for d in range(n):
        s = plan["src"][int(plan["row_ptr"][d]):int(plan["row_ptr"][d + 1])]
        assert len(s) == 0 or s.max() < n or s.min() >= n_pad
        sid = order[d]
        want = sorted(dev_of[g.src[int(g.row_ptr[sid]):int(g.row_ptr[sid + 1])]].tolist())
        assert sorted(_expand(plan, d, n_pad)) == want        # the tree covers exactly the row's in-edges


@pytest.mark.parametrize("world", [2, 3, 8])
def test_planner_owner_slices(world):
    """Destination partition layout: `world` equal slices, slice g = the sids with sid % world == g in
    descending out-degree order; the trees still cover exactly every row's in-edges."""
    g = synth.RmatGraph(11, 15_000)
    plan = _lib.host_plan(g.row_ptr, g.src, 0, 16, (0, 0, 0, 6, 4, 0, 0, world))
    n, n_pad, S = g.n, plan["n_pad"], plan["slice"]
    order = plan["order"].astype(np.int64)
    assert n_pad == S * world and S % 64 == 0 and len(order) == n_pad
    real = order != 0xFFFFFFFF
    assert sorted(order[real].tolist()) == list(range(n))
    outdeg = np.bincount(g.src, minlength=n)
    for r in range(world):
        sl = order[r * S:(r + 1) * S]
        sids = sl[sl != 0xFFFFFFFF]
        assert np.all(sids % world == r)
        assert np.all(sl[len(sids):] == 0xFFFFFFFF)          # padding rows at the end of each slice
        assert np.all(np.diff(outdeg[sids]) <= 0)
    dev_of = np.zeros(n, np.int64)
    dev_of[order[real]] = np.nonzero(real)[0]
    for d in np.nonzero(real)[0][::7]:
        sid = order[d]
        want = sorted(dev_of[g.src[int(g.row_ptr[sid]):int(g.row_ptr[sid + 1])]].tolist())
        assert sorted(_expand(plan, int(d), n_pad)) == want
    for d in np.nonzero(~real)[0]:
        assert plan["row_ptr"][d] == plan["row_ptr"][d + 1]


def test_planner_randomized_coverage():
    """Random small graphs x random knobs: every row's tree covers exactly its in-edges, rows obey the chunk
    limit, levels only read the level below."""
    rng = np.random.default_rng(20240922)
    for case in range(60):
        kind, edges = graphs.random_graph(rng)
        if not edges:
            continue
        ids, row_ptr, src = graphs.dense_from_tuples(edges)
        n = len(ids)
        chunk = int(rng.choice([4, 5, 8, 16, 64]))
        tune = (0, 0, 0, int(rng.integers(4, 9)), int(rng.integers(1, 9)), int(rng.integers(0, chunk + 1)), 0,
                int(rng.choice([0, 0, 2, 3])))
        flags = int(rng.choice([0, _lib.HB_FLAG_NO_REORDER, _lib.HB_FLAG_NO_XCD_MAP]))
        plan = _lib.host_plan(row_ptr, src, flags, chunk, tune)
        n_pad = plan["n_pad"]
        order = plan["order"].astype(np.int64)
        real = np.nonzero(order != 0xFFFFFFFF)[0] if len(order) == n_pad else np.arange(n)
        sids = order[real] if len(order) == n_pad else order
        assert sorted(sids.tolist()) == list(range(n)), (case, kind)
        dev_of = np.zeros(n, np.int64)
        dev_of[sids] = real
        lens = np.diff(plan["row_ptr"].astype(np.int64))
        assert lens.max(initial=0) <= chunk, (case, kind, chunk)
        for d, sid in zip(real.tolist(), sids.tolist()):
            want = sorted(dev_of[src[int(row_ptr[sid]):int(row_ptr[sid + 1])]].tolist())
            assert sorted(_expand(plan, d, n_pad)) == want, (case, kind, chunk, tune, flags)


def test_planner_deep_hub():
    # one destination with 5000 in-edges and chunk 4 needs a 6-level tree
    n = 5001
    row_ptr = np.zeros(n + 1, dtype=np.uint64)
    row_ptr[1:] = 5000
    src = np.arange(1, 5001, dtype=np.uint32)
    plan = _lib.host_plan(row_ptr, src, _lib.HB_FLAG_NO_REORDER, 4)
    assert len(plan["level_begin"]) - 1 == 6
    assert sorted(_expand(plan, 0, plan["n_pad"])) == list(range(1, 5001))


def test_partition_helpers():
    g = synth.RmatGraph(10, 6000)
    e = g.edges(salt=1, salt_seed=5)
    parts = [dist.partition_edges(e, r, 3) for r in range(3)]
    assert sum(len(p) for p in parts) == len(e)
    owner = dist.edge_owner(e, 3)
    # all records of one (from,to) pair live on one rank
    keys = {}
    for r, rec in zip(owner.tolist(), e):
        k = (int(rec["from"]["lo"]), int(rec["from"]["hi"]), int(rec["to"]["lo"]), int(rec["to"]["hi"]))
        assert keys.setdefault(k, r) == r
    # dense partition: disjoint cover, CSR consistent
    tot = []
    for r in range(3):
        rp, s = dist.partition_dense(g.row_ptr, g.src, r, 3)
        assert rp[0] == 0 and rp[-1] == len(s) and np.all(np.diff(rp.astype(np.int64)) >= 0)
        for v in (0, 1, g.n // 2, g.n - 1):
            full = g.src[int(g.row_ptr[v]):int(g.row_ptr[v + 1])]
            idx = np.arange(int(g.row_ptr[v]), int(g.row_ptr[v + 1]))
            assert np.array_equal(s[int(rp[v]):int(rp[v + 1])], full[idx % 3 == r])
        tot.append(len(s))
    assert sum(tot) == g.m
    # destination partition: rank r holds exactly the rows r mod world, complete
    tot = 0
    for r in range(3):
        rp, s = dist.partition_dense_by_dest(g.row_ptr, g.src, r, 3)
        assert rp[0] == 0 and rp[-1] == len(s)
        for v in range(0, g.n, 97):
            mine = s[int(rp[v]):int(rp[v + 1])]
            full = g.src[int(g.row_ptr[v]):int(g.row_ptr[v + 1])]
            assert np.array_equal(mine, full if v % 3 == r else full[:0])
        tot += len(s)
    assert tot == g.m
    ids = g.ids
    owner = dist.dest_owner_of_edges(e, np.unique(np.concatenate([e["from"], e["to"]])), 3)
    assert owner.min() >= 0 and owner.max() <= 2


def test_host_stages_under_sanitizers(tmp_path):
    """tools/asan_host_check.cpp: ingest + planner on 300 random inputs / knob sets under AddressSanitizer and
    UBSan, with the coverage invariant re-checked in C++ (sanitizer runs of the host code)."""
    import shutil
    import subprocess

    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_host_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tools", "asan_host_check.cpp"), os.path.join(ROOT, "stract_amd", "csrc", "hb_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available")
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "asan_host_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_streamed_export_reduces_to_clean_graph():
    """stract_amd/csrc/hb_synth.cpp hbs_stream_*: the record stream used to feed BASELINE-sized graphs through the real
    boundary (hb_append_edges) slab by slab.  Claim: under the reference semantics (store.rs:313 first occurrence,
    harmonic.rs:131 filter after) the salted stream reduces to EXACTLY the clean graph.  Checked against the
    structure-faithful oracle on the records and the host ingest; slabs of any size give the same bytes."""
    from oracle import hbo
    for scale, m in ((10, 6000), (13, 60_000)):
        g = synth.RmatGraph(scale, m)
        for salt in (0, 2):
            total = g.stream_len(salt)
            full = np.zeros(total, dtype=_lib.EDGE)
            assert g.stream_fill(full, 0, salt) == total
            parts = np.concatenate([sl.copy() for sl in g.stream(salt, slab=4097)])
            assert parts.tobytes() == full.tobytes()
            assert total == g.m + (g.m // 15) * 3 * (salt == 2)
            ids, rp, src, m_unique = _lib.host_ingest(full)
            assert np.array_equal(ids, g.ids) and np.array_equal(rp, g.row_ptr) and np.array_equal(src, g.src)
            assert m_unique == g.m + g.stream_lost_pairs(salt)
            if salt == 2:
                flagged = (full["rel_flags"] & np.uint64(0x6FED00)) != 0
                assert 0.1 < flagged.mean() < 0.2 and g.stream_lost_pairs(2) > g.m // 20
            fids, fvals, fst = hbo.faithful_run(full)
            o = hbo.Dense(g.id_low64(), g.row_ptr, g.src)
            T = o.run()
            ovals, keep, k = o.finish()
            assert (fst["n"], fst["m_eff"], fst["m_unique"], fst["passes"]) == (g.n, g.m, m_unique, T)
            assert np.array_equal(fids, g.ids[keep]) and np.array_equal(fvals.view(np.uint64), ovals[keep].view(np.uint64))


def test_tail_index_filter_and_mapping():
    """hb_debug_tail_index (host only): the index behind hb_load_tail_edges - what ForwardlinksQuery::new(host) yields from
    the documents (one segment, doc order; LinksScorer restated independently in oracle/pyref.py), then the rel filter and
    the two lookups (harmonic.rs:87,91-92), as a CSR by source device row, duplicates dropped."""
    import ctypes
    from tests import graphs
    lib = _lib.load()
    rng = np.random.default_rng(4)
    n, n_pad = 300, 320
    vals = sorted(int(x) for x in rng.choice(1 << 40, size=n, replace=False))
    ids = np.zeros(n, dtype=_lib.U128)
    ids["lo"] = np.array(vals, dtype=np.uint64)
    ids["hi"] = np.arange(n, dtype=np.uint64) % 3           # ascending (hi, lo) order is required
    order = np.lexsort((ids["lo"], ids["hi"]))
    ids = ids[order]
    dev_of = rng.permutation(n_pad)[:n].astype(np.uint32)
    m = 4000
    recs = np.zeros(m, dtype=_lib.EDGE)
    f, t = rng.integers(0, n, m), rng.integers(0, n, m)
    recs["from"], recs["to"] = ids[f], ids[t]
    foreign = rng.random(m) < 0.1
    recs["from"]["lo"][foreign] ^= np.uint64(1 << 50)      # not a host id: falls out at the lookup
    flagged = rng.random(m) < 0.2
    recs["rel_flags"][flagged] = graphs.NOFOLLOW
    recs["rel_flags"][~flagged & (rng.random(m) < 0.3)] = 1  # a flag outside SKIPPED_REL: kept
    recs[:50] = recs[50:100]                                # duplicates far apart in the stream
    # neighbouring duplicates with conflicting flags: flagged first (the link is lost) / clean first (kept) - the query's
    # LinksScorer keeps the first of a run, harmonic.rs:87 filters on the survivor (query/raw/links.rs:115-232)
    for k in range(200, 400, 4):
        recs[k + 1] = recs[k]
        recs["rel_flags"][k] = graphs.NOFOLLOW if (k // 4) % 2 else 0
        recs["rel_flags"][k + 1] = 0 if (k // 4) % 2 else graphs.NOFOLLOW
    recs[400:460]["to"] = recs[400:460]["from"]             # self links: skipped by the query
    from oracle import pyref
    key = {(int(r["hi"]) << 64) | int(r["lo"]): i for i, r in enumerate(ids)}
    as_int = lambda v: (int(v["hi"]) << 64) | int(v["lo"])
    pages = [(as_int(r["from"]), as_int(r["to"]), int(r["rel_flags"])) for r in recs]
    fwd = pyref.forwardlinks_result(pages, set(key))
    want = {(int(dev_of[key[f]]), int(dev_of[key[t]])) for f, ts in fwd.items() for t in ts}
    naive = {(int(dev_of[key[f]]), int(dev_of[key[t]])) for f, t, fl in pages if not fl & 0x6FED00 and f in key and t in key}
    assert want < naive                                     # "any record that passes" would keep more
    ptr = np.zeros(n_pad + 1, dtype=np.uint64)
    to = np.zeros(m, dtype=np.uint32)
    k = ctypes.c_uint64(0)
    rc = lib.hb_debug_tail_index(n, ids.ctypes.data, dev_of.ctypes.data, n_pad, recs.ctypes.data, m, ptr.ctypes.data, to.ctypes.data, m,
                                 ctypes.byref(k))
    assert rc == 0 and k.value == len(want) and int(ptr[-1]) == len(want) and 0 < len(want) < m
    got = [(row, int(x)) for row in range(n_pad) for x in to[int(ptr[row]):int(ptr[row + 1])]]
    assert got == sorted(want)
    rc = lib.hb_debug_tail_index(n, ids.ctypes.data, dev_of.ctypes.data, n_pad, None, 0, ptr.ctypes.data, to.ctypes.data, m, ctypes.byref(k))
    assert rc == 0 and k.value == 0 and not ptr.any()


def test_bench_finds_the_committed_pmc_launch_classes():
    """bench.py's roofline.traffic is read from profiles/current_<config>_pmc.json by kernel NAME: a renamed template
    argument list silently turns it into null.  Every committed summary must resolve both dense launch classes."""
    import glob
    import bench
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "current_*_pmc.json")))
    assert files, "no committed PMC summary"
    for f in files:
        config = os.path.basename(f)[len("current_"):-len("_pmc.json")]
        pmc = bench._pmc(config)
        for cls in ("hub_level1_dense", "node_rows_dense"):
            assert cls in pmc, (config, cls, "not matched: kernel names changed?")
            assert pmc[cls]["hbm_bytes_per_dispatch"] > 0 and 0 < pmc[cls]["l2_hit_rate"] < 1
            assert pmc[cls]["_kernel"].startswith("hbk::pass_kernel<")


def test_bench_has_no_net_under_the_record_path():
    """Round 3's bench reloaded through hb_load_dense when the record path failed and restarted a child that a signal had
    killed; both are gone: a failing hb_append_edges / hb_finalize propagates out of load_records (non-zero exit, no line)."""
    import inspect
    import bench

    assert not hasattr(bench, "supervise")
    src = inspect.getsource(bench.main)
    assert "load_dense" in src                      # the explicit --input dense / N > 1 paths still exist ...
    assert "record path FAILED" not in src          # ... but not as a fallback
    body = src[src.index('a.input == "records"'):]
    assert "except" not in body[:body.index("ctx.load_dense")]

    class Ctx:  # a context whose ingest does not reduce to the clean graph
        def append_edges(self, e):
            pass

        def finalize(self):
            pass

        def stats(self):
            return {"n": 1, "m_eff": 1, "m_input": 1, "ingest_peak_bytes": 0, "m_unique": 1}

    class G:
        n, m = 5, 7

        def stream_len(self, salt):
            return 3

        def stream_fill(self, buf, at, salt):
            return 3

    import pytest as _pt

    class FakePinned:  # no GPU here: hb_pinned_alloc needs one
        def __init__(self, count):
            self.array = np.zeros(count, dtype=_lib.EDGE)

        def close(self):
            pass

    real = _lib.PinnedRecords
    _lib.PinnedRecords = FakePinned
    try:
        with _pt.raises(RuntimeError, match="did not reduce to the clean graph"):
            bench.load_records(Ctx(), G())
    finally:
        _lib.PinnedRecords = real
