"""Driver entry points: build() (CPU: hipcc cross-compiles without a GPU), bench.py's behaviour without a
device, smoke() on the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_entry_point():
    import __graft_entry__ as g

    g.build()  # incremental: a no-op when the libraries are up to date
    for rel in ("stract_amd/lib/libhyperball.so", "stract_amd/lib/libhb_synth.so", "oracle/libhb_oracle.so"):
        assert os.path.exists(os.path.join(ROOT, rel)), rel


def test_bench_refuses_to_run_without_a_gpu():
    from stract_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stdout + r.stderr)


def test_bench_help_lists_the_contract_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup"):
        assert flag in r.stdout


def test_bench_line_at_one_gpu_is_the_scaling_runs_first_point(monkeypatch):
    """The driver takes BENCH from `bench.py --steps K --warmup W` and the first point of the scaling curve from `bench.py --gpus 1
    --steps K --warmup W`; efficiency at N > 1 is computed against that point.  Both must be the SAME measurement of the SAME
    workload - BASELINE.json configs[3] (C4: the graph the north-star target is quoted on, 100M hosts / 2B edges) - and N > 1 must
    run that workload too (strong scaling), with the north-star decomposition (edge partition + all-reduce) as `value`."""
    import json

    import bench
    from stract_amd import synth

    monkeypatch.delenv("HB_BENCH_CONFIG", raising=False)
    monkeypatch.delenv("HB_BENCH_INPUT", raising=False)

    def args(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        return vars(bench.parse())

    plain, one, eight = args("--steps", "20", "--warmup", "5"), args("--gpus", "1", "--steps", "20", "--warmup", "5"), args("--gpus", "8", "--steps", "20", "--warmup", "5")
    assert plain == one
    assert {k: v for k, v in eight.items() if k != "gpus"} == {k: v for k, v in one.items() if k != "gpus"}
    assert one["config"] == "C4" and one["partition"] == "both" and one["parity"] == "auto" and one["input"] == "records"
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert "100M-host / 2B-edge" in base["configs"][3] and synth.CONFIGS["C4"]["label"] == "100M-host / 2B-edge"
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'main_part = "single" if world == 1 else ("dest" if a.partition == "dest" else "edge")' in src  # `value` at N > 1 = edge partition


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs: float64 files only, NodeIDs exact as 32-bit limbs, the whole list when it is short, a seeded sample of at most
    DUMP_SAMPLE positions (the same one for the same result count) when it is long; --steps below 1 is refused."""
    import numpy as np

    import bench
    from stract_amd._lib import U128

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--dump-outputs", str(tmp_path)])
    assert bench.parse().steps == 2

    def lst(k):
        rng = np.random.default_rng(k)
        ids = np.zeros(k, U128)
        ids["lo"] = rng.integers(0, 1 << 63, k, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        ids["hi"] = rng.integers(0, 1 << 63, k, dtype=np.uint64)
        return ids, rng.random(k)

    ids, vals = lst(1000)
    bench.dump_outputs(str(tmp_path / "short"), ids, vals, 7)
    d = {f[:-4]: np.load(str(tmp_path / "short" / f)) for f in os.listdir(str(tmp_path / "short"))}
    assert set(d) == {"result_count", "passes", "result_positions", "result_ids_u32x4", "result_values"}
    assert all(x.dtype == np.float64 for x in d.values())
    assert d["result_count"].tolist() == [1000] and d["passes"].tolist() == [7]
    assert d["result_positions"].tolist() == list(range(1000)) and np.array_equal(d["result_values"], vals)
    limbs = d["result_ids_u32x4"].astype(np.uint64)
    assert np.array_equal(limbs[:, 0] | (limbs[:, 1] << np.uint64(32)), ids["lo"])
    assert np.array_equal(limbs[:, 2] | (limbs[:, 3] << np.uint64(32)), ids["hi"])

    k = bench.DUMP_SAMPLE + 12345
    ids, vals = lst(k)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), ids, vals, 3)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 64 * 1000 * 1000
    for f in os.listdir(str(tmp_path / "a")):
        assert open(str(tmp_path / "a" / f), "rb").read() == open(str(tmp_path / "b" / f), "rb").read(), f
    pos = np.load(str(tmp_path / "a" / "result_positions.npy")).astype(np.int64)
    assert len(pos) == bench.DUMP_SAMPLE and np.all(np.diff(pos) > 0) and pos[-1] < k
    assert np.array_equal(np.load(str(tmp_path / "a" / "result_values.npy")), vals[pos])


@pytest.mark.gpu
def test_smoke_entry_point():
    import __graft_entry__ as g

    g.smoke()


@pytest.mark.gpu
def test_offline_bridge_tool(tmp_path):
    """tools/centrality_from_records.py on a dump of raw records = the operator mirror on the same records."""
    import numpy as np

    from oracle import hbo
    from stract_amd import synth
    from stract_amd.harmonic import EdgeListGraph, HarmonicCentrality

    g = synth.RmatGraph(11, 12_000)
    e = g.edges(salt=1, salt_seed=2)
    rec = tmp_path / "records.bin"
    e.tofile(str(rec))
    out = tmp_path / "out.csv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "centrality_from_records.py"), str(rec), str(out),
                        "--chunk-records", "5000"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [line.strip().split(",") for line in open(out)][1:]
    hc = HarmonicCentrality.calculate(EdgeListGraph(e))
    ids, vals = hc.arrays()
    assert [int(x[0], 16) for x in rows] == [(int(h) << 64) | int(l) for l, h in zip(ids["lo"], ids["hi"])]
    assert [float(x[1]) for x in rows] == vals.tolist()
    assert [int(x[2]) for x in rows] == hbo.rank_results(vals).tolist()
