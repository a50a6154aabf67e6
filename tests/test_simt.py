"""The library's DEVICE SOURCES under a SIMT interpreter on the host (tests/simt/simt.h: test infrastructure, not a compute path).

tests/simt builds stract_amd/csrc/*.hip - unchanged, kernels included - with the host compiler against a fake
<hip/hip_runtime.h> / <rocprim/rocprim.hpp> / <rccl/rccl.h>: the lanes of a workgroup run as fibers, cross-lane operations
(ballot, shuffles, DPP quad permutations, wavefront fences, __syncthreads) are served with min-PC re-convergence, device memory
is poisoned host memory, the device-side index checks of the `bounds` build are compiled in.  This test then runs a slice of
the GPU parity suite (tests/test_gpu.py, the very same test functions that run on the MI355X) against that build in a child
process: per-pass registers / Kahan words / sizes / changed counts of every pass mode and layout variant, the device ingest and
planner against the host ones, the logical-rank and one-rank-communicator exchanges, the reference-tail mode, the AMPC
operator - all compared with the oracle exactly as on the GPU.

What it proves: the LOGIC of the kernels (tiling, collectives, LDS hand-overs, bitmaps, lazy double buffer, epilogues) - so a
kernel change can be checked here before GPU minutes are spent on it.  What it cannot prove: anything about speed, about
memory ordering between workgroups (they run one after the other), or about the compiler's gfx950 code: the parity tests
proper remain the `-m gpu` tests.  stract_amd/_lib.py refuses to load this build unless HB_ALLOW_SIMT_INTERPRETER=1 (set
here, for the child only); __graft_entry__.smoke() and bench.py never see it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMT = os.path.join(ROOT, "tests", "simt")
LIB = os.path.join(SIMT, "_build", "libhyperball_simt.so")

# a slice of tests/test_gpu.py sized for the CPU suite (~2 minutes); HB_SIMT_FULL=1: everything the interpreter can run (~5 min)
# The per-pass variants under the plain order all run; under the live-first order (ids "<variant>-order_live") those of LIVE_QUICK:
# every pass mode, the chunk trees, the banded and sliced layouts, the lean pass 0, the staged results, the long tail and its kernel,
# and the variants that must ignore the flag.  The rest of that half runs with HB_SIMT_FULL=1.
LIVE_QUICK = ("default or chunk4_multilevel or sparse_always_multilevel or frontier_always_multilevel or frontier_always_chunk128 or "
              "no_reorder_unroll4 or unfused or pass_stats or staged_results_every_pass or staged_results_sweep_tiny_list or "
              "banded_chunks or xcd_slices_small_bands or few_blocks or sweep_general_seed_path or tail_kernel_after_any_pass")
PER_PASS = "(test_per_pass_state_matches_oracle and (not order_live or %s))" % LIVE_QUICK
QUICK = (PER_PASS + " or test_gpu_ingest_equals_host_ingest or test_device_plan_equals_host_plan or test_record_stream_whose_dead_hosts_occur_only_as_from or "
         "test_logical_ranks_on_one_device or test_rccl_call_path_single_rank or test_first_occurrence_flag_wins or "
         "test_empty_and_singleton_graphs or test_streamed_ingest_chunks_refusal_and_spill or test_ampc_counter_table_upsert_semantics")
# under a shuffled order: the plain half, and of the live half a chunk tree in each pass mode and the long tail
PER_PASS_SHUFFLED = ("(test_per_pass_state_matches_oracle and (not order_live or chunk4_multilevel or sparse_always_multilevel or "
                     "frontier_always_multilevel or long_tail_default))")
FULL = "not test_c2 and not test_caching_allocator_under_memory_pressure"


@pytest.fixture(scope="module")
def simt_lib():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++") and not os.environ.get("CLANG"):
        pytest.skip("no clang++ to build the interpreted library with")
    subprocess.check_call(["make", "-s", "-j8", "-C", SIMT])
    assert os.path.exists(LIB)
    return LIB


def _child_env(lib):
    return dict(os.environ, HB_LIB_PATH=lib, HB_ALLOW_SIMT_INTERPRETER="1", PYTHONPATH=ROOT)


def test_loader_refuses_the_interpreter_build_unless_asked(simt_lib):
    code = "from stract_amd import _lib\ntry:\n    _lib.load()\n    print('LOADED')\nexcept _lib.HyperballError as e:\n    print('REFUSED', e.code)\n"
    env = dict(os.environ, HB_LIB_PATH=simt_lib, PYTHONPATH=ROOT)
    env.pop("HB_ALLOW_SIMT_INTERPRETER", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.stdout.strip() == "REFUSED -2", r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_child_env(simt_lib), cwd=ROOT, timeout=120)
    assert r.stdout.strip() == "LOADED", r.stdout + r.stderr


def test_device_sources_match_the_oracle_under_the_interpreter(simt_lib):
    select = FULL if os.environ.get("HB_SIMT_FULL") == "1" else QUICK
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu.py"), "-m", "gpu", "-q", "-x", "-k", select,
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=_child_env(simt_lib), cwd=ROOT, timeout=1700)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail and "error" not in tail.lower(), tail


def test_reload_after_all_three_operators_under_the_interpreter(simt_lib):
    """tests/test_reload.py: what a load has to forget about the graph before it.  Device memory is poisoned host memory here, so a
    pointer or a size kept from the previous graph shows up without a GPU."""
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_reload.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=_child_env(simt_lib), cwd=ROOT, timeout=1700)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and "3 passed" in tail and "failed" not in tail, tail


def test_no_dependence_on_workgroup_or_lane_order(simt_lib):
    """The machine promises no order among the workgroups of a launch, nor among the lanes of a workgroup between two cross-lane
    operations.  The interpreter's default is ascending; HB_SIMT_ORDER=shuffle:<seed> takes a new random order of the workgroups for
    every launch and of the runnable lanes for every turn ("reverse": descending).  Results that depended on an order - one
    workgroup consuming what another has not produced yet, a lane reading LDS before its neighbour wrote it - would differ from the
    oracle here.  All per-pass variants under a shuffled order (the whole interpretable suite was run under reverse, shuffle:1 and
    shuffle:2 in round 4: 69 passed each).  HB_SIMT_FULL=1: both halves of the variant matrix, the live-first one whole."""
    env = dict(_child_env(simt_lib), HB_SIMT_ORDER="shuffle:7", HB_SIMT_THREADS="3")  # ... and three host threads share the workgroups: they overlap in time
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu.py"), "-m", "gpu", "-q", "-x", "-k",
                        ("test_per_pass_state_matches_oracle" if os.environ.get("HB_SIMT_FULL") == "1" else PER_PASS_SHUFFLED) +
                        " or test_sweep_seeds_with_very_long_reader_lists or test_gpu_ingest_equals_host_ingest",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=1700)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, tail


def test_bench_multi_rank_control_flow_on_the_interpreter(simt_lib, tmp_path):
    """`bench.py --gpus N` for N > 1 is the script the driver launches on an 8-GPU node - a node this repository has never had.
    `--collectives host-staged` runs the SAME code path (rendezvous, one context per rank, W + K runs bracketed by barriers, max over
    ranks, parity at N > 1 with the collective checksum re-run, the three extra decompositions under their watchdog, the JSON line)
    with gloo and host-staged exchanges in place of RCCL; here on the interpreted build with 2 ranks and the smallest BASELINE
    config.  Functional only - the line says so - but a Python-level mistake in the N > 1 path would show up here."""
    import json
    env = dict(_child_env(simt_lib), HB_BENCH_FUNCTIONAL="1", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    # [r6] launched the way the driver launches `--gpus 1`: plain `python bench.py --gpus 2` with NO launcher - the script must re-execute
    # itself under torch.distributed.run (one rank per GPU, rendezvous on 127.0.0.1, a free port) instead of exiting (VERDICT r5 #3a)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--config", "C1", "--collectives", "host-staged",
                        "--cpu-seconds", "5", "--full"], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=1500)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-1500:] + r.stderr[-3000:]
    assert "re-executing as" in r.stderr and "torch.distributed.run" in r.stderr, r.stderr[-1500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["warmup"] == 1 and d["metric"].startswith("HyperBall") and "FUNCTIONAL RUN" in d["data"]
    assert d["parity_bit_exact"] is True and d["config"]["parallelism"].startswith("edge-partition x2")
    legs = d["detail"]["partitions"]
    assert set(legs) == {"edge_changed_only", "dest_allgather", "dest_changed_only"}
    assert all(v["same_result_as_edge_partition"] is True for v in legs.values()), legs
    assert d["detail"]["collective"]["ran"] == "edge" and d["cpu_baseline"] is None
    best = d["best_decomposition"]  # [r6] the fastest leg with the main leg's results, at the top level of every N > 1 line
    assert best["name"] in set(legs) | {"edge_allreduce"} and best["value"] >= d["value"] and best["unit"] == "GTEPS", best
    # and the script still refuses the interpreted build for anything that would look like a measurement
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C1", "--steps", "1", "--c4-leg", "off"], capture_output=True, text=True,
                       env=_child_env(simt_lib), cwd=str(tmp_path), timeout=600)
    assert r.returncode != 0 and "gfx950 library only" in (r.stdout + r.stderr) and not any(ln.startswith("{") for ln in r.stdout.splitlines())


def _asan_runtime():
    r = subprocess.run([os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang++"), "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True)
    path = r.stdout.strip()
    return path if os.path.isabs(path) and os.path.exists(path) else None


def test_device_sources_under_address_sanitizer(simt_lib):
    """`make asan`: the interpreted build under AddressSanitizer, every "device" buffer an allocation of its exact size
    (-DHB_EXACT_ALLOC: no caching allocator, no planner slab): every load and store of every kernel - and of the stand-ins for
    the rocPRIM primitives - is checked against the bounds of the allocation it touches.  First the checker itself: a kernel
    that reads one element past a buffer must be caught, the same kernel inside its buffer must not.  Then GPU parity tests
    run under it.  Default: two per-pass variants (dense + bitmap + sweep passes, device ingest and planner on the way);
    HB_SIMT_ASAN=1: everything the interpreter can run (68 tests, ~16 min; profiles/r04_simt_asan_gpu_suite.txt)."""
    rt = _asan_runtime()
    if rt is None:
        pytest.skip("no AddressSanitizer runtime next to clang")
    subprocess.check_call(["make", "-s", "-j8", "-C", SIMT, "asan"])
    clang = os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang++")
    exe = os.path.join(SIMT, "_build_asan", "asan_selftest")
    subprocess.check_call([clang, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address", "-shared-libasan", "-fno-omit-frame-pointer",
                           "-I", os.path.join(SIMT, "include"), os.path.join(SIMT, "asan_selftest.cpp"), os.path.join(SIMT, "simt_core.cpp"),
                           os.path.join(SIMT, "simt_runtime.cpp"), "-o", exe, "-Wl,-rpath," + os.path.dirname(rt)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    ok = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert ok.returncode == 0 and ok.stdout.strip() == "clean 1000", ok.stdout + ok.stderr
    bad = subprocess.run([exe, "over"], capture_output=True, text=True, env=env, timeout=120)
    assert bad.returncode != 0 and "heap-buffer-overflow" in bad.stderr and "0 bytes after 4000-byte region" in bad.stderr, bad.stderr[-2000:]
    assert "sum_kernel" in bad.stderr  # ... and names the kernel's source line
    select = ("not test_c2 and not test_caching_allocator_under_memory_pressure and not test_multi_process" if os.environ.get("HB_SIMT_ASAN") == "1"
              else "test_per_pass_state_matches_oracle and (default or sparse_always_multilevel) and not long_tail")
    lib = os.path.join(SIMT, "_build_asan", "libhyperball_simt_asan.so")
    env = dict(_child_env(lib), LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu.py"), "-m", "gpu", "-q", "-x", "-k", select,
                        "-p", "no:cacheprovider"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=3400)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and "AddressSanitizer" not in r.stdout + r.stderr, tail
    assert " passed" in tail and "failed" not in tail, tail


@pytest.mark.skipif(os.environ.get("HB_SIMT_UBSAN") != "1", reason="opt-in (HB_SIMT_UBSAN=1, ~2 min): the interpreted device sources under UndefinedBehaviorSanitizer")
def test_device_sources_under_undefined_behaviour_sanitizer(simt_lib):
    """`make ubsan`: shift widths, signed overflow, misaligned accesses, out-of-range float -> integer casts in the device sources
    (the gfx950 compiler may assume none of them happens).  Round 4: 68 tests, no report (profiles/r04_simt_asan_gpu_suite.txt)."""
    rt = _asan_runtime()
    if rt is None:
        pytest.skip("no sanitizer runtimes next to clang")
    ub = os.path.join(os.path.dirname(rt), "libclang_rt.ubsan_standalone-x86_64.so")
    subprocess.check_call(["make", "-s", "-j8", "-C", SIMT, "ubsan"])
    lib = os.path.join(SIMT, "_build_ubsan", "libhyperball_simt_ubsan.so")
    env = dict(_child_env(lib), LD_PRELOAD=ub, UBSAN_OPTIONS="halt_on_error=1:abort_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu.py"), "-m", "gpu", "-q", "-x", "-s", "-k",
                        "not test_c2 and not test_caching_allocator_under_memory_pressure and not test_multi_process", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=3400)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and "runtime error" not in r.stdout + r.stderr, tail


@pytest.mark.skipif(os.environ.get("HB_SIMT_TSAN") != "1", reason="opt-in (HB_SIMT_TSAN=1, ~10 min): ThreadSanitizer over concurrently running workgroups and the loader's threads")
def test_kernels_and_loader_under_thread_sanitizer(simt_lib):
    """`make tsan` + HB_SIMT_THREADS=4: the workgroups of every launch are shared out among four host threads, i.e. they really run at
    the same time, and ThreadSanitizer sees every access of every kernel: two workgroups touching one address without atomics would
    be reported as the data race it is on the machine (workgroups run in no order and share nothing but global memory).  First the
    detector itself (tests/simt/race_selftest.cpp: a plain read-modify-write of one counter by all workgroups must be reported, the
    atomicAdd form must not).  Then the interpretable GPU suite.  The same build covers hb_load_webgraph's own threads (reader /
    checksum / hand-over, many-slab path).  Round 4: no report in any kernel or in the loader (libgomp-run test-support code is
    suppressed: tests/simt/tsan.supp)."""
    rt = _asan_runtime()
    if rt is None:
        pytest.skip("no sanitizer runtimes next to clang")
    ts = os.path.join(os.path.dirname(rt), "libclang_rt.tsan-x86_64.so")
    subprocess.check_call(["make", "-s", "-j8", "-C", SIMT, "tsan"])
    clang = os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang++")
    bdir = os.path.join(SIMT, "_build_tsan")
    subprocess.check_call([clang, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=thread", "-fno-omit-frame-pointer", "-I", os.path.join(SIMT, "include"),
                           "-c", os.path.join(SIMT, "race_selftest.cpp"), "-o", os.path.join(bdir, "race_selftest.o")])
    exe = os.path.join(bdir, "race_selftest")
    subprocess.check_call([clang, "-fsanitize=thread", "-shared-libsan", os.path.join(bdir, "race_selftest.o"), os.path.join(bdir, "simt_core.o"),
                           os.path.join(bdir, "simt_runtime.o"), "-o", exe, "-Wl,-rpath," + os.path.dirname(rt), "-lpthread"])
    env = dict(os.environ, HB_SIMT_THREADS="4")
    quiet = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert quiet.returncode == 0 and "ThreadSanitizer" not in quiet.stderr and quiet.stdout.strip() == "atomic 327680", quiet.stdout + quiet.stderr[-2000:]
    loud = subprocess.run([exe, "racy"], capture_output=True, text=True, env=env, timeout=300)
    assert "ThreadSanitizer: data race" in loud.stderr and "count_kernel" in loud.stderr, loud.stderr[-2000:]
    lib = os.path.join(bdir, "libhyperball_simt_tsan.so")
    env = dict(_child_env(lib), LD_PRELOAD=ts, HB_SIMT_THREADS="4", HB_SIMT_CUS="4",
               TSAN_OPTIONS="halt_on_error=1:abort_on_error=1:suppressions=" + os.path.join(SIMT, "tsan.supp"))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu.py"), "-m", "gpu", "-q", "-x", "-s", "-k",
                        "not test_c2 and not test_caching_allocator_under_memory_pressure and not test_multi_process", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=3400)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stdout + r.stderr, tail
