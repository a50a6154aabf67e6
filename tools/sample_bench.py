"""Time hb_sampled_harmonic (ApproxHarmonic, default k) on the R-MAT configs bench.py uses, next to one hb_run on the same context.

    python tools/sample_bench.py --configs C3,C4 --out profiles/sample_bench.json

Per config: 1 warm-up and --runs timed sampled runs (median reported; the dense-level ratio compares the medians over runs of the
largest dense level and of the largest dense pass of 3 hb_run), per level its mode / changed rows / GPU ms (of the median run),
k * m / t, and the yardstick from the same process and context: one hb_run and its dense passes' GPU ms (hb_get_pass_stats, mode 0).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stract_amd import _lib, synth  # noqa: E402

MODES = {1: "dense", 2: "bitmap", 4: "sweep"}


def bench(name, runs, seed):
    g, _, label = synth.make_config(name)
    out = {"config": name, "label": label, "n": int(len(g.ids)), "m": int(len(g.src))}
    with _lib.Context() as ctx:
        ctx.load_dense(g.ids, g.row_ptr, g.src)
        hb_runs = []
        for _ in range(3):  # the yardstick, run to run: the largest dense pass of each hb_run
            st = ctx.run()
            dense = [p["ms_gpu"] for p in ctx.pass_stats() if p["mode"] == 0]
            hb_runs.append(max(dense) if dense else None)
        out["hyperball"] = {"ms_loop": st["ms_loop"], "passes": st["passes"], "dense_pass_ms": dense,
                            "dense_pass_ms_max_per_run": hb_runs,
                            "dense_pass_ms_max": statistics.median([x for x in hb_runs if x is not None]) if any(x is not None for x in hb_runs) else None}
        ctx.sampled_harmonic(seed=seed)  # warm-up
        walls, stats = [], []
        for r in range(runs):
            t0 = time.perf_counter()
            s = ctx.sampled_harmonic(seed=seed + 1 + r)
            walls.append((time.perf_counter() - t0) * 1e3)
            stats.append(s)
        med = statistics.median(walls)
        s = stats[walls.index(sorted(walls)[len(walls) // 2])]
        out["sampled"] = {
            "k": s["k_req"], "sources": s["sources"], "batches": s["batches"], "results": s["results"],
            "ms_runs": walls, "ms_median": med, "k_m_per_s": s["sources"] * out["m"] / (med * 1e-3),
            "levels": [{"d": d + 1, "mode": "+".join(v for b, v in MODES.items() if s["level_modes"][d] & b) or "-",
                        "changed": s["level_changed"][d], "ms": s["level_ms"][d]} for d in range(s["levels"])],
        }
        lim = out["hyperball"]["dense_pass_ms_max"]
        per_run = [max([s_["level_ms"][d] for d in range(s_["levels"]) if s_["level_modes"][d] == 1] or [0.0]) for s_ in stats]
        out["sampled"]["dense_level_ms_max_per_run"] = per_run
        dl = statistics.median(per_run) if any(per_run) else None
        out["dense_level_over_dense_pass_max"] = (dl / lim) if (dl and lim) else None  # medians over runs of the largest dense level / pass
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,C4")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"tool": "tools/sample_bench.py", "results": [bench(c, a.runs, a.seed) for c in a.configs.split(",")]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
