"""Time of one resilience() call with the report's 64 cases beside two
existing calls of the same handle as yardsticks: graph_metrics() with 64
seeded sources and the handle's statistics call.  The overlay is the one of
overlay_report (doubling bootstrap plus 10 settle rounds).  Each call is timed
`--reps` times after one untimed call (host clock around calls that end in a
device synchronise).  The same call capped at one BFS level gives the time
outside the BFS loop: setup_s = capped - (full - capped) / (levels - 1).  One
JSON line per overlay, appended to measure_n<nodes>.jsonl in --out.

    python profiles/resilience/measure.py --nodes 1048576 --kind hv scamp
    python profiles/resilience/measure.py --nodes 16777216 --kind hv scamp
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partisan_amd import resilience_report as P  # noqa: E402
from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.sim import Simulator, default_config  # noqa: E402


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return r, out


def measure(n, seed, kind, reps):
    extra = dict(manager=1, strategy=2, scamp_c=5) if kind == "scamp" else {}
    sched = W.doubling_join(n, seed)
    with Simulator(default_config(n_nodes=n, seed=seed, **extra)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + P.SETTLE)
        stats = sim.strategy_histograms if kind == "scamp" else sim.histograms
        cases = P.cases(P.live_sources(sim, seed))
        stats(), sim.graph_metrics(seed=seed), sim.resilience(*cases, fail_seed=P.FAIL_SEED)
        m, res_s = _timed(lambda: sim.resilience(*cases, fail_seed=P.FAIL_SEED), reps)
        _, cap1_s = _timed(lambda: sim.resilience(*cases, fail_seed=P.FAIL_SEED, max_levels=1), reps)
        g, graph_s = _timed(lambda: sim.graph_metrics(seed=seed), reps)
        h, stats_s = _timed(stats, reps)
    assert m["links"] == g["links"] == h["links" if kind == "scamp" else "active_links"]
    full, cap1, lv = min(res_s), min(cap1_s), m["levels"]
    level_s = (full - cap1) / (lv - 1) if lv > 1 else 0.0
    setup_s = cap1 - level_s
    return {"kind": kind, "nodes": n, "seed": seed, "lib": os.environ.get("PSIM_LIB", ""), "n_up": m["n_up"],
            "links": m["links"], "levels": lv, "graph_levels": g["levels"],
            "resilience_s": res_s, "resilience_1level_s": cap1_s, "graph_s": graph_s, "stats_s": stats_s,
            "level_s": round(level_s, 5), "setup_s": round(setup_s, 4), "outside_bfs_share": round(setup_s / full, 3),
            "reliability": [round(r["reliability"], 4) for r in P.rows(m)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--kind", nargs="+", default=["hv"], choices=["hv", "scamp"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for kind in a.kind:
        line = json.dumps(measure(a.nodes, a.seed, kind, a.reps), sort_keys=True)
        with open(os.path.join(a.out, f"measure_n{a.nodes}.jsonl"), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)


if __name__ == "__main__":
    main()
