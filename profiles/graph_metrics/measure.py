"""Time of one graph_metrics() call (64 seeded sources) beside the existing
statistics call of the same handle: the overlay of overlay_report (doubling
bootstrap plus 10 settle rounds), each call timed `--reps` times after one
untimed call of each (host clock around calls that end in a device
synchronise).  One JSON line per overlay.

    python profiles/graph_metrics/measure.py --nodes 1048576 --kind hv
    python profiles/graph_metrics/measure.py --nodes 16777216 --kind hv scamp
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

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
        sim.run_schedule(sched, sched[-1][0] + 1 + 10)
        stats = sim.strategy_histograms if kind == "scamp" else sim.histograms
        stats(), sim.graph_metrics(seed=seed)
        h, stats_s = _timed(stats, reps)
        g, graph_s = _timed(lambda: sim.graph_metrics(seed=seed), reps)
        _, cluster_s = _timed(lambda: sim.graph_metrics([]), reps)
    links = h["links" if kind == "scamp" else "active_links"]
    assert g["links"] == links
    return {"kind": kind, "nodes": n, "seed": seed, "lib": os.environ.get("PSIM_LIB", ""), "n_up": g["n_up"],
            "links": links, "levels": g["levels"],
            "stats_s": stats_s, "graph_s": graph_s, "clustering_only_s": cluster_s,
            "path_mean": g["dist_sum"] / max(1, g["pairs_reached"]), "path_max": g["ecc_max"],
            "pairs_unreached": g["pairs_unreached"], "sources_live": g["sources_live"],
            "clustering_mean": g["cl_sum_q32"] / 2.0 ** 32 / max(1, g["n_up"]),
            "transitivity": g["cl_closed"] / max(1, g["cl_pairs"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--kind", nargs="+", default=["hv"], choices=["hv", "scamp"])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for kind in a.kind:
        print(json.dumps(measure(a.nodes, a.seed, kind, a.reps), sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
