"""Time of one latency_metrics() call (64 seeded sources) beside graph_metrics()
on the same handle and sources -- the nearest existing call: the same link
set, a hop BFS instead of weighted sweeps.  The overlay is latency_report's
(doubling bootstrap plus `--rounds` rounds, X-BOT optimizing every
`--xbot-period`); each call is timed `--reps` times after one untimed call
(host clock around calls that end in a device synchronise).  The call is timed
under each of the kernel choices the library reads from the environment at the
call: PSIM_LAT_PUSH (walk over all nodes | compacted frontier list) and
PSIM_LAT_CELL (cell array | xbot_latency per link); every setting must return
the same struct.  One JSON line per overlay.

    python profiles/latency/measure.py --nodes 1048576 --kind hv xbot
    python profiles/latency/measure.py --nodes 16777216 --kind hv xbot
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.sim import Simulator, default_config  # noqa: E402

SETTINGS = (("walk", "cell"), ("list", "cell"), ("walk", "link"), ("list", "link"))


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return r, out


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def measure(n, seed, kind, reps, rounds, period):
    extra = dict(manager=2, xbot_period=period) if kind == "xbot" else {}
    sched = W.doubling_join(n, seed)
    with Simulator(default_config(n_nodes=n, seed=seed, **extra)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + rounds)
        sim.graph_metrics(seed=seed)
        g, graph_s = _timed(lambda: sim.graph_metrics(seed=seed), reps)
        sim.latency_metrics([])
        _, census_s = _timed(lambda: sim.latency_metrics([]), reps)
        first, by = None, {}
        for push, cell in SETTINGS:
            os.environ["PSIM_LAT_PUSH"], os.environ["PSIM_LAT_CELL"] = push, cell
            sim.latency_metrics(seed=seed)
            m, lat_s = _timed(lambda: sim.latency_metrics(seed=seed), reps)
            first = first or m
            assert _same(m, first), (push, cell)
            best = min(lat_s)
            by[f"{push}+{cell}"] = {"latency_s": lat_s, "ms_per_sweep": round((best - min(census_s)) * 1e3 / m["sweeps"], 3),
                                    "over_graph": round(best / min(graph_s), 2)}
        os.environ.pop("PSIM_LAT_PUSH"), os.environ.pop("PSIM_LAT_CELL")
        _, tree_s = _timed(lambda: sim.latency_metrics([], tree_root=0), reps) if sim.cfg.plumtree else (None, [])
    m = first
    assert m["links"] == g["links"] and m["n_up"] == g["n_up"]
    return {"kind": kind, "nodes": n, "seed": seed, "rounds": rounds, "xbot_period": period,
            "lib": os.environ.get("PSIM_LIB", ""), "n_up": m["n_up"], "links": m["links"],
            "sources_live": m["sources_live"], "sweeps": m["sweeps"], "bfs_levels": g["levels"],
            "graph_s": graph_s, "census_only_s": census_s, "tree_half_only_s": tree_s, "settings": by,
            "link_cost_mean": m["link_cost_sum"] / max(1, m["links"]),
            "hops_mean": g["dist_sum"] / max(1, g["pairs_reached"]),
            "latency_mean": m["lat_sum_all"] / max(1, m["pairs_reached"]), "latency_max": m["lat_max"],
            "pairs_unreached": m["pairs_unreached"], "row_bytes": 2 * 64 * 4 * n}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--kind", nargs="+", default=["hv"], choices=["hv", "xbot"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=60, help="rounds after the bootstrap's last join")
    ap.add_argument("--xbot-period", type=int, default=10)
    a = ap.parse_args()
    for kind in a.kind:
        print(json.dumps(measure(a.nodes, a.seed, kind, a.reps, a.rounds, a.xbot_period), sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
