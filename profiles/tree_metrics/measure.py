"""Time of one tree_metrics() call beside two baselines on the same handle:
the overlay of overlay_report (doubling bootstrap plus 10 settle rounds, seed
31) after `--broadcasts` completed broadcasts from root 0.  Each call is timed
`--reps` times after one untimed call (host clock around calls that end in a
device synchronise): tree_metrics(0) with the row kernel's 16-lane layout and
with its 64-lane one (PSIM_TREE_LANES), graph_metrics([0]) and histograms().
--host: also the route the call replaces, nodes() in chunks plus the tests'
reference, whose result must equal the call's.  One JSON line.

    python profiles/tree_metrics/measure.py --nodes 262144 --host
    python profiles/tree_metrics/measure.py --nodes 1048576
    python profiles/tree_metrics/measure.py --nodes 16777216
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.sim import Simulator, default_config  # noqa: E402
from partisan_amd.tree_report import SETTLE, complete_broadcast, row  # noqa: E402


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return r, out


def _host_route(sim, root, got, chunk=1 << 16):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _tree_metrics as R
    t0 = time.perf_counter()
    rows = []
    for lo in range(0, sim.n, chunk):
        rows += R.rows_of(sim.nodes(lo, min(chunk, sim.n - lo)))
    t1 = time.perf_counter()
    want = R.reference_rows(rows, root)
    t2 = time.perf_counter()
    R.compare(got, want)
    return round(t1 - t0, 2), round(t2 - t1, 2)


def measure(n, seed, broadcasts, reps, host):
    sched = W.doubling_join(n, seed)
    with Simulator(default_config(n_nodes=n, seed=seed)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + SETTLE)
        done = []
        for k in range(1, broadcasts + 1):
            print(f"round {int(sim.round)}: broadcast {k}", file=sys.stderr, flush=True)
            done.append(complete_broadcast(sim, 0, k))
        out = {"nodes": n, "seed": seed, "lib": os.environ.get("PSIM_LIB", ""), "round": int(sim.round),
               "broadcast_rounds": [r for r, _ in done],
               "delivered": [int(d) for _, d in done]}
        for lanes in (16, 64):
            os.environ["PSIM_TREE_LANES"] = str(lanes)
            sim.tree_metrics(0)
            m, out[f"tree_lanes{lanes}_s"] = _timed(lambda: sim.tree_metrics(0), reps)
        del os.environ["PSIM_TREE_LANES"]
        sim.graph_metrics([0]), sim.histograms()
        g, out["graph_1src_s"] = _timed(lambda: sim.graph_metrics([0]), reps)
        h, out["histograms_s"] = _timed(sim.histograms, reps)
        assert m["overlay_reached"] == g["reach"][0] and m["n_up"] == h["n_up"]
        out.update(levels=m["levels"], overlay_levels=g["levels"], tree=row(m))
        if host:
            print("device calls timed; the host route", file=sys.stderr, flush=True)
            out["host_nodes_s"], out["host_reference_s"] = _host_route(sim, 0, m)
            out["host_equal"] = True
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--broadcasts", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    print(json.dumps(measure(a.nodes, a.seed, a.broadcasts, a.reps, a.host), sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
