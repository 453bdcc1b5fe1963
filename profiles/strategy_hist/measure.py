"""Wall time of Simulator.strategy_histograms() against the host route to the
same means (strategy_nodes() over all nodes plus numpy, as
tests/d24_loopback.py takes view_mean / in_mean): a SCAMP v2 handle, the
doubling bootstrap, 40 rounds; one warm call, then the median of 5 (each call
ends in a device synchronise and a copy of the counters to the host).

    python profiles/strategy_hist/measure.py --nodes 1048576 [--nodes ...] --out timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partisan_amd import Simulator, _abi  # noqa: E402
from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.sim import default_config  # noqa: E402

ROUNDS, SEED, REPS = 40, 31, 5


def host_route(sim, n, chunk=1 << 20):
    """view_mean and in_mean from every node's strategy view on the host"""
    vs = ins = up = 0
    for lo in range(0, n, chunk):
        v = sim.strategy_nodes(lo, min(chunk, n - lo))
        live = v["up"] == 1
        vs += int(v["view_n"][live].sum()); ins += int(v["in_n"][live].sum()); up += int(live.sum())
    return vs / up, ins / up, up


def measure(n, host_reps):
    sim = Simulator(default_config(n_nodes=n, seed=SEED, manager=1, strategy=2, scamp_c=5))
    sim.run_schedule(W.doubling_join(n, SEED), ROUNDS)
    h = sim.strategy_histograms()                      # warm: code objects, first allocations
    dev = []
    for _ in range(REPS):
        t = time.perf_counter()
        h = sim.strategy_histograms()
        dev.append(time.perf_counter() - t)
    host = []
    for _ in range(host_reps):
        t = time.perf_counter()
        vm, im, up = host_route(sim, n)
        host.append(time.perf_counter() - t)
    sim.close()
    assert up == h["n_up"] and abs(vm - h["view_sum"] / up) < 1e-9 and abs(im - h["in_sum"] / up) < 1e-9
    return {"nodes": n, "rounds": ROUNDS, "seed": SEED, "n_up": h["n_up"], "links": h["links"],
            "view_mean": h["view_sum"] / up, "in_mean": h["in_sum"] / up,
            "components": h["components"], "largest_component": h["largest_component"],
            "strategy_histograms_s": {"median": statistics.median(dev), "all": dev},
            "strategy_nodes_numpy_s": {"median": statistics.median(host), "all": host},
            "host_bytes": n * _abi.STRATEGY_VIEW_DTYPE.itemsize,
            "speedup": statistics.median(host) / statistics.median(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, action="append", required=True)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default="timing.json")
    a = ap.parse_args()
    res = []
    for n in a.nodes:
        res.append(measure(n, a.host_reps))
        print(json.dumps(res[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"what": "strategy_histograms() wall time, median of 5 after one warm call, against "
                           "strategy_nodes() over all nodes plus numpy (the only route before); MI355X, one shard",
                   "runs": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
