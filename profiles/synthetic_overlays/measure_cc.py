"""psim_get_histograms on config C (bench.py's survey schedule): the getter's
wall time over `reps` calls and what it counts, one JSON line.  PSIM_LIB=<variant>
selects another build of the library (partisan_amd/_lib.py), so the same
command measures the parent commit's library beside this one's.

  python profiles/synthetic_overlays/measure_cc.py --nodes 262144"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partisan_amd import Simulator, workloads as W  # noqa: E402
from partisan_amd.sim import default_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 18)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    sched = W.BenchSchedule("C", "survey", a.nodes, a.seed, warmup=5)
    boot, until = sched.bootstrap()
    sim = Simulator(default_config(n_nodes=a.nodes, seed=a.seed))
    sim.run_schedule(boot, until)
    sim.histograms()                                 # (first call: allocations)
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        h = sim.histograms()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    print(json.dumps(dict(lib=os.environ.get("PSIM_LIB", "") or "this", nodes=a.nodes, rounds=until,
                          components=h["components"], largest_component=h["largest_component"],
                          active_links=h["active_links"], symmetric_links=h["symmetric_links"],
                          ms_median=round(ms[len(ms) // 2], 3), ms_min=round(ms[0], 3), ms_max=round(ms[-1], 3))))
    sim.close()


if __name__ == "__main__":
    main()
