"""What an armed message trace costs a round, on config C's overlay (bench.py's
workload: survey_join's ramp and warm-up, then the one broadcast from node 0).

    python profiles/trace/armed_cost.py MODE [--nodes N] [--rounds K] [--windows W]

MODE  unarmed   no watch (run it under PSIM_NO_BATCH=1 for the single-round
                path an armed handle takes by construction, and without for
                the batched path)
      watch64   64 nodes watched, both directions, every type
      watchall  every node watched
W windows of K rounds each are timed with a host clock around psim_step, which
ends in a device synchronise; the first window starts with the broadcast.  The
trace is read (untimed) after every window, so each window starts with an empty
buffer of `capacity` records.  Under PSIM_PHASE_TIMERS=1 the line also carries
psim_kernel_times' entries of the last window (the timers put a bubble between
kernels: take the round time from a run without them).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from partisan_amd import Simulator, workloads as W          # noqa: E402
from partisan_amd.sim import default_config                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["unarmed", "watch64", "watchall"])
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    n = a.nodes
    sched = W.BenchSchedule("C", "survey", n, a.seed, 5)
    sim = Simulator(default_config(n_nodes=n, seed=a.seed, device=0))
    boot, until = sched.bootstrap()
    sim.run_schedule(boot, until)
    if a.mode != "unarmed":
        ids = None
        if a.mode == "watch64":
            ids = np.random.Generator(np.random.PCG64([a.seed, 0x7A])).choice(n, size=64, replace=False)
        sim.trace_watch(ids, capacity=a.capacity)
    for i in range(sched.t_start):
        sched.apply(sim, i)
        sim.step(1)
    if a.mode != "unarmed":
        sim.trace_read()
    out = {"mode": a.mode, "nodes": n, "rounds": a.rounds, "capacity": a.capacity,
           "no_batch": "PSIM_NO_BATCH" in os.environ, "phase_timers": os.environ.get("PSIM_PHASE_TIMERS", "0"),
           "ms_per_round": [], "records": [], "lost": [], "emitted": []}
    for w in range(a.windows):
        if w == 0:
            sched.apply(sim, sched.t_start)
        t0 = time.perf_counter()
        st = sim.step(a.rounds)
        out["ms_per_round"].append(round((time.perf_counter() - t0) * 1e3 / a.rounds, 4))
        out["emitted"].append(int(st["emitted"].sum()))
        kt = sim.kernel_times()
        if a.mode != "unarmed":
            recs, _, lost = sim.trace_read()
            out["records"].append(len(recs))
            out["lost"].append(lost)
    out["kernel_ms"] = {k: [round(v[0], 4), int(v[1])] for k, v in kt.items() if v[1]}
    print(json.dumps(out, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
