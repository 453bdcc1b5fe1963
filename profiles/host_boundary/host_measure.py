"""Config C (bench.py's survey schedule, 2^20 nodes) through a host-exchange
handle: ms per round of emit + absorb.  mode diag: lo = 0, hi = n;
mode mixed: the top 1/64 of the ids outside, absorbing an empty list."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from partisan_amd import workloads as W          # noqa: E402
from partisan_amd.sim import HostSim, _Driver, default_config   # noqa: E402

mode, steps, warmup = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
n = 1 << 20
hi = n if mode == "diag" else n - n // 64
pair = mode == "pair"      # a second handle owns the top 1/64 and the two exchange their outbound lists
NONE16 = np.zeros((0, 16), np.uint32)


class Drv:
    def __init__(self):
        self.s = HostSim(default_config(n_nodes=n, seed=1), 0, hi)
        self.b = HostSim(default_config(n_nodes=n, seed=1), hi, n) if pair else None
        self.kt, self.rounds = {}, 0

    def broadcast(self, *a):
        self.s.broadcast(*a)
        if self.b: self.b.broadcast(*a)

    def join(self, *a):
        self.s.join(*a)
        if self.b: self.b.join(*a)

    def one(self):
        self.s.emit()
        if self.b:
            self.b.emit()
            ao, bo = self.s.outbound(), self.b.outbound()
            st = self.s.absorb(bo)
            self.b.absorb(ao)
        else:
            st = self.s.absorb(NONE16)
        for name, (ms, cnt) in self.s.kernel_times().items():
            a, b = self.kt.get(name, (0.0, 0))
            self.kt[name] = (a + ms, b + cnt)
        self.rounds += 1
        return st

    def __getattr__(self, k):
        return getattr(self.s, k)

    @property
    def round(self):
        return self.s.round

    def step(self, k=1):
        st = []
        for _ in range(k):
            st.append(self.one())
        return np.concatenate(st)

    run_schedule = _Driver.run_schedule


d = Drv()
sched = W.BenchSchedule("C", "survey", n, 1, warmup)
boot, until = sched.bootstrap()
d.run_schedule(boot, until)
for i in range(sched.t_start):
    sched.apply(d, i)
    d.step(1)
whole = {"rounds": d.rounds, "records": d.s.exchange_stats()[0],
         "kernel_ms_total": {k: (round(v[0], 4), v[1]) for k, v in d.kt.items() if k.startswith("k_host") and v[1]}}
d.kt = {}
x0 = d.s.exchange_stats()
t0 = time.perf_counter()
for i in range(steps):
    sched.apply(d, sched.t_start + i)
    d.one()
dt = time.perf_counter() - t0
x1 = d.s.exchange_stats()
kt = d.kt
print(json.dumps({"mode": mode, "nodes": n, "owned": hi, "steps": steps, "ms_per_round": 1e3 * dt / steps,
                  "records_per_round": (x1[0] - x0[0]) / steps, "before_window": whole,
                  "kernel_ms_per_round": {k: v[0] / steps for k, v in kt.items() if v[1]},
                  "kernel_launches": {k: v[1] for k, v in kt.items() if k.startswith("k_host")},
                  "phase_timers": os.environ.get("PSIM_PHASE_TIMERS", "")}), flush=True)
