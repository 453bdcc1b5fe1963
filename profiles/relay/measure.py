"""Time of relay_reach() with 64 seeded pairs (relay_report.seeded_pairs) at one
ttl, beside graph_metrics() with 64 sources on the same handle, the device
yardstick.  The overlay is the one of overlay_report (doubling bootstrap plus
10 settle rounds).  Each call is timed `--reps` times after one untimed call
(host clock around calls that end in a device synchronise); the best counts.
The call without cases is the census (and, on shards, the gather) alone, so
flood_s = call - census.  --ab times the call under both PSIM_RELAY_LANES
values, alternating on the same handle.  --host also takes the host route:
nodes() in chunks and tests/_relay.py over them, and records whether the two
structs are equal.  One JSON line per ttl, appended to measure_n<nodes>.jsonl
in --out.

    python profiles/relay/measure.py --nodes 1048576 --host --ab
    python profiles/relay/measure.py --nodes 16777216 --ab
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from partisan_amd import relay_report as Q  # noqa: E402
from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.overlay_report import SETTLE  # noqa: E402
from partisan_amd.sim import Simulator, default_config  # noqa: E402

CHUNK = 1 << 16


def _timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t0, 5))
    return r, out


def _host(sim, cases):
    import _relay as P
    t0 = time.perf_counter()
    rows = []
    for lo in range(0, sim.n, CHUNK):
        rows += P.rows_of(sim.nodes(lo, min(CHUNK, sim.n - lo)))
    t1 = time.perf_counter()
    want = P.reference_rows(rows, cases)
    return want, round(t1 - t0, 3), round(time.perf_counter() - t1, 3)


def measure(n, seed, ttls, reps, host, ab):
    sched = W.doubling_join(n, seed)
    with Simulator(default_config(n_nodes=n, seed=seed)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + SETTLE)
        pairs = Q.seeded_pairs(n, seed)
        src, dst = [p[0] for p in pairs], [p[1] for p in pairs]
        _, gm = _timed(lambda: sim.graph_metrics(src), reps)
        _, census = _timed(lambda: sim.relay_reach([], [], 5), reps)
        for ttl in ttls:
            os.environ.pop("PSIM_RELAY_LANES", None)
            m, full = _timed(lambda: sim.relay_reach(src, dst, ttl), reps)
            rec = {"nodes": n, "seed": seed, "ttl": ttl, "relay_s": full, "census_s": census, "graph_metrics_s": gm,
                   "flood_s": round(min(full) - min(census), 5), "flood_share": round(1 - min(census) / min(full), 4),
                   "relay_over_graph_metrics": round(min(full) / min(gm), 4),
                   "peak_sum": int(m["peak"].sum()), "peak_max": int(m["peak"].max()), "levels_max": m["levels_max"],
                   "relays": int(m["relays"].sum()), "row": Q.row(m, ttl)}
            if ab:
                lanes = {"8": [], "1": []}
                for _ in range(reps):
                    for v in ("8", "1"):
                        os.environ["PSIM_RELAY_LANES"] = v
                        x, t = _timed(lambda: sim.relay_reach(src, dst, ttl), 1)
                        assert all(np.array_equal(x[k], m[k]) for k in m), v
                        lanes[v] += t
                os.environ.pop("PSIM_RELAY_LANES", None)
                rec["lanes_s"] = lanes
                rec["lane1_over_lane8"] = round(min(lanes["1"]) / min(lanes["8"]), 4)
            if host and ttl == ttls[0]:          # (the fetch is the same for every ttl: once)
                import _relay as P
                want, fetch_s, ref_s = _host(sim, [(s, d, ttl) for s, d in pairs])
                equal = all(np.array_equal(np.asarray(m[k], np.uint64), np.asarray(want[k], np.uint64))
                            for k in P.ARRAYS + P.HISTS) and all(int(m[k]) == int(want[k]) for k in P.SCALARS)
                rec.update({"host_fetch_s": fetch_s, "host_reference_s": ref_s, "host_equal": bool(equal),
                            "host_over_relay": round((fetch_s + ref_s) / min(full), 1)})
            yield rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--ttl", nargs="+", type=int, default=[5, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for rec in measure(a.nodes, a.seed, a.ttl, a.reps, a.host, a.ab):
        line = json.dumps(rec, sort_keys=True)
        with open(os.path.join(a.out, f"measure_n{a.nodes}.jsonl"), "a") as f:
            f.write(line + "\n")
        print(line, flush=True)


if __name__ == "__main__":
    main()
