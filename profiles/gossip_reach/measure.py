"""Time of gossip_reach() with the report's 64 cases (gossip_report.cases: 8
fanouts times 8 sources) per failed share, beside two calls of the same handle
with the same 64 (source, threshold, salt): resilience(), the yardstick, and
gossip_reach() with every fanout 0, which does that flood's BFS plus the
selection, one `sel` word per link and the tally.  The overlay is the one of
overlay_report (doubling bootstrap plus 10 settle rounds).  Each call is timed
`--reps` times after one untimed call (host clock around calls that end in a
device synchronise); the best counts.  The same call capped at one BFS level
gives the time outside the level loop -- link set, survivor words, selection
and tally (census and sweep for resilience()):
level_s = (full - capped) / (levels - 1), setup_s = capped - level_s.  One
JSON line per overlay and share, appended to measure_n<nodes>.jsonl in --out.

    python profiles/gossip_reach/measure.py --nodes 1048576 --kind hv scamp
    python profiles/gossip_reach/measure.py --nodes 16777216 --kind hv scamp
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partisan_amd import gossip_report as Q  # noqa: E402
from partisan_amd import resilience_report as P  # noqa: E402
from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.sim import Simulator, default_config  # noqa: E402


def _timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(round(time.perf_counter() - t0, 4))
    return r, out


def _split(fn, reps):
    """the call in full and capped at one level: its struct, both lists of times, level_s and setup_s"""
    m, full = _timed(lambda: fn(0), reps)
    _, cap1 = _timed(lambda: fn(1), reps)
    lv = m["levels"]
    level_s = (min(full) - min(cap1)) / (lv - 1) if lv > 1 else 0.0
    return m, {"s": full, "1level_s": cap1, "levels": lv, "truncated": m["truncated"], "level_s": round(level_s, 6),
               "setup_s": round(min(cap1) - level_s, 4)}


def measure(n, seed, kind, reps):
    extra = dict(manager=1, strategy=2, scamp_c=5) if kind == "scamp" else {}
    sched = W.doubling_join(n, seed)
    out = []
    with Simulator(default_config(n_nodes=n, seed=seed, **extra)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + P.SETTLE)
        sources = P.live_sources(sim, seed)
        for q in Q.SHARES:
            src, fan, thr, salt = Q.cases(sources, q)
            g, gossip = _split(lambda cap: sim.gossip_reach(src, fan, thr, salt, P.FAIL_SEED, cap), reps)
            f, flood = _split(lambda cap: sim.gossip_reach(src, np.zeros_like(fan), thr, salt, P.FAIL_SEED, cap), reps)
            r, res = _split(lambda cap: sim.resilience(src, thr, salt, P.FAIL_SEED, cap), reps)
            assert all(np.array_equal(f[k], r[k]) for k in ("alive", "reached", "hop_sum", "ecc"))
            assert f["levels"] == r["levels"] and g["links"] == r["links"]
            out.append({"kind": kind, "nodes": n, "seed": seed, "failed_share": q / 10, "n_up": g["n_up"],
                        "links": g["links"], "gossip": gossip, "flood": flood, "resilience": res,
                        "flood_over_resilience": round(min(flood["s"]) / min(res["s"]), 3),
                        "reliability": [round(x["reliability"], 4) for x in Q.rows(g, q, len(sources))]})
    return out


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
        for rec in measure(a.nodes, a.seed, kind, a.reps):
            line = json.dumps(rec, sort_keys=True)
            with open(os.path.join(a.out, f"measure_n{a.nodes}.jsonl"), "a") as f:
                f.write(line + "\n")
            print(line, flush=True)


if __name__ == "__main__":
    main()
