"""One relay_reach() call of measure.py's 64 pairs on the overlay of
overlay_report, for a kernel trace of its own (rocprofv3 --kernel-trace
--stats -- python profiles/relay/one_call.py ...): the k_rl_* rows of the
trace's kernel statistics are that call's, PSIM_RELAY_LANES chooses the layout
of k_rl_expand.  Prints the levels and the frontier's sizes.

    python profiles/relay/one_call.py --nodes 1048576 --ttl 8
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from partisan_amd import relay_report as Q  # noqa: E402
from partisan_amd import workloads as W  # noqa: E402
from partisan_amd.overlay_report import SETTLE  # noqa: E402
from partisan_amd.sim import Simulator, default_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--ttl", type=int, default=8)
    a = ap.parse_args()
    sched = W.doubling_join(a.nodes, a.seed)
    with Simulator(default_config(n_nodes=a.nodes, seed=a.seed)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + SETTLE)
        pairs = Q.seeded_pairs(a.nodes, a.seed)
        m = sim.relay_reach([p[0] for p in pairs], [p[1] for p in pairs], a.ttl)
    print(json.dumps({"nodes": a.nodes, "ttl": a.ttl, "lanes": os.environ.get("PSIM_RELAY_LANES", "8"),
                      "levels_max": m["levels_max"], "peak_sum": int(m["peak"].sum()), "relays": int(m["relays"].sum())}))


if __name__ == "__main__":
    main()
