"""What a transitive unicast -- forward_message with {broadcast, true} and
{transitive, true} under the HyParView manager -- reaches and what it pays:
the overlay of overlay_report, and 64 seeded (source, target) pairs sent with
each ttl of TTLS, one relay_reach() call a ttl.  One JSON file
and one Markdown table with the census line and a row per ttl: the share of
the pairs delivered, the mean first hop of those, the messages per unicast
sum(relays + delivered) / pairs, and the refused and expired shares of the
copies, refused / (relays + refused) and expired / relays.

    python -m partisan_amd.relay_report --nodes N --seed S --out DIR [--settle R] [--device D]
"""
import argparse
import json
import os
import time

import numpy as np

from . import workloads as W
from .overlay_report import SETTLE
from .sim import Simulator, default_config

TTLS = (1, 2, 3, 5, 8, 12, 16)
PAIRS = 64


def seeded_pairs(n, seed, k=PAIRS):
    """k seeded (source, target) pairs, source != target (the bootstrap leaves
    every node up; a pair naming a dead node would be skipped by the call)"""
    rng = np.random.Generator(np.random.PCG64([seed, 0x72]))
    out = []
    while len(out) < k:
        s, d = (int(x) for x in rng.integers(0, n, size=2))
        if s != d:
            out.append((s, d))
    return out


def row(m, ttl):
    """the table's row of one ttl from a relay_reach() dict"""
    live = int(m["cases_live"])
    got = int(np.count_nonzero(m["delivered"]))
    t = {x: int(m[x].sum()) for x in ("delivered", "first_hop", "hop_sum", "relays", "refused", "expired", "restarts",
                                      "in_flight")}
    return {
        "ttl": ttl, "cases": live, "direct": bin(m["direct_mask"]).count("1"), "pairs_delivered": got, **t,
        "truncated": bin(m["truncated_mask"]).count("1"), "levels_max": int(m["levels_max"]), "peak_max": int(m["peak"].max()),
        "delivered_share": got / live if live else 0.0,
        "first_hop_mean": t["first_hop"] / got if got else 0.0,
        "messages_per_unicast": (t["relays"] + t["delivered"]) / live if live else 0.0,
        "refused_share": t["refused"] / (t["relays"] + t["refused"]) if t["relays"] + t["refused"] else 0.0,
        "expired_share": t["expired"] / t["relays"] if t["relays"] else 0.0,
    }


def build(n, seed, settle=SETTLE, device=-1):
    sched = W.doubling_join(n, seed)
    until = sched[-1][0] + 1 + settle
    rep = {"nodes": n, "seed": seed, "settle_rounds": settle, "round": until, "ttls": list(TTLS)}
    with Simulator(default_config(n_nodes=n, seed=seed, device=device)) as sim:
        sim.run_schedule(sched, until)
        pairs = seeded_pairs(n, seed)
        src, dst = [p[0] for p in pairs], [p[1] for p in pairs]
        rows, call_s, m = [], [], None
        for ttl in TTLS:
            t0 = time.time()
            m = sim.relay_reach(src, dst, ttl)
            call_s.append(round(time.time() - t0, 3))
            rows.append(row(m, ttl))
    rep.update({"pairs": [list(p) for p in pairs], "rows": rows, "call_s": call_s,
                "census": {k: int(m[k]) for k in ("n_up", "out_entries", "out_usable", "out_nonmember", "members_down")},
                "out_degree": {str(k): int(v) for k, v in enumerate(m["out_degree"]) if v}})
    return rep


def markdown(rep):
    c = rep["census"]
    out = [f"# Transitive unicast at {rep['nodes']} nodes (seed {rep['seed']}, round {rep['round']})", "",
           f"{len(rep['pairs'])} seeded pairs of nodes; a pair whose source holds a connection to its target is sent",
           "directly, every other as the relay_message flood down the common out-links, which nothing deduplicates.",
           "`delivered`: pairs with at least one copy at the target.  `first hop`: sends on the shortest delivering walk.",
           "`messages`: relays and deliveries per unicast.  `refused`: sends to an out entry without a connection, of",
           "all sends tried.  `expired`: copies dropped at ttl 0, of the relays.", "",
           f"Census: {c['n_up']} live nodes, {c['out_entries']} out entries, {c['out_usable']} usable, "
           f"{c['out_nonmember']} naming a non-member, {c['members_down']} members without a connection.", "",
           "| ttl | delivered | first hop | messages | refused | expired | truncated |", "|---|---|---|---|---|---|---|"]
    for r in rep["rows"]:
        out.append(f"| {r['ttl']} | {r['delivered_share']:.4f} | {r['first_hop_mean']:.3f} | {r['messages_per_unicast']:.1f} "
                   f"| {r['refused_share']:.4f} | {r['expired_share']:.4f} | {r['truncated']} |")
    out.append("")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--out", default=".")
    ap.add_argument("--settle", type=int, default=SETTLE, help="rounds after the bootstrap's last join")
    ap.add_argument("--device", type=int, default=-1)
    a = ap.parse_args(argv)
    rep = build(a.nodes, a.seed, a.settle, a.device)
    os.makedirs(a.out, exist_ok=True)
    stem = os.path.join(a.out, f"report_n{a.nodes}")
    with open(stem + ".json", "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(stem + ".md", "w") as f:
        f.write(markdown(rep))
    print(json.dumps({"json": stem + ".json", "markdown": stem + ".md",
                      "delivered_share": [round(r["delivered_share"], 4) for r in rep["rows"]]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
