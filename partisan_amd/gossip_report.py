"""What gossip with a fanout reaches and what it pays, beside a flood, when a
share of all nodes fails at one instant, before any healing: the two overlays
and the 8 sources of resilience_report, one gossip_reach() call per failed
share in (0, 30 %, 50 %), each with 64 cases -- the fanouts FANOUTS (0: a
flood) times the 8 sources, slot 8 fi + k = (source k, threshold
floor(q 2^32 / 10), salt k, FANOUTS[fi]).  One JSON file and one Markdown table
with a row per share and fanout: reliability sum(reached) / sum(alive - 1),
mean hops sum(hop_sum) / sum(reached), largest ecc, copies per survivor
sum(sent) / sum(alive), the lost share sum(lost) / sum(sent) and the duplicates
per delivery sum(sent - lost - reached) / sum(reached).

    python -m partisan_amd.gossip_report --nodes N --seed S --out DIR [--settle R] [--device D]
"""
import argparse
import json
import os
import time

import numpy as np

from . import workloads as W
from .overlay_report import SETTLE
from .resilience_report import FAIL_SEED, SIDES, live_sources
from .sim import Simulator, default_config

SHARES = (0, 3, 5)                      # failed tenths
FANOUTS = (1, 2, 3, 4, 5, 6, 8, 0)


def cases(sources, q):
    """(sources, fanouts, thresholds, salts) of the 64 slots of failed share q / 10"""
    k = len(sources)
    src = np.tile(np.asarray(sources, np.uint32), len(FANOUTS))
    fan = np.repeat(np.array(FANOUTS, np.uint32), k)
    thr = np.full(src.size, (q << 32) // 10, np.uint32)
    return src, fan, thr, np.tile(np.arange(k, dtype=np.uint32), len(FANOUTS))


def rows(m, q, k):
    """the table's rows of share q / 10 from a gossip_reach() dict of cases(sources, q)"""
    out = []
    for fi, f in enumerate(FANOUTS):
        s = slice(fi * k, (fi + 1) * k)
        live = bin((m["live_mask"] >> (fi * k)) & ((1 << k) - 1)).count("1")
        t = {x: int(m[x][s].sum()) for x in ("alive", "reached", "hop_sum", "sent", "lost")}
        others, arrived = t["alive"] - live, t["sent"] - t["lost"]
        out.append({
            "failed_share": q / 10, "fanout": f, "cases": live, **t,
            "reliability": t["reached"] / others if others else 0.0,
            "hops_mean": t["hop_sum"] / t["reached"] if t["reached"] else 0.0,
            "ecc_max": int(m["ecc"][s].max()) if k else 0,
            "copies_per_survivor": t["sent"] / t["alive"] if t["alive"] else 0.0,
            "lost_share": t["lost"] / t["sent"] if t["sent"] else 0.0,
            "duplicates_per_delivery": (arrived - t["reached"]) / t["reached"] if t["reached"] else 0.0,
        })
    return out


def _side(cfg, sched, until, seed):
    with Simulator(cfg) as sim:
        sim.run_schedule(sched, until)
        src = live_sources(sim, seed)
        out, levels, call_s, m = [], [], [], None
        for q in SHARES:
            t0 = time.time()
            m = sim.gossip_reach(*cases(src, q), fail_seed=FAIL_SEED)
            call_s.append(round(time.time() - t0, 3))
            levels.append(m["levels"])
            out += rows(m, q, len(src))
        rounds = int(sim.round)
    return {"n_up": m["n_up"], "links": m["links"], "out_degree_mean": m["links"] / m["n_up"] if m["n_up"] else 0.0,
            "rounds": rounds, "sources": src, "levels": levels, "call_s": call_s, "rows": out}


def build(n, seed, settle=SETTLE, device=-1):
    sched = W.doubling_join(n, seed)
    until = sched[-1][0] + 1 + settle
    rep = {"nodes": n, "seed": seed, "settle_rounds": settle, "round": until, "fail_seed": FAIL_SEED,
           "shares": [q / 10 for q in SHARES], "fanouts": list(FANOUTS)}
    for key, _, extra in SIDES:
        rep[key] = _side(default_config(n_nodes=n, seed=seed, device=device, **extra), sched, until, seed)
    return rep


def markdown(rep):
    out = [f"# Gossip with a fanout under mass failure at {rep['nodes']} nodes (seed {rep['seed']}, round {rep['round']})",
           "", "A share of all nodes fails at one instant; a gossip starts at a survivor.  Every node reached pushes",
           "once, to `fanout` of its links chosen among all of them -- the failure is not yet detected, so a copy",
           "to a failed node is lost; fanout `all` is a flood.  Each row: 8 sources, each with a failure set of its",
           "own.  `reliability`: reached survivors over all other survivors.  `copies`: copies sent per survivor.",
           "`lost`: the share of them sent to failed nodes.  `dup`: copies that reach a node that has one, per delivery.",
           ""]
    for key, title, _ in SIDES:
        x = rep[key]
        out += [f"## {title}: {x['n_up']} live nodes, {x['links']} links, mean out-degree {x['out_degree_mean']:.3f}", "",
                "| failed | fanout | reliability | mean hops | largest ecc | copies | lost | dup |",
                "|---|---|---|---|---|---|---|---|"]
        for r in x["rows"]:
            out.append(f"| {r['failed_share']:.0%} | {r['fanout'] or 'all'} | {r['reliability']:.4f} | {r['hops_mean']:.3f} "
                       f"| {r['ecc_max']} | {r['copies_per_survivor']:.3f} | {r['lost_share']:.4f} "
                       f"| {r['duplicates_per_delivery']:.3f} |")
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
                      "reliability": {k: [round(r["reliability"], 4) for r in rep[k]["rows"]] for k, _, _ in SIDES}}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
