"""How far a flood still gets when a share of all nodes fails at one instant,
before any healing: the HyParView and the SCAMP v2 overlay of overlay_report
(workloads.doubling_join(N, seed) plus `--settle` rounds, scamp_c 5), one
resilience() call each with 64 cases -- failed shares q/10 for q = 0..7 times 8
seeded live sources, slot 8q + k = (source k, salt k, threshold
floor(q 2^32 / 10)).  One JSON file and one Markdown table with a row per
share: mean survivors, reliability sum(reached) / sum(alive - 1), mean hops
sum(hop_sum) / sum(reached), largest ecc, and the shares of survivors with no
in-link and with no out-link.

    python -m partisan_amd.resilience_report --nodes N --seed S --out DIR [--settle R] [--device D]
"""
import argparse
import json
import os
import time

import numpy as np

from . import workloads as W
from .overlay_report import SETTLE
from .sim import Simulator, default_config

SHARES, PER_SHARE = 8, 8
FAIL_SEED = 0x72
SIDES = (("hyparview", "HyParView", {}), ("scamp_v2", "SCAMP v2 (c = 5)", dict(manager=1, strategy=2, scamp_c=5)))


def live_sources(sim, seed, k=PER_SHARE):
    """the first k live ids of 64 drawn from np.random.Generator(PCG64([seed,
    0x72])): the live mask of a call in which every other node fails"""
    rng = np.random.Generator(np.random.PCG64([seed, 0x72]))
    ids = rng.choice(sim.n, size=min(64, sim.n), replace=False).astype(np.uint32)
    mask = sim.resilience(ids, np.full(ids.size, 0xFFFFFFFF, np.uint32))["live_mask"]
    return [int(s) for j, s in enumerate(ids) if (mask >> j) & 1][:k]


def cases(sources):
    """(sources, thresholds, salts) of the 64 slots"""
    k = len(sources)
    src = np.tile(np.asarray(sources, np.uint32), SHARES)
    thr = np.repeat(np.array([(q << 32) // 10 for q in range(SHARES)], np.uint32), k)
    return src, thr, np.tile(np.arange(k, dtype=np.uint32), SHARES)


def rows(m, k=PER_SHARE):
    """the table's rows from a resilience() dict of cases(sources)"""
    out = []
    for q in range(SHARES):
        s = slice(q * k, (q + 1) * k)
        live = bin((m["live_mask"] >> (q * k)) & ((1 << k) - 1)).count("1")
        t = {f: int(m[f][s].sum()) for f in ("alive", "links_alive", "no_out", "no_in", "reached", "hop_sum")}
        others = t["alive"] - live
        out.append({
            "failed_share": q / 10, "cases": live, **t,
            "alive_mean": t["alive"] / live if live else 0.0,
            "reliability": t["reached"] / others if others else 0.0,
            "hops_mean": t["hop_sum"] / t["reached"] if t["reached"] else 0.0,
            "ecc_max": int(m["ecc"][s].max()) if k else 0,
            "no_in_share": t["no_in"] / t["alive"] if t["alive"] else 0.0,
            "no_out_share": t["no_out"] / t["alive"] if t["alive"] else 0.0,
        })
    return out


def _side(cfg, sched, until, seed):
    with Simulator(cfg) as sim:
        sim.run_schedule(sched, until)
        src = live_sources(sim, seed)
        t0 = time.time()
        m = sim.resilience(*cases(src), fail_seed=FAIL_SEED)
        call_s = round(time.time() - t0, 3)
        rounds = int(sim.round)
    return {"n_up": m["n_up"], "links": m["links"], "out_degree_mean": m["links"] / m["n_up"] if m["n_up"] else 0.0,
            "rounds": rounds, "sources": src, "levels": m["levels"], "truncated": m["truncated"], "call_s": call_s,
            "rows": rows(m, len(src))}


def build(n, seed, settle=SETTLE, device=-1):
    sched = W.doubling_join(n, seed)
    until = sched[-1][0] + 1 + settle
    rep = {"nodes": n, "seed": seed, "settle_rounds": settle, "round": until, "fail_seed": FAIL_SEED}
    for key, _, extra in SIDES:
        rep[key] = _side(default_config(n_nodes=n, seed=seed, device=device, **extra), sched, until, seed)
    return rep


def markdown(rep):
    out = [f"# Reach of a flood under mass failure at {rep['nodes']} nodes (seed {rep['seed']}, round {rep['round']})",
           "", "A share of all nodes fails at one instant; a flood starts at a survivor and runs over the links",
           "whose two ends survived, with no healing.  Each row: 8 sources, each with a failure set of its own.",
           "`reliability`: reached survivors over all other survivors.  `no in` / `no out`: survivors left",
           "without an in-link (no flood can reach them) / without an out-link.", ""]
    for key, title, _ in SIDES:
        x = rep[key]
        out += [f"## {title}: {x['n_up']} live nodes, {x['links']} links, mean out-degree "
                f"{x['out_degree_mean']:.3f}, {x['levels']} BFS levels", "",
                "| failed | mean survivors | reliability | mean hops | largest ecc | no in | no out |",
                "|---|---|---|---|---|---|---|"]
        for r in x["rows"]:
            out.append(f"| {r['failed_share']:.0%} | {r['alive_mean']:.1f} | {r['reliability']:.4f} "
                       f"| {r['hops_mean']:.3f} | {r['ecc_max']} | {r['no_in_share']:.4f} | {r['no_out_share']:.4f} |")
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
