"""HyParView against X-BOT by latency, side by side: both handles run the same
doubling bootstrap (workloads.doubling_join(N, seed)) and step to the same
round (`--rounds` past the bootstrap's last join; X-BOT optimizes every
`--xbot-period` rounds), then latency_metrics() and graph_metrics() from the
same 64 seeded sources give the link costs, the hop paths and the cheapest
paths by latency of each.  With `--broadcasts B`, B broadcasts from `--root`
follow, each stepped until it has finished, and the tree half of
latency_metrics() gives the tree's mean latency depth and its stretch over the
overlay's cheapest paths.  Output: the Markdown table, and with `--json PATH`
the same numbers as JSON.

    python -m partisan_amd.latency_report --nodes N [--seed S] [--rounds R] [--xbot-period P]
                                          [--broadcasts B] [--root R] [--json PATH] [--out FILE]
"""
import argparse
import json
import time

from . import workloads as W
from .sim import Simulator, default_config
from .tree_report import complete_broadcast

ROUNDS = 60
PERIOD = 10
KINDS = (("hyparview", dict()), ("xbot", dict(manager=2)))


def columns(m, g):
    """the report's numbers from a latency_metrics() and a graph_metrics() dict
    of the same handle and sources"""
    return {
        "n_up": m["n_up"], "links": m["links"],
        "link_cost_mean": m["link_cost_sum"] / m["links"] if m["links"] else 0.0,
        "link_cost_worst_mean": m["worst_sum"] / m["link_nodes"] if m["link_nodes"] else 0.0,
        "link_cost_best_mean": m["best_sum"] / m["link_nodes"] if m["link_nodes"] else 0.0,
        "sources": m["sources_live"],
        "hops_mean": g["dist_sum"] / g["pairs_reached"] if g["pairs_reached"] else 0.0, "hops_max": g["ecc_max"],
        "bfs_levels": g["levels"],
        "latency_mean": m["lat_sum_all"] / m["pairs_reached"] if m["pairs_reached"] else 0.0,
        "latency_max": m["lat_max"], "pairs_unreached": m["pairs_unreached"], "sweeps": m["sweeps"],
    }


def tree_columns(m):
    """... from the tree half of a latency_metrics() dict"""
    r, b = m["tree_reached"], m["both_reached"]
    return {
        "tree_links": m["tree_links"],
        "tree_link_cost_mean": m["tree_link_cost_sum"] / m["tree_links"] if m["tree_links"] else 0.0,
        "tree_reached": r, "tree_latency_mean": m["tree_lat_sum"] / r if r else 0.0,
        "tree_latency_max": m["tree_lat_max"], "tree_sweeps": m["tree_sweeps"],
        "tree_stretch": m["tree_lat_sum_both"] / m["overlay_lat_sum_both"] if b and m["overlay_lat_sum_both"] else 0.0,
        "tree_slower": m["slower"], "tree_faster": m["faster"],
    }


def _run(cfg, sched, until, broadcasts, root):
    with Simulator(cfg) as sim:
        sim.run_schedule(sched, until)
        t0 = time.time()
        m = sim.latency_metrics(seed=cfg.seed)
        t1 = time.time()
        g = sim.graph_metrics(seed=cfg.seed)
        t2 = time.time()
        out = {"round": int(sim.round), **columns(m, g), "latency_call_s": round(t1 - t0, 4),
               "graph_call_s": round(t2 - t1, 4)}
        if broadcasts:
            for k in range(1, broadcasts + 1):
                complete_broadcast(sim, root, k)
            out.update(tree_columns(sim.latency_metrics([], tree_root=root)))
            out["tree_round"] = int(sim.round)
    return out


def build(n, seed=31, rounds=ROUNDS, xbot_period=PERIOD, broadcasts=0, root=0, device=-1):
    sched = W.doubling_join(n, seed)
    until = sched[-1][0] + 1 + rounds
    rep = {"nodes": n, "seed": seed, "rounds": rounds, "xbot_period": xbot_period, "broadcasts": broadcasts,
           "root": root}
    for name, kw in KINDS:
        if kw:
            kw = dict(kw, xbot_period=xbot_period)
        rep[name] = _run(default_config(n_nodes=n, seed=seed, device=device, **kw), sched, until, broadcasts, root)
    return rep


ROWS = (
    ("live nodes", "n_up", "d"), ("links", "links", "d"),
    ("mean link cost", "link_cost_mean", ".2f"), ("mean worst link of a node", "link_cost_worst_mean", ".2f"),
    ("mean best link of a node", "link_cost_best_mean", ".2f"),
    ("mean hop path", "hops_mean", ".3f"), ("longest hop path", "hops_max", "d"),
    ("mean cheapest-path latency", "latency_mean", ".2f"), ("largest cheapest-path latency", "latency_max", "d"),
    ("pairs not reached", "pairs_unreached", "d"), ("sweeps", "sweeps", "d"),
)
TREE_ROWS = (
    ("tree links", "tree_links", "d"), ("mean tree link cost", "tree_link_cost_mean", ".2f"),
    ("nodes the tree reaches", "tree_reached", "d"), ("mean tree latency depth", "tree_latency_mean", ".2f"),
    ("largest tree latency depth", "tree_latency_max", "d"), ("tree stretch", "tree_stretch", ".4f"),
    ("nodes slower by tree", "tree_slower", "d"), ("nodes faster by tree", "tree_faster", "d"),
)


def markdown(rep):
    a, b = rep["hyparview"], rep["xbot"]
    out = [f"# HyParView and X-BOT by latency at {rep['nodes']} nodes (seed {rep['seed']}, round {a['round']}, "
           f"X-BOT period {rep['xbot_period']})", "",
           f"Cheapest paths and hop paths from the same {a['sources']} seeded sources; `ratio` is X-BOT over HyParView.",
           "", "| | HyParView | X-BOT | ratio |", "|---|---|---|---|"]
    rows = ROWS + (TREE_ROWS if rep["broadcasts"] else ())
    for label, key, fmt in rows:
        x, y = a[key], b[key]
        out.append(f"| {label} | {x:{fmt}} | {y:{fmt}} | {(y / x if x else 0.0):.4f} |")
    if rep["broadcasts"]:
        out += ["", f"Tree rows: after {rep['broadcasts']} broadcasts from root {rep['root']} (round {a['tree_round']}); "
                "the stretch is the tree latency over the overlay's cheapest-path latency, summed over the nodes "
                "reached by both."]
    return "\n".join(out) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=ROUNDS, help="rounds after the bootstrap's last join")
    ap.add_argument("--xbot-period", type=int, default=PERIOD)
    ap.add_argument("--broadcasts", type=int, default=0)
    ap.add_argument("--root", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the numbers to this file")
    ap.add_argument("--out", default=None, help="also write the Markdown table to this file")
    ap.add_argument("--device", type=int, default=-1)
    a = ap.parse_args(argv)
    rep = build(a.nodes, a.seed, a.rounds, a.xbot_period, a.broadcasts, a.root, a.device)
    md = markdown(rep)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
            f.write("\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(md)
    print(md)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
