"""HyParView and SCAMP v2 overlays built the same way, side by side (SURVEY
8(d) config D): both handles run the same doubling bootstrap
(workloads.doubling_join(N, seed)) plus `--settle` rounds to the same round,
then the device statistics of each -- histograms() and
strategy_histograms() -- go into one JSON file and one Markdown table:
in-degree histograms, view fill, links and reciprocity, components, and from
graph_metrics() the clustering coefficient and the shortest paths from 64
seeded sources.

    python -m partisan_amd.overlay_report --nodes N --seed S [--out DIR]
"""
import argparse
import json
import os
import time

import numpy as np

from . import workloads as W
from .sim import Simulator, default_config

SETTLE = 10


def _trim(h):
    """a histogram as a list without its trailing zero bins"""
    h = [int(x) for x in h]
    while len(h) > 1 and h[-1] == 0:
        h.pop()
    return h


def _mean(h, n):
    """mean of a histogram's bins (a lower bound once the last bin is in use)"""
    return float(np.dot(np.arange(len(h)), h)) / n if n else 0.0


def _run(cfg, sched, until):
    t0 = time.time()
    with Simulator(cfg) as sim:
        st = sim.run_schedule(sched, until)
        t1 = time.time()
        h = sim.histograms() if cfg.manager == 0 else sim.strategy_histograms()
        t2 = time.time()
        g = sim.graph_metrics(seed=cfg.seed)
        t3 = time.time()
        rounds = int(sim.round)
    return h, g, {"rounds": rounds, "messages": int(st["emitted"].sum()), "overflow": int(st["overflow"].sum()),
                  "run_s": round(t1 - t0, 3), "stats_s": round(t2 - t1, 3), "graph_s": round(t3 - t2, 3)}


def _graph(g):
    """the report's keys from a graph_metrics() dict: the mean local
    clustering coefficient over all live nodes (a node with fewer than two
    neighbours counts 0), and the path lengths from the 64 seeded sources"""
    return {
        "clustering_mean": g["cl_sum_q32"] / 2.0 ** 32 / g["n_up"] if g["n_up"] else 0.0,
        "path_mean": g["dist_sum"] / g["pairs_reached"] if g["pairs_reached"] else 0.0,
        "path_max": g["ecc_max"], "pairs_unreached": g["pairs_unreached"],
        "path_sources": g["sources_live"], "path_levels": g["levels"],
    }


def build(n, seed, settle=SETTLE, device=-1):
    sched = W.doubling_join(n, seed)
    until = sched[-1][0] + 1 + settle
    hv, hv_g, hv_run = _run(default_config(n_nodes=n, seed=seed, device=device), sched, until)
    sc, sc_g, sc_run = _run(default_config(n_nodes=n, seed=seed, manager=1, strategy=2, scamp_c=5, device=device),
                            sched, until)
    up_h, up_s = hv["n_up"], sc["n_up"]
    hyparview = {
        "n_up": up_h, **hv_run,
        "in_degree": _trim(hv["active_in"]), "in_degree_mean": _mean(hv["active_in"], up_h),
        "view_fill": _trim(hv["active_out"]), "view_fill_mean": _mean(hv["active_out"], up_h),
        "passive_fill": _trim(hv["passive_fill"]), "passive_fill_mean": _mean(hv["passive_fill"], up_h),
        "links": hv["active_links"], "mutual_links": hv["symmetric_links"],
        "reciprocity": hv["symmetric_links"] / hv["active_links"] if hv["active_links"] else 0.0,
        "components": hv["components"], "largest_component": hv["largest_component"],
        **_graph(hv_g),
    }
    scamp = {
        "n_up": up_s, **sc_run,
        "in_degree": _trim(sc["in_degree"]), "in_degree_mean": sc["links"] / up_s if up_s else 0.0,
        "in_degree_max": sc["in_degree_max"],
        "view_fill": _trim(sc["out_degree"]), "view_fill_mean": _mean(sc["out_degree"], up_s),
        "raw_view_fill": _trim(sc["view_fill"]), "raw_view_mean": sc["view_sum"] / up_s if up_s else 0.0,
        "view_max": sc["view_max"],
        "in_view_fill": _trim(sc["in_fill"]), "in_view_mean": sc["in_sum"] / up_s if up_s else 0.0,
        "links": sc["links"], "mutual_links": sc["mutual_links"],
        "reciprocity": sc["mutual_links"] / sc["links"] if sc["links"] else 0.0,
        "dangling_links": sc["dangling_links"], "self_entries": sc["self_entries"],
        "duplicate_entries": sc["duplicate_entries"],
        "in_view_links": sc["in_view_links"], "in_view_confirmed": sc["in_view_confirmed"],
        "components": sc["components"], "largest_component": sc["largest_component"], "isolated": sc["isolated"],
        **_graph(sc_g),
    }
    return {"config": "D", "nodes": n, "seed": seed, "settle_rounds": settle, "round": until,
            "hyparview": hyparview, "scamp_v2": scamp}


def markdown(rep):
    a, b = rep["hyparview"], rep["scamp_v2"]
    rows = [
        ("live nodes", a["n_up"], b["n_up"]),
        ("round", a["rounds"], b["rounds"]),
        ("messages sent", a["messages"], b["messages"]),
        ("mean view size (distinct ids != self)", f"{a['view_fill_mean']:.3f}", f"{b['view_fill_mean']:.3f}"),
        ("mean in-degree", f"{a['in_degree_mean']:.3f}", f"{b['in_degree_mean']:.3f}"),
        ("fill of the second view (passive / in_view), mean", f"{a['passive_fill_mean']:.3f}",
         f"{b['in_view_mean']:.3f}"),
        ("links (live -> live)", a["links"], b["links"]),
        ("... with the reverse link", a["mutual_links"], b["mutual_links"]),
        ("reciprocity", f"{a['reciprocity']:.4f}", f"{b['reciprocity']:.4f}"),
        ("components", a["components"], b["components"]),
        ("largest component", a["largest_component"], b["largest_component"]),
        ("statistics call (s)", a["stats_s"], b["stats_s"]),
        ("clustering_mean (local clustering coefficient, mean over live nodes)", f"{a['clustering_mean']:.6f}",
         f"{b['clustering_mean']:.6f}"),
        (f"path_mean (shortest paths from {a['path_sources']} / {b['path_sources']} sources, reached pairs)",
         f"{a['path_mean']:.3f}", f"{b['path_mean']:.3f}"),
        ("path_max (longest shortest path seen; pairs not reached)", f"{a['path_max']} ({a['pairs_unreached']})",
         f"{b['path_max']} ({b['pairs_unreached']})"),
    ]
    out = [f"# HyParView and SCAMP v2 at {rep['nodes']} nodes (seed {rep['seed']}, round {rep['round']})", "",
           "| | HyParView | SCAMP v2 (c = 5) |", "|---|---|---|"]
    out += [f"| {k} | {x} | {y} |" for k, x, y in rows]
    out += ["", "## In-degree histogram (live nodes by in-degree; the last bin of 64 saturates)", "",
            "| in-degree | HyParView | SCAMP v2 |", "|---|---|---|"]
    ha, hb = a["in_degree"], b["in_degree"]
    for k in range(max(len(ha), len(hb))):
        x, y = (ha[k] if k < len(ha) else 0), (hb[k] if k < len(hb) else 0)
        if x or y:
            out.append(f"| {k} | {x} | {y} |")
    out += ["", "## View fill (live nodes by distinct ids != self in the active / partial view)", "",
            "| size | HyParView | SCAMP v2 |", "|---|---|---|"]
    ha, hb = a["view_fill"], b["view_fill"]
    for k in range(max(len(ha), len(hb))):
        x, y = (ha[k] if k < len(ha) else 0), (hb[k] if k < len(hb) else 0)
        if x or y:
            out.append(f"| {k} | {x} | {y} |")
    return "\n".join(out) + "\n"


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
    stem = os.path.join(a.out, f"d_compare_n{a.nodes}_s{a.seed}")
    with open(stem + ".json", "w") as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(stem + ".md", "w") as f:
        f.write(markdown(rep))
    print(json.dumps({"json": stem + ".json", "markdown": stem + ".md", "n_up": [rep["hyparview"]["n_up"],
                                                                               rep["scamp_v2"]["n_up"]]}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
