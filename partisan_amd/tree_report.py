"""How far Plumtree's eager graph of one root is from a tree, broadcast after
broadcast: a HyParView handle runs the doubling bootstrap
(workloads.doubling_join(N, seed)) plus 10 settle rounds, then K broadcasts
from root R, each stepped until it has finished; tree_metrics(R) goes into one
table row before the first broadcast (every node answers from common_eagers)
and one after each.  Columns: eager / lazy / both links, the nodes only a
graft reaches, mean and max depth, the stretch over the overlay, and the
payload redundancy of the next broadcast over frozen sets.  Output: the
Markdown table and one JSON line.

    python -m partisan_amd.tree_report --nodes N --root R --broadcasts K [--seed S] [--out FILE]
"""
import argparse
import json

from . import workloads as W
from .sim import Simulator, default_config

SETTLE = 10
CHUNK = 8


def complete_broadcast(sim, root, msg_id, chunk=CHUNK, max_chunks=64):
    """broadcast msg_id from root and step until it has finished: `chunk`
    rounds at a time until a chunk delivers it to no further node (that
    chunk lets the last PRUNE, IHAVE and GRAFT exchanges end).  Returns
    (rounds stepped, live nodes holding it)."""
    sim.broadcast(root, msg_id)
    rounds, last = 0, -1
    for _ in range(max_chunks):
        sim.step(chunk)
        rounds += chunk
        d = sim.histograms()["delivered"]
        if d == last:
            break
        last = d
    return rounds, last


def row(m):
    """the table's columns from a tree_metrics() dict"""
    r, b = m["reached"], m["both_reached"]
    return {
        "n_up": m["n_up"], "slot_nodes": m["slot_nodes"],
        "eager_links": m["eager_links"], "lazy_links": m["lazy_links"], "both_links": m["both_links"],
        "eager_both_forms": m["eager_both_forms"], "unreached": m["unreached"],
        "depth_mean": m["depth_sum"] / r if r else 0.0, "depth_max": m["depth_max"],
        "stretch": m["depth_sum_both"] / m["dist_sum_both"] if b and m["dist_sum_both"] else 0.0,
        "redundancy": m["links_from_reached"] / r - 1 if r else 0.0,
    }


def build(n, root, broadcasts, seed=31, device=-1):
    sched = W.doubling_join(n, seed)
    rows = []
    with Simulator(default_config(n_nodes=n, seed=seed, device=device)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + SETTLE)
        rows.append({"broadcast": 0, "round": int(sim.round), "rounds": 0, "delivered": 0,
                     **row(sim.tree_metrics(root))})
        for k in range(1, broadcasts + 1):
            rounds, delivered = complete_broadcast(sim, root, k)
            rows.append({"broadcast": k, "round": int(sim.round), "rounds": rounds, "delivered": int(delivered),
                         **row(sim.tree_metrics(root))})
    return {"nodes": n, "root": root, "seed": seed, "settle_rounds": SETTLE, "rows": rows}


def markdown(rep):
    out = [f"# Broadcast tree of root {rep['root']} at {rep['nodes']} nodes (seed {rep['seed']})", "",
           "Row 0: before the first broadcast, every node answers from common_eagers. `both`: lazy links whose",
           "peer is still an eager link (the atom / map identity forms). `unreached`: live nodes only a graft",
           "reaches. `stretch`: tree depth over overlay distance, summed over the nodes reached in both.",
           "`redundancy`: payload copies per reached node of the next broadcast over frozen sets, minus one.", "",
           "| broadcast | round | nodes with a slot | eager links | lazy links | both | unreached | mean depth "
           "| max depth | stretch | redundancy |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rep["rows"]:
        out.append(f"| {r['broadcast']} | {r['round']} | {r['slot_nodes']} | {r['eager_links']} | {r['lazy_links']} "
                   f"| {r['both_links']} | {r['unreached']} | {r['depth_mean']:.3f} | {r['depth_max']} "
                   f"| {r['stretch']:.4f} | {r['redundancy']:.4f} |")
    return "\n".join(out) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--root", type=int, default=0)
    ap.add_argument("--broadcasts", type=int, default=5)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--out", default=None, help="also write the Markdown table to this file")
    ap.add_argument("--device", type=int, default=-1)
    a = ap.parse_args(argv)
    rep = build(a.nodes, a.root, a.broadcasts, a.seed, a.device)
    md = markdown(rep)
    if a.out:
        with open(a.out, "w") as f:
            f.write(md)
    print(md)
    print(json.dumps(rep, sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
