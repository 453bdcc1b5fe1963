"""Who told a node what, and who did not: a HyParView + Plumtree handle runs
the doubling bootstrap (workloads.doubling_join(N, seed)) plus 10 settle
rounds, arms a message trace on the nodes given (psim_trace_watch, both
directions, every type), broadcasts once from root R and steps until the
broadcast has finished.  Output: each watched node's timeline, one line per
record -- round, direction, peer, type, ttl, arguments (Plumtree: message id,
hop, root identity) -- and per node who delivered the tracked broadcast to it
first, and which of its active in-neighbours never sent it a BROADCAST or an
IHAVE of it.

    python -m partisan_amd.trace_report --nodes N --watch I[,J...] [--root R] [--seed S]
"""
import argparse

import numpy as np

from . import _abi
from . import workloads as W
from .sim import Simulator, default_config
from .tree_report import SETTLE, complete_broadcast

BROADCAST, IHAVE = 9, 11
MSG_ID = 1
CHUNK = 1 << 16


def in_neighbours(sim, watch):
    """{w: sorted live nodes whose active view holds w}, read CHUNK nodes at a time"""
    out = {w: [] for w in watch}
    for lo in range(0, sim.n, CHUNK):
        v = sim.nodes(lo, min(CHUNK, sim.n - lo))
        used = np.arange(v["act"].shape[1])[None, :] < v["act_n"][:, None]
        for w in watch:
            rows = np.nonzero(v["up"].astype(bool) & ((v["act"] == w) & used).any(1))[0] + lo
            out[w] += [int(i) for i in rows if int(i) != w]
    return out


def build(n, watch, root=0, seed=31, device=-1, capacity=1 << 20):
    sched = W.doubling_join(n, seed)
    with Simulator(default_config(n_nodes=n, seed=seed, device=device)) as sim:
        sim.run_schedule(sched, sched[-1][0] + 1 + SETTLE)
        sim.trace_watch(watch, capacity=capacity)
        first = int(sim.round)
        complete_broadcast(sim, root, MSG_ID)
        recs, rounds, lost = sim.trace_read()
        have, rnd, hop = sim.delivery()
        nbrs = in_neighbours(sim, watch)
    return {"nodes": n, "root": root, "seed": seed, "watch": list(watch), "first_round": first, "recs": recs,
            "rounds": rounds, "lost": lost, "in_neighbours": nbrs,
            "delivery": {w: (int(have[w]), int(rnd[w]), int(hop[w])) for w in watch}}


def timeline(rep, w):
    """the lines of node w: records to it ("<-") and by it ("->"), in trace order"""
    recs, rounds = rep["recs"], rep["rounds"]
    out = []
    for k in np.nonzero((recs[:, 0] == w) | (recs[:, 1] == w))[0]:
        r = recs[k]
        t = int(r[2]) & 0xFF
        name = _abi.MSG_TYPES[t] if t < len(_abi.MSG_TYPES) and _abi.MSG_TYPES[t] else str(t)
        arrow, peer = ("<-", int(r[1])) if int(r[0]) == w else ("->", int(r[0]))
        args = " ".join(f"{int(x):#x}" if int(x) & _abi.PSIM_MAP_BIT else str(int(x)) for x in r[4:8])
        out.append(f"  round {int(rounds[k]):4d} {arrow} {peer:8d}  {name:<18} ttl {(int(r[2]) >> 8) & 0xFF:3d}  {args}")
    return out


def answer(rep, w):
    """(first deliverer or None, its round, in-neighbours that sent w neither a
    BROADCAST nor an IHAVE of the tracked message)"""
    recs, rounds = rep["recs"], rep["rounds"]
    t = recs[:, 2] & 0xFF
    to_w = (recs[:, 0] == w) & (recs[:, 4] == MSG_ID) & ((t == BROADCAST) | (t == IHAVE))
    told = set(int(x) for x in recs[to_w, 1])
    b = np.nonzero(to_w & (t == BROADCAST))[0]
    first = (int(recs[b[0], 1]), int(rounds[b[0]])) if len(b) else (None, None)
    return first[0], first[1], [p for p in rep["in_neighbours"][w] if p not in told]


def text(rep):
    out = [f"Message trace of {len(rep['watch'])} nodes at {rep['nodes']} nodes (seed {rep['seed']}): broadcast "
           f"{MSG_ID} from root {rep['root']}, armed from round {rep['first_round']}, {len(rep['recs'])} records"
           f" ({rep['lost']} lost)", ""]
    for w in rep["watch"]:
        out.append(f"node {w}:")
        out += timeline(rep, w)
        who, when, silent = answer(rep, w)
        have, rnd, hop = rep["delivery"][w]
        if w == rep["root"]:
            out.append(f"  => node {w} is the root")
        elif who is None:
            out.append(f"  => no BROADCAST reached node {w} (delivered: {have})")
        else:
            # (a record sent in round r is handled in round r + 1)
            out.append(f"  => first BROADCAST from node {who}, sent in round {when}; delivered in round {rnd} at hop {hop}")
        out.append(f"  => active in-neighbours {rep['in_neighbours'][w]}; never sent it a BROADCAST or IHAVE: {silent}")
        out.append("")
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nodes", type=int, required=True)
    ap.add_argument("--watch", required=True, help="comma-separated node ids")
    ap.add_argument("--root", type=int, default=0)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--device", type=int, default=-1)
    a = ap.parse_args(argv)
    watch = sorted(set(int(x) for x in a.watch.split(",")))
    print(text(build(a.nodes, watch, a.root, a.seed, a.device)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
