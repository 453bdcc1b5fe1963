"""Scenario groups of tests/test_gpu_relay_lead.py, shared by the parent (the
oracle's run of each, once) and its child processes (the GPU's, per knob set):
group -> [(name, run(make, each_round=None) -> (sim, stats))].

k_relay's lanes run the SHUFFLE relays of a lite node's inbox that come before
its first terminal SHUFFLE or SHUFFLE_REPLY (RoundArgs::relay_lead).  What each
scenario is there for:

steady      doubling bootstrap, then 120 rounds with a broadcast every 10: lite
            nodes whose inbox has Plumtree records before the first terminal,
            and lite nodes in k_ptl's late part
multistep   the same at n = 4096 with several rounds a step call: the batch
            path, rounds prepared inside the route
churn_partition
            crash rounds, and a half/half partition: leading relays whose send
            fails, so the lane emitted fewer records than it ran
ramp        a join ramp's first rounds, shuffles every other round
small_views the ramp with max_active_size 2: nodes with one active member,
            where a SHUFFLE with TTL left ends the walk, and relays with one
            eligible member
deep_star   every node joins node 0 in one round, then shuffles every round
            with long walks and four roots broadcasting: lite nodes with
            inboxes past 32 records (left whole to the lite kernel) beside
            ones with leading relays
"""
import numpy as np

import _scenarios as S
from partisan_amd import workloads as W
from partisan_amd.sim import default_config

MSG_SHUFFLE, MSG_SHUFFLE_REPLY, MSG_PT_BROADCAST, MSG_XBOT = 7, 8, 9, 16

STEADY_ROUNDS = 120


def _ramp_rounds(n):
    return len(W.doubling_join(n, 0))


def steady(make, n, seed, each_round=None):
    sim = make(default_config(n_nodes=n, seed=seed))
    bc = S._bcast_every(sim, 10, 20)

    def hook(r):
        bc(r)
        if each_round is not None:
            each_round(sim, r)
    return sim, sim.run_schedule(W.doubling_join(n, seed), _ramp_rounds(n) + STEADY_ROUNDS, extra=hook)


def multistep(make, n=4096, seed=9, each_round=None):
    """the bootstrap a round at a time, then a broadcast and step(k) for k =
    3, 7, 10, 10, ...: 120 rounds"""
    sim = make(default_config(n_nodes=n, seed=seed))
    st = [sim.run_schedule(W.doubling_join(n, seed), _ramp_rounds(n))]
    left, i = STEADY_ROUNDS, 0
    for k in [3, 7] + [10] * 11:
        sim.broadcast(0, i)
        st.append(sim.step(min(k, left)))
        left -= k
        i += 1
    return sim, np.concatenate(st)


PART_ON, PART_OFF = 90, 100


def churn_partition(make, each_round=None):
    sim = make(default_config(n_nodes=2048, seed=5))
    n, seed = 2048, 5
    churn = {r: (v, c) for r, v, c in W.churn_schedule(n, seed, 0.2, 40, 40)}
    part = W.half_partition(n)
    bc = S._bcast_every(sim, 10, 30)

    def hook(r):
        if r in churn:
            v, c = churn[r]
            sim.crash(v)
            sim.join(v, c)
        if r == PART_ON:
            sim.set_partition(part)
        if r == PART_OFF:
            sim.clear_partition()
        bc(r)
        if each_round is not None:
            each_round(sim, r)
    return sim, sim.run_schedule(W.doubling_join(n, seed), 140, extra=hook)


def ramp(make, each_round=None):
    n, seed = 2048, 3
    sim = make(default_config(n_nodes=n, seed=seed, shuffle_period=2))

    def hook(r):
        if each_round is not None:
            each_round(sim, r)
    return sim, sim.run_schedule(W.doubling_join(n, seed), 30, extra=hook)


def small_views(make, each_round=None):
    n, seed = 1024, 3
    sim = make(default_config(n_nodes=n, seed=seed, shuffle_period=1, max_active_size=2, min_active_size=1))

    def hook(r):
        if each_round is not None:
            each_round(sim, r)
    return sim, sim.run_schedule(W.doubling_join(n, seed), 40, extra=hook)


STAR_N, STAR_ROOTS, STAR_BCAST_FROM = 1024, (0, 256, 512, 768), 25


def deep_star(make, each_round=None):
    sim = make(default_config(n_nodes=STAR_N, seed=3, shuffle_period=1, arwl=12))
    state = {"k": 0}

    def hook(r):
        if r >= STAR_BCAST_FROM:
            for root in STAR_ROOTS:
                sim.broadcast(root, state["k"] % 0x10000)
                state["k"] += 1
        if each_round is not None:
            each_round(sim, r)
    return sim, sim.run_schedule(W.star_join(STAR_N), 50, extra=hook)


GROUPS = {
    "steady": [("steady1024", lambda make, **kw: steady(make, 1024, 7, **kw)),
               ("steady4096", lambda make, **kw: steady(make, 4096, 9, **kw))],
    "multistep": [("multistep", multistep)],
    "churn_partition": [("churn_partition", churn_partition)],
    "edges": [("ramp", ramp), ("small_views", small_views), ("deep_star", deep_star)],
}


def inbox_shapes(inbox, act_n):
    """Of an Oracle.inbox() array (the records about to be delivered, a node's
    in delivery order) and the nodes' active-view sizes before the round: the
    nodes whose HyParView records are all SHUFFLEs and SHUFFLE_REPLYs with at
    least one that is no relay -- what k_relay files as lite unless something
    outside the inbox makes the node heavy -- counted as
      lead       with a relay before the first such record, at most 32 records
      lead_pt    ... and a Plumtree record before that relay's successor
      deep       with more than 32 records
      one_active with one active member and a SHUFFLE with TTL left"""
    out = {"lead": 0, "lead_pt": 0, "deep": 0, "one_active": 0}
    if len(inbox) == 0:
        return out
    dst = inbox[:, 0]
    order = np.argsort(dst, kind="stable")
    d = dst[order]
    start = np.r_[0, np.nonzero(d[1:] != d[:-1])[0] + 1]
    end = np.r_[start[1:], len(d)]
    tt = inbox[order, 3]
    typ, ttl = tt & 0xFF, (tt >> 8) & 0xFF
    for s, e in zip(start, end):
        node = int(d[s])
        t, l = typ[s:e], ttl[s:e]
        hv = (t < MSG_PT_BROADCAST) | (t >= MSG_XBOT)
        if not hv.any() or not np.isin(t[hv], (MSG_SHUFFLE, MSG_SHUFFLE_REPLY)).all():
            continue
        relay = hv & (t == MSG_SHUFFLE) & (l > 0) & (act_n[node] > 1)
        term = hv & ~relay
        if not term.any():
            continue
        first = int(np.argmax(term))
        if e - s > 32:
            out["deep"] += 1
        elif relay[:first].any():
            out["lead"] += 1
            out["lead_pt"] += bool((~hv[:first]).any())
        if act_n[node] == 1 and ((t == MSG_SHUFFLE) & (l > 0)).any():
            out["one_active"] += 1
    return out
