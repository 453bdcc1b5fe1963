"""Scenarios that drive the lite kernel (k_lite_quarter: four nodes a wave,
the passive view two entries a lane) through the places where its layout
matters, shared by tests/test_lite_quarter_scenarios.py (the oracle alone:
each scenario still reaches what it is there for) and
tests/test_gpu_lite_quarter.py (GPU against oracle).

F   full passive views at the slot boundaries: max_passive_size 1 (slot 0 of
    lane 0 alone), 15 and 17 (an odd count: the last entry in slot 0; one
    past the half cap), 30 with one-element shuffles
F16 a 16-entry view with four-element passive samples
F30 the defaults: 30 entries, every merge of a full view evicts
D   deep inboxes: SHUFFLE / SHUFFLE_REPLY records past the first 16 and the
    first 32 of a node's inbox (k_lite_quarter reads the inbox 16 records at
    a time, k_lite_half 32)
"""
import numpy as np

import _scenarios as S
from partisan_amd import workloads as W
from partisan_amd.sim import default_config

MSG_SHUFFLE, MSG_SHUFFLE_REPLY = 7, 8

# name -> (n, seed, rounds, max_passive_size, config)
F_CASES = {
    "F-m1": (1021, 7, 120, 1, dict(shuffle_period=2, max_passive_size=1)),
    "F-m15": (1021, 7, 120, 15, dict(shuffle_period=2, max_passive_size=15)),
    "F-m17": (1021, 7, 120, 17, dict(shuffle_period=2, max_passive_size=17)),
    "F-m30-k1": (1021, 7, 120, 30, dict(shuffle_period=2, max_passive_size=30, k_active=1, k_passive=1)),
    "F16": (1023, 5, 120, 16, dict(max_passive_size=16, k_passive=4)),
    "F30": (2048, 3, 150, 30, dict()),
}


def run_f(make, name):
    n, seed, rounds, _, cfg = F_CASES[name]
    return S.doubling(make, n, seed, rounds, **cfg)


def full_share(sim, name):
    """share of nodes whose passive view holds max_passive_size entries"""
    return float((sim.nodes()["pas_n"] == F_CASES[name][3]).mean())


# D: every node shuffles every round with a long walk, and from round
# D_BCAST_FROM on four roots broadcast every round
# (on the oracle: a largest inbox of 141 records, 260 k SHUFFLE /
# SHUFFLE_REPLY records at position >= 16, 153 k at >= 32, no overflow, in
# under a second)
D_N, D_SEED, D_ROUNDS, D_BCAST_FROM = 1024, 3, 60, 30
D_ROOTS = (0, 256, 512, 768)


def run_d(make, each_round=None):
    """`each_round(sim, r)` runs before round r's step (the oracle test reads
    the inbox there)"""
    sim = make(default_config(n_nodes=D_N, seed=D_SEED, shuffle_period=1, arwl=12))
    state = {"k": 0}

    def hook(r):
        if r >= D_BCAST_FROM:
            for root in D_ROOTS:
                sim.broadcast(root, state["k"] % 0x10000)
                state["k"] += 1
        if each_round is not None:
            each_round(sim, r)
    st = sim.run_schedule(W.doubling_join(D_N, D_SEED), D_ROUNDS, extra=hook)
    return sim, st


def inbox_depths(inbox, position=16):
    """(largest inbox, SHUFFLE / SHUFFLE_REPLY records at `position` or later
    in their node's inbox) of an Oracle.inbox() array"""
    if len(inbox) == 0:
        return 0, 0
    dst = inbox[:, 0]
    order = np.argsort(dst, kind="stable")
    d = dst[order]
    start = np.r_[0, np.nonzero(d[1:] != d[:-1])[0] + 1]
    sizes = np.diff(np.r_[start, len(d)])
    pos = np.arange(len(d)) - np.repeat(start, sizes)
    typ = inbox[order, 3] & 0xFF
    deep = (pos >= position) & ((typ == MSG_SHUFFLE) | (typ == MSG_SHUFFLE_REPLY))
    return int(sizes.max()), int(deep.sum())
