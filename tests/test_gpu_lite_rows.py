"""The lite kernel fetches the next node's rows (header words, active and
passive rows, partition byte, connection bits, outbox bound) and the
descriptor of the node after it into LDS by LDS-DMA, issued before the body
of the node it runs (psim_lite.h, PSIM_LITE_ROWS_LDS).  The GPU must still
reproduce the oracle bit for bit -- every round's stats and digest, and the
final node rows -- on the row kernel inside k_hv_phase (the default), on
k_lite_half, with the phase's kernels launched one by one (k_lite_quarter on
its own), with k_relay's leading relays off (longer inbox runs in the lite
kernel), and on the rank path.

The scenarios are tests/_lite_rows_cases.py's: the smallest lists at which a
wave's DMA can go wrong (lanes of groups without a node, of groups that left
the loop, a single node), inboxes long enough for ordinary loads while a DMA
is in flight, failed sends, and a shard whose rows start at a nonzero id.  The
knobs are read once per process, so every (knob set, group) runs in a child
process (tests/_lite_rows_run.py); the oracle runs each scenario once, here.

So that the tests cannot pass with the path dead, test_reach_tiny reads the
default child's kernel_counts after every round: the lite kernel ran nodes in
every tiny overlay, and from n = 5 up in some round a count that is no
multiple of 4 and in some round a single node.  On the oracle's inboxes (the
GPU's are the same) it checks that the long-inbox cases the lists are there
for occur: lite-like nodes with more than 16 records from n = 5 up."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _lite_rows_cases as L
from _oracle import Oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = L.GROUPS

KNOBS = {
    "default": {},
    "half": {"PSIM_LITE_HALF": "1"},
    "fused0": {"PSIM_PHASE_FUSED": "0"},
    "lead0": {"PSIM_RELAY_LEAD": "0"},
    "loopback3": {"PSIM_KNOB_PATH": "loopback3"},
}
_OURS = ("PSIM_RELAY_LEAD", "PSIM_LITE_HALF", "PSIM_LITE_WAVE", "PSIM_PHASE_FUSED", "PSIM_KNOB_PATH",
         "PSIM_LIB")
# (the rank path runs one shard a rank: the two-shard run is not its case)
CASES = [(k, g) for k in KNOBS for g in GROUPS if not (k == "loopback3" and g == "shards2")]

MSG_SHUFFLE, MSG_SHUFFLE_REPLY, MSG_PT_BROADCAST, MSG_XBOT = 7, 8, 9, 16
long_inboxes = {}    # tiny scenario -> lite-like node-rounds with more than 16 records, on the oracle
lite_like = {}       # tiny scenario -> rounds with a lite-like node, on the oracle


def _lite_like(inbox, act_n):
    """of an Oracle.inbox() array and the active-view sizes before the round:
    (nodes whose HyParView records are all SHUFFLEs and SHUFFLE_REPLYs with at
    least one that is no relay -- lite unless k_relay has another reason to
    file the node as heavy --, those of them with more than 16 records)"""
    nodes = deep = 0
    if len(inbox) == 0:
        return 0, 0
    order = np.argsort(inbox[:, 0], kind="stable")
    d = inbox[order, 0]
    start = np.r_[0, np.nonzero(d[1:] != d[:-1])[0] + 1]
    end = np.r_[start[1:], len(d)]
    tt = inbox[order, 3]
    typ, ttl = tt & 0xFF, (tt >> 8) & 0xFF
    for s, e in zip(start, end):
        t, l = typ[s:e], ttl[s:e]
        hv = (t < MSG_PT_BROADCAST) | (t >= MSG_XBOT)
        if not hv.any() or not np.isin(t[hv], (MSG_SHUFFLE, MSG_SHUFFLE_REPLY)).all():
            continue
        relay = hv & (t == MSG_SHUFFLE) & (l > 0) & (act_n[int(d[s])] > 1)
        if not (hv & ~relay).any():
            continue
        nodes += 1
        deep += e - s > 16
    return nodes, deep


class Watched(Oracle):
    """the oracle, counting the lite-like inboxes of every round"""
    tally = None

    def step(self, n_rounds=1):
        if n_rounds == 1 and Watched.tally is not None:
            nodes, deep = _lite_like(self.inbox(), self.nodes()["act_n"])
            Watched.tally[0] += nodes > 0
            Watched.tally[1] += deep
        return super().step(n_rounds)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """group -> .npz of the oracle's stats and nodes of its scenarios (each
    computed once, on first use)"""
    d = tmp_path_factory.mktemp("lite_rows_ref")

    @functools.lru_cache(maxsize=None)
    def ref(group):
        out = {}
        for name, run in GROUPS[group]:
            Watched.tally = [0, 0] if group == "tiny" else None
            sim, st = run(lambda cfg, n_shards=1: Watched(cfg))
            if group == "tiny":
                lite_like[name], long_inboxes[name] = Watched.tally
            Watched.tally = None
            out[name + ".stats"], out[name + ".nodes"] = st, sim.nodes()
            sim.close()
        path = os.path.join(d, group + ".npz")
        np.savez(path, **out)
        return path
    return ref


@functools.lru_cache(maxsize=None)
def _child(knobs, group, ref):
    env = {k: v for k, v in os.environ.items() if k not in _OURS}
    env.update(KNOBS[knobs])
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_lite_rows_run.py"), group, ref], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("knobs,group", CASES)
def test_lite_rows_keep_parity(knobs, group, refs):
    _child(knobs, group, refs(group))


@pytest.mark.parametrize("n", L.TINY_SIZES)
def test_reach_tiny(n, refs):
    name = "tiny%d" % n
    rows = _child("default", "tiny", refs("tiny"))[name]
    assert len(rows) == L.TINY_ROUNDS
    nodes = [r[1] for r in rows]
    ran = [k for k in nodes if k > 0]
    print(name, "rounds with lite nodes:", len(ran), "of", len(rows), "counts", min(ran, default=0), "to",
          max(ran, default=0), "no multiple of 4 in", sum(k % 4 != 0 for k in ran), "single node in",
          sum(k == 1 for k in ran), "| oracle: rounds with a lite-like node", lite_like[name],
          "lite-like node-rounds past 16 records", long_inboxes[name])
    assert ran, "the lite kernel ran no node"
    if n >= 5:
        assert any(k % 4 != 0 for k in ran), "every lite list a multiple of 4: no group without a node"
        assert any(k == 1 for k in ran), "no lite list of a single node"
        assert long_inboxes[name] > 0, "no lite-like node with more than 16 records"
