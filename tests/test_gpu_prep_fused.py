"""A batch's route prepares the next round (PSIM_PREP_FUSED, psim_engine.hip:
k_bucket_route with a RoutePrep, run_batch): the packed bound | work words,
ocnt = 0, the ranges' sums for k_desc and the prepare's stats rows come from
the route blocks, no k_node_prep launch.  Every case must reproduce the oracle
bit for bit -- every round's stats and digest, the final node rows, the overlay
histograms -- with the knob at 1 and at 0.

Sizes, for the places the block code can go wrong: 1500 (one partial bucket),
2049 (a one-node last bucket; k_node_prep's own range of 1280 nodes would not
nest in the 2048-node buckets), 5000 (three buckets, the last partial, five
ranges), 65536 (32 buckets, 64 ranges).  At the three small sizes every
scenario of tests/_prep_fused_run.py runs; at 65536 `multistep` and the star
hotspot (the oracle takes 12 s for multistep there and would take a minute
for all five; what the other scenarios add is per-node -- the saturated
nibble, X-BOT's closing connections, the quiet ticks -- and the small sizes
cover it on full and partial buckets alike).

Fallbacks, each with the knob at 1 and at 0: PSIM_TEST_DESC_CAP with 1 slot and
with MID slots (test_gpu_batch_redo's, which stops heal_after_quiet at n = 512
inside batches: the redo of a round the route had prepared); PSIM_RCAP_INIT=16
(the route's regrow and the exact reroute); the star at 65536 (node 0's bucket
of the fused route overflows: the returning blocks must leave ocnt alone);
PSIM_ROUTE_FUSED=0 (the path must be off); PSIM_ROUTE_LIDX=0.

The knobs are read once per process, so every (knob set, case list) runs in a
child process, stepped in calls of several rounds (tests/_prep_fused_run.py);
the oracle runs each case once, here.  So that a green run cannot have missed
the path, the parent reads the children's PSIM_TRACE_BATCH lines: rounds were
prepared in the route in every knob-1 child where batches form (never with
PSIM_ROUTE_FUSED=0), none with the knob at 0; a batch whose first round has
crashes prepares two rounds fewer than it has (multistep), and the
churn_partition children have a batch with both kinds of round."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _oracle import Oracle
from _prep_fused_run import CASES, parse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SCENARIOS = ("multistep", "churn_partition", "heal_after_quiet", "out_tail", "xbot_churn")
MID = 4000      # (tests/test_gpu_batch_redo.py: between heal_after_quiet's settled rounds and its peaks at n = 512)

# name -> (cases, environment)
SETS = {
    "n1500": (",".join(f"{s}:1500" for s in SCENARIOS), {}),
    "n2049": (",".join(f"{s}:2049" for s in SCENARIOS), {}),
    "n5000": (",".join(f"{s}:5000" for s in SCENARIOS), {}),
    "n65536": ("multistep:65536", {}),
    "cap1": ("multistep:1500,heal_after_quiet:512", {"PSIM_TEST_DESC_CAP": "1"}),
    "mid": ("heal_after_quiet:512,multistep:1500", {"PSIM_TEST_DESC_CAP": str(MID)}),
    "rcap16": ("multistep:1500,churn_partition:2049", {"PSIM_RCAP_INIT": "16"}),
    "star": ("star:65536", {}),
    "route_fused0": ("multistep:1500", {"PSIM_ROUTE_FUSED": "0"}),
    "lidx0": ("multistep:5000,out_tail:2049", {"PSIM_ROUTE_LIDX": "0"}),
}
OURS = ("PSIM_PREP_FUSED", "PSIM_TEST_DESC_CAP", "PSIM_RCAP_INIT", "PSIM_ROUTE_FUSED", "PSIM_ROUTE_LIDX",
        "PSIM_ROUTE_WSHIFT", "PSIM_NO_BATCH", "PSIM_NO_RESERVE", "PSIM_TEST_FAIL_ROUND", "PSIM_TRACE_RELAY",
        "PSIM_PHASE_TIMERS", "PSIM_LIB")

BATCH_RE = re.compile(r"psim: batch of (\d+) from round (\d+): .*?, (\d+) prepared in the route")
STOP_RE = re.compile(r"psim: round (\d+): outbox grows past its capacity")


@functools.lru_cache(maxsize=None)
def _oracle_case(name, n):
    sim = CASES[name](Oracle, n)
    out = {"stats": sim[1], "nodes": sim[0].nodes()}
    for k, v in sim[0].histograms().items():
        out["hist." + k] = np.asarray(v)
    sim[0].close()
    return out


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """case list -> .npz of the oracle's stats, nodes and histograms (each case computed once)"""
    d = tmp_path_factory.mktemp("prep_fused_ref")

    @functools.lru_cache(maxsize=None)
    def ref(cases):
        out = {}
        for name, n in parse(cases):
            for k, v in _oracle_case(name, n).items():
                out[f"{name}:{n}.{k}"] = v
        path = os.path.join(d, "ref%d.npz" % (abs(hash(cases)) % 10 ** 8))
        np.savez(path, **out)
        return path
    return ref


_done, _died = {}, []


def _child(sname, knob, refs):
    """the child's batches (first round, rounds, rounds prepared in the route)
    and the rounds k_desc stopped; each (set, knob) run once"""
    if (sname, knob) not in _done:
        assert not _died, f"an earlier child died ({_died[0]}): no further child is started"
        cases, extra = SETS[sname]
        env = {k: v for k, v in os.environ.items() if k not in OURS}
        env.update(extra, PSIM_PREP_FUSED=knob, PSIM_TRACE_BATCH="1")
        try:
            r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_prep_fused_run.py"), cases, refs(cases)],
                               env=env, capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            _died.append(f"{sname} {knob}: time limit")
            raise
        if r.returncode < 0 or r.returncode in (134, 139):
            _died.append(f"{sname} {knob}: exit status {r.returncode}")
        err = [ln for ln in r.stderr.splitlines() if not ln.startswith("psim: ")]
        assert r.returncode == 0, f"child exit status {r.returncode}: " + "\n".join(r.stdout.splitlines()[-6:] + err[-12:])
        assert "all identical" in r.stdout
        _done[sname, knob] = {"batches": [(int(m[2]), int(m[1]), int(m[3])) for m in BATCH_RE.finditer(r.stderr)],
                              "stops": sorted({int(m[1]) for m in STOP_RE.finditer(r.stderr)})}
    return _done[sname, knob]


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("sname", list(SETS))
def test_prep_fused_keeps_parity(sname, knob, refs):
    out = _child(sname, knob, refs)
    multi = [b for b in out["batches"] if b[1] > 1]
    prepared = sum(b[2] for b in out["batches"])
    print(sname, knob, "batches", len(out["batches"]), "of several rounds", len(multi), "rounds prepared", prepared,
          "stops", out["stops"])
    assert multi, "no batch of several rounds formed"
    assert all(p <= k - 1 for _, k, p in out["batches"]), "a batch's first round is never prepared in the route"
    if knob == "0" or sname == "route_fused0":
        assert prepared == 0, "rounds prepared in the route with the path off"
    else:
        assert prepared > 0, "no round was prepared in the route"


def test_crash_round_successor_takes_the_kernel(refs):
    """multistep's crash wave starts a call of 20 rounds (from round 90): its
    second round follows a round-end half (k_uncrash) and launches k_node_prep,
    the others are prepared in the route; the call from round 60, a broadcast
    and no crash, prepares all but its first round"""
    out = _child("n1500", "1", refs)
    # (the set's first case is multistep: its batches, up to where the round numbers start again)
    b = out["batches"]
    first = b[: next((i for i in range(1, len(b)) if b[i][0] < b[i - 1][0]), len(b))]
    by_r0 = {r0: (k, p) for r0, k, p in first}
    print(by_r0)
    assert 90 in by_r0 and 60 in by_r0, sorted(by_r0)
    k, p = by_r0[90]
    assert k >= 3 and p == k - 2, (k, p)
    k, p = by_r0[60]
    assert k >= 2 and p == k - 1, (k, p)


def test_churn_partition_has_both_kinds(refs):
    for sname in ("n1500", "n2049", "n5000"):
        out = _child(sname, "1", refs)
        both = [b for b in out["batches"] if 0 < b[2] < b[1]]
        assert both, "no batch with a round from k_node_prep and a round from the route"


def test_redo_after_a_route_side_prepare(refs):
    """with MID slots k_desc stops heal_after_quiet (n = 512) past a batch's
    first round: a round the route had prepared is redone from k_node_prep"""
    out = _child("mid", "1", refs)
    inside = [r for r in out["stops"] if any(r0 < r < r0 + k and p >= r - r0 for r0, k, p in out["batches"])]
    print("stops", out["stops"], "inside a batch, in a prepared round", inside)
    assert inside, "no stop at a round the route had prepared"
    assert _child("cap1", "1", refs)["stops"], "no stop with a 1-slot cap"


def test_star_overflows_a_bucket_inside_a_batch(refs):
    """the star's batches stop at the route (no k_desc stop is reported): a
    batch ends before its last round, the next begins where it stopped"""
    out = _child("star", "1", refs)
    b = out["batches"]
    cut = [(r0, k) for (r0, k, _), (n0, _, _) in zip(b, b[1:]) if r0 < n0 < r0 + k and n0 - 1 not in out["stops"]
           and n0 not in out["stops"]]
    print("batches cut short at the route:", cut)
    assert cut, "no batch stopped at the route"
