"""The redo of a batch round that k_desc stopped (run_batch, run_batch_ranked:
the round's outbox bound passed the outbox capacity, abort code 1) must
reproduce the oracle bit for bit -- also when the stopped round is the
batch's first, whose events the stopped attempt already applied: the redo
(run_round with events_applied) must still wake the quiet nodes a heal
reconnects, rebuild nothing twice and run the round-end halves of the events.

PSIM_TEST_DESC_CAP=<slots>[@<rank>] (psim_engine.hip, batch_desc_cap) caps the
capacity k_desc checks against, so the stop comes at will: with 1 slot every
batch stops at its first round -- every event round of every scenario goes
through the redo -- with MID slots only the rounds whose bound passes it, some
of them in the middle of a batch.  The hook is read once per process, so every
(knob set, scenario) runs in a child process (tests/_batch_redo_run.py); the
oracle runs each scenario once, here.

So that a green run cannot have missed the path, the parent reads from the
child's stderr which rounds stopped (the engine's `outbox grows past its
capacity` line) and where each batch began (PSIM_TRACE_BATCH=1), and asserts
the reach conditions below.

MID.  The totals (the outbox bound + 1) the cap1 child printed for
heal_after_quiet (n = 512, seed 3) on an MI355X, per round:
  60-67 (the quiet step(7) and step(1)): 9447 9122 8863 8646 8399 7898 7765 7455
  68-75 (the heal's step(8)):  10655 24866 44584 122165 240431 159722 75491 33451
  76-83 (partition + broadcast): 27138 9744 1842 1197 383 220 219 243
  84-90 (crash wave):            616 329 345 321 613 1146 505
  91-98 (heal, rejoin, broadcast): 1152 2525 3795 4738 7025 6482 7403 7286
  99-104 (crash wave):           3792 1890 1786 1164 721 747
  105-112 (revive + broadcast):  522 459 543 1108 2565 4470 5947 4945
The bound of the rounds before the heal is loose (623 messages against a
bound of 7454 in round 67: the nodes still working bound their lazy ticks by
their whole tables), so the band between them and the heal round (9447 ..
10655) holds no value that also stops a batch past its first round.  MID =
4000 lies between the settled rounds of the second leg (78-93 and 99-109:
219 .. 3795) and every event-driven peak (68-77: 9744 and more; 94-98:
4738 .. 7403; 110-112: 4470 .. 5947): the heal round stops its batch of 8 at
its first round, rounds 94 and 110 stop theirs (from 91 and 105) at the
fourth and sixth, and the batches from 78, 84 and 99 run to their ends."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from _batch_redo_run import CASES
from _oracle import Oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

MID = 4000

KNOBS = {
    "cap1": {"PSIM_TEST_DESC_CAP": "1"},
    "mid": {"PSIM_TEST_DESC_CAP": str(MID)},
    "loopback2_cap1": {"PSIM_TEST_DESC_CAP": "1", "PSIM_KNOB_PATH": "loopback2"},
    # only rank 1's outbox is short: ranks 0 and 2 redo the round from their owner partition
    "loopback3_cap1_at1": {"PSIM_TEST_DESC_CAP": "1@1", "PSIM_KNOB_PATH": "loopback3"},
}
CAP1 = ("cap1", "loopback2_cap1", "loopback3_cap1_at1")

# the event rounds that must be among the stopped ones under a 1-slot cap:
# the heal (68) and the first round of every later multi-round step of
# heal_after_quiet; the first round of every multi-round step of multistep;
# the partition's set and clear rounds of the scenarios stepped one by one
MUST_STOP = {
    "heal_after_quiet": [68, 76, 84, 91, 99, 105],
    "multistep": [20, 60, 90, 110, 122],
    "out_tail": [40, 80],
    "churn_partition": [90, 100],
    "xbot_churn": [90],
}

STOP_RE = re.compile(r"psim: round (\d+): outbox grows past its capacity \((\d+) -> (\d+) slots\)")
BATCH_RE = re.compile(r"psim: (?:rank (\d+): )?batch of (\d+) from round (\d+):")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """scenario -> .npz of the oracle's stats and nodes (computed once, on first use)"""
    d = tmp_path_factory.mktemp("batch_redo_ref")

    @functools.lru_cache(maxsize=None)
    def ref(name):
        sim, st = CASES[name](Oracle)
        path = os.path.join(d, name + ".npz")
        np.savez(path, stats=st, nodes=sim.nodes())
        sim.close()
        return path
    return ref


_done, _died = {}, []


def _child(knobs, name, ref):
    """the child's JSON and what its stderr tells, each (knob set, scenario)
    run once -- a failed one too: its failure is raised again"""
    if (knobs, name) not in _done:
        try:
            _done[knobs, name] = _run_child(knobs, name, ref)
        except (AssertionError, subprocess.TimeoutExpired) as e:
            if isinstance(e, subprocess.TimeoutExpired):
                _died.append(f"{knobs} {name}: time limit")
            _done[knobs, name] = e
    if isinstance(_done[knobs, name], BaseException):
        raise AssertionError(str(_done[knobs, name]))
    return _done[knobs, name]


def _run_child(knobs, name, ref):
    drop = ("PSIM_TEST_DESC_CAP", "PSIM_KNOB_PATH", "PSIM_NO_RESERVE", "PSIM_NO_BATCH", "PSIM_NO_RANK_BATCH",
            "PSIM_TEST_FAIL_ROUND", "PSIM_TRACE_RELAY")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(KNOBS[knobs], PSIM_TRACE_BATCH="1")
    # (a child that a signal ended may have left the GPU in trouble: no more are started)
    assert not _died, f"an earlier child died ({_died[0]}): no further child is started"
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_batch_redo_run.py"), name, ref], env=env,
                       capture_output=True, text=True, timeout=240)
    stops = [(int(m[1]), int(m[3])) for m in STOP_RE.finditer(r.stderr)]
    print(knobs, name, "stopped rounds and their totals:", sorted(set(stops)))
    if r.returncode < 0 or r.returncode in (134, 139):
        _died.append(f"{knobs} {name}: exit status {r.returncode}")
    if r.returncode != 0:          # (the child's own words, without the engine's trace lines)
        err = [ln for ln in r.stderr.splitlines() if not ln.startswith("psim: ")]
        raise AssertionError(f"child exit status {r.returncode}: " + "\n".join(r.stdout.splitlines()[-5:] + err[-12:]))
    assert "identical" in r.stdout
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out["stops"] = sorted({s[0] for s in stops})
    # (rank 0's batches, or the local path's: every rank runs the same ones)
    out["batches"] = sorted({(int(m[3]), int(m[2])) for m in BATCH_RE.finditer(r.stderr) if m[1] in (None, "0")})
    return out


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_redo_keeps_parity(knobs, name, refs):
    out = _child(knobs, name, refs(name))
    if knobs in CAP1:
        missed = [r for r in MUST_STOP[name] if r not in out["stops"]]
        assert not missed, f"event rounds {missed} were not stopped at k_desc: stopped {out['stops']}"



def test_heal_round_had_quiet_nodes(refs):
    """(the children are test_redo_keeps_parity's, run once) quiet nodes
    existed when the heal came: the single-round step of round 67 counted
    their ticks in k_node_prep without running them; and no outstanding table
    overflowed (the oracle's own count, which the children equal)"""
    for knobs in ("cap1", "mid"):
        out = _child(knobs, "heal_after_quiet", refs("heal_after_quiet"))
        assert out["prep"]["67"] > 0, out["prep"]
        assert out["overflow"] == 0


def test_mid_stops_inside_batches(refs):
    """with MID slots heal_after_quiet has a stop at a round that is not its
    batch's first and a batch that ran to its end"""
    out = _child("mid", "heal_after_quiet", refs("heal_after_quiet"))
    firsts = {r0 for r0, _ in out["batches"]}
    inside = [r for r in out["stops"] if r not in firsts]
    whole = [(r0, k) for r0, k in out["batches"] if k > 1 and not any(r0 <= r < r0 + k for r in out["stops"])]
    print("stops", out["stops"], "inside a batch", inside, "whole batches", whole)
    assert 68 in out["stops"]
    assert inside, "no stop past a batch's first round"
    assert whole, "no multi-round batch ran to its end"
