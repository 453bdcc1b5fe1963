"""k_relay's lanes run the SHUFFLE relays of a lite node's inbox that come
before its first terminal SHUFFLE or SHUFFLE_REPLY, and hand the lite kernel
the rest of the inbox and the count of records they emitted (PSIM_RELAY_LEAD,
RoundArgs::relay_lead).  The GPU must reproduce the oracle bit for bit --
every round's stats and digest, and the final node rows -- with the knob on
and off, on the half and the wave-per-node lite kernels, with the phase's
kernels launched one by one, and on the rank path.

The scenarios are tests/_relay_lead_cases.py's.  The knobs are read once per
process, so every (knob set, scenario group) runs in a child process
(tests/_relay_lead_run.py); the oracle runs each scenario once, here, and the
children compare against its saved results.

So that the tests cannot pass with the path dead, test_reach compares the
kernels' counts (kernel_counts after every single-round step) of the default
child with those of the PSIM_RELAY_LEAD=0 child, round by round: the results
being identical, the records that moved are k_relay's rise in deliveries,
which must equal the lite kernel's fall.
  steady           records moved, in both sizes
  churn_partition  during the partition more deliveries moved than emissions:
                   a leading relay whose send failed (the lane ran more relays
                   than it emitted records; with two active members or more a
                   relay always has an eligible member, so nothing else
                   separates the two counts)
  deep_star        on the oracle's inboxes (the GPU's are the same): lite
                   nodes with more than 32 records, which stay whole, in
                   rounds in which records of other nodes moved"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _relay_lead_cases as R
from _oracle import Oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = R.GROUPS

KNOBS = {
    "default": {},
    "lead0": {"PSIM_RELAY_LEAD": "0"},
    "half": {"PSIM_LITE_HALF": "1"},
    "wave": {"PSIM_LITE_WAVE": "1"},
    "fused0": {"PSIM_PHASE_FUSED": "0"},
    "loopback3": {"PSIM_KNOB_PATH": "loopback3"},
}
_OURS = ("PSIM_RELAY_LEAD", "PSIM_LITE_HALF", "PSIM_LITE_WAVE", "PSIM_PHASE_FUSED", "PSIM_KNOB_PATH")

deep_rounds = {}     # deep_star on the oracle: round -> lite-like nodes with more than 32 records


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """group -> .npz of the oracle's stats and nodes of its scenarios (each
    computed once, on first use)"""
    d = tmp_path_factory.mktemp("relay_lead_ref")

    def shapes(sim, r):
        if r >= R.STAR_BCAST_FROM:
            deep_rounds[r] = R.inbox_shapes(sim.inbox(), sim.nodes()["act_n"])["deep"]

    @functools.lru_cache(maxsize=None)
    def ref(group):
        out = {}
        for name, run in GROUPS[group]:
            sim, st = run(Oracle, each_round=shapes) if name == "deep_star" else run(Oracle)
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
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_relay_lead_run.py"), group, ref], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_relay_lead_keeps_parity(knobs, group, refs):
    _child(knobs, group, refs(group))


def _moved(group, name, refs):
    """round -> (deliveries, emissions) that k_relay took over from the lite
    kernel: the default child's counts less the PSIM_RELAY_LEAD=0 child's
    (the children are test_relay_lead_keeps_parity's, run once)"""
    on = _child("default", group, refs(group))[name]
    off = _child("lead0", group, refs(group))[name]
    assert len(on) == len(off) > 0
    out = {}
    for a, b in zip(on, off):
        assert a[0] == b[0]
        dd, de = a[1] - b[1], a[3] - b[3]
        assert dd == b[2] - a[2] and de == b[4] - a[4], (name, a, b)
        assert dd >= de >= 0, (name, a, b)
        out[a[0]] = (dd, de)
    return out


@pytest.mark.parametrize("name", ["steady1024", "steady4096"])
def test_reach_steady(name, refs):
    m = _moved("steady", name, refs)
    rounds = [r for r, (dd, _) in m.items() if dd > 0]
    print(name, "rounds with moved records:", len(rounds), "records:", sum(dd for dd, _ in m.values()))
    assert len(rounds) > 0, "k_relay ran no lite node's leading relays"


def test_reach_partition(refs):
    m = _moved("churn_partition", "churn_partition", refs)
    failed = sum(dd - de for r, (dd, de) in m.items() if R.PART_ON <= r < R.PART_OFF)
    print("churn_partition: leading relays whose send failed during the partition:", failed,
          "over the run:", sum(dd - de for dd, de in m.values()))
    assert failed > 0, "no leading relay whose send failed"


def test_reach_deep(refs):
    m = _moved("edges", "deep_star", refs)
    both = [r for r, k in deep_rounds.items() if k > 0 and m[r][0] > 0]
    print("deep_star: lite nodes past 32 records:", sum(deep_rounds.values()), "rounds with those and moved records:",
          len(both))
    assert both, "no round with a lite node past 32 records beside moved records"
