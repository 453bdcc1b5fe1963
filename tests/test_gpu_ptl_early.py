"""The early part of k_ptl's list -- the Plumtree phase of the nodes whose
HyParView phase k_relay itself finished, run as a fourth block range of
k_hv_phase beside the HyParView bodies (PSIM_PTL_EARLY, phase_consume) -- must
reproduce the oracle bit for bit, every round's stats and the final node
state: under every value of the knob, on the fallback paths (one k_ptl launch
over the four bins: PSIM_PHASE_FUSED 0 and 2, crash rounds), with other
sub-grid sizes (the block ranges and the stats-row offsets move; five k_ptl
blocks, far below the resident grid, so the range and the launch stride over
their lists) and on the rank path.  The knob's default is 0, where k_relay
files every node in the first two bins (one list, as before the split), so the
fallback, sub-grid and rank-path sets run with the default and with the knob
set (the four bins).

The scenarios (tests/_ptl_early_cases.py): doubling at n = 4096 with
broadcasts (Plumtree traffic beside due shuffles, terminals and joins),
churn_partition at n = 2048 (crash rounds serial, the rounds between
overlapped), multistep (the batch path) and xbot_churn (closing entries: nodes
that fall to k_pt from either part).

The knobs are read once per process, so every (knob set, scenario) runs in a
child process (tests/_ptl_early_run.py); the oracle runs each scenario once,
here, and the children compare against its saved results.

A lite, shuf or heavy node in an early bin would run its Plumtree phase before
its outbox count and draw counter are final: a sequence or digest mismatch --
provided such nodes exist in the rounds that overlap.  So the children count,
after every single-round step (psim_debug_kernel_counts with cap 32; a kernel
counts when its records-delivered count is above zero), and test_reach
asserts: for `doubling` (n = 4096, seed 9) a non-crash round in which the
early part, the late part (the k_ptl entry less the early one) and the lite
kernel all delivered records; for `churn_partition` (n = 2048, seed 5) a crash
round; for `xbot_churn` (n = 2048, seed 5) a round in which k_pt and the early
part both delivered.  The counts are those of the PSIM_PTL_EARLY=1 children:
the knob's default is 0 (the overlap measured slower),
where one k_ptl launch runs both parts and the early entry is zeros, so only
with the knob set do the counts say anything about the overlap.  Measured (an
MI355X): doubling 39 such rounds of 60, churn_partition 40 crash rounds,
xbot_churn 51 rounds with k_pt beside the early part."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _oracle import Oracle
from _ptl_early_cases import GROUPS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

KNOBS = {
    "default": {},
    "early0": {"PSIM_PTL_EARLY": "0"},
    "early1": {"PSIM_PTL_EARLY": "1"},
    "early2": {"PSIM_PTL_EARLY": "2"},
    "fused0": {"PSIM_PHASE_FUSED": "0"},
    "fused2": {"PSIM_PHASE_FUSED": "2"},
    "grids": {"PSIM_LITE_GRID": "x1", "PSIM_PTL_GRID": "5"},
    "loopback3": {"PSIM_KNOB_PATH": "loopback3"},
    # (the default of PSIM_PTL_EARLY is 0, and k_relay then files one list: the same sets with the list split)
    "fused0_early1": {"PSIM_PHASE_FUSED": "0", "PSIM_PTL_EARLY": "1"},
    "fused2_early1": {"PSIM_PHASE_FUSED": "2", "PSIM_PTL_EARLY": "1"},
    "grids_early1": {"PSIM_LITE_GRID": "x1", "PSIM_PTL_GRID": "5", "PSIM_PTL_EARLY": "1"},
    "grids_early2": {"PSIM_LITE_GRID": "x1", "PSIM_PTL_GRID": "5", "PSIM_PTL_EARLY": "2"},
    "loopback3_early1": {"PSIM_KNOB_PATH": "loopback3", "PSIM_PTL_EARLY": "1"},
}
OURS = ("PSIM_PTL_EARLY", "PSIM_PHASE_FUSED", "PSIM_LITE_GRID", "PSIM_PTL_GRID", "PSIM_KNOB_PATH")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """group -> .npz of the oracle's stats and nodes of its scenarios (each
    computed once, on first use)"""
    d = tmp_path_factory.mktemp("ptl_early_ref")

    @functools.lru_cache(maxsize=None)
    def ref(group):
        out = {}
        for name, run in GROUPS[group]:
            sim, st = run(Oracle)
            out[name + ".stats"], out[name + ".nodes"] = st, sim.nodes()
            sim.close()
        path = os.path.join(d, group + ".npz")
        np.savez(path, **out)
        return path
    return ref


@functools.lru_cache(maxsize=None)
def _child(knobs, group, ref):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(KNOBS[knobs])
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_ptl_early_run.py"), group, ref], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_ptl_early_keeps_parity(knobs, group, refs):
    _child(knobs, group, refs(group))


def test_reach(refs):
    """(the three children are test_ptl_early_keeps_parity's, run once)"""
    counts = _child("early1", "doubling", refs("doubling"))
    print("doubling:", counts)
    assert counts["overlap"] > 0, "no non-crash round in which the early part, the late part and the lite kernel all delivered"
    counts = _child("early1", "churn_partition", refs("churn_partition"))
    print("churn_partition:", counts)
    assert counts["crash"] > 0, "no crash round"
    counts = _child("early1", "xbot_churn", refs("xbot_churn"))
    print("xbot_churn:", counts)
    assert counts["pt_early"] > 0, "no round in which k_pt and the early part both delivered"
