"""k_hv_phase -- k_shuf's, k_consume's and k_lite_quarter's bodies in one
launch, each on its own range of blocks (PSIM_PHASE_FUSED, phase_consume) --
must reproduce the oracle bit for bit, every round's stats and the final node
state, under every value of the knob, with other sub-grid sizes (the block
ranges and the stats-row offsets move) and on the rank path.

The scenarios (tests/_phase_fused_cases.py): multistep (several rounds a step
call), churn_partition (crash rounds run the three kernels serially, the
rounds between fused, in one run), doubling at n = 4096 with broadcasts
(joins and promotions in k_consume beside due shuffle starts), xbot_churn
(k_consume's heaviest handlers), and the lite kernel's own F and D scenarios.

The knobs are read once per process, so every (knob set, scenario group) runs
in a child process (tests/_phase_fused_run.py); the oracle runs each scenario
once, here, and the children compare against its saved results.

So that the tests cannot pass without the three bodies ever having had work
at once, the children count (kernel_counts after every single-round step) the
non-crash rounds with nodes in k_shuf, the lite kernel and k_consume all
three, and the crash rounds: test_reach asserts the first for `doubling`
(n = 4096, seed 9) and the second for `churn_partition` (n = 2048, seed 5),
on the default knobs.  k_shuf's nodes are counted by k_relay, which lists
them; what shows that k_shuf ran nodes is its own row's emitted SHUFFLEs."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _oracle import Oracle
from _phase_fused_cases import GROUPS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

KNOBS = {
    "default": {},
    "fused0": {"PSIM_PHASE_FUSED": "0"},
    "fused2": {"PSIM_PHASE_FUSED": "2"},
    "fused3": {"PSIM_PHASE_FUSED": "3"},
    "grids": {"PSIM_LITE_GRID": "x1", "PSIM_CONSUME_GRID": "x2"},
    "loopback3": {"PSIM_KNOB_PATH": "loopback3"},
}


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """group -> .npz of the oracle's stats and nodes of its scenarios (each
    computed once, on first use)"""
    d = tmp_path_factory.mktemp("phase_fused_ref")

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
    env = {k: v for k, v in os.environ.items() if k != "PSIM_PHASE_FUSED"}
    env.update(KNOBS[knobs])
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_phase_fused_run.py"), group, ref], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_phase_fused_keeps_parity(knobs, group, refs):
    _child(knobs, group, refs(group))


def test_reach(refs):
    """(the two children are test_phase_fused_keeps_parity's, run once)"""
    counts = _child("default", "doubling", refs("doubling"))
    print("doubling:", counts)
    assert counts["reach"] > 0, "no non-crash round with nodes in k_shuf, the lite kernel and k_consume at once"
    counts = _child("default", "churn_partition", refs("churn_partition"))
    print("churn_partition:", counts)
    assert counts["crash"] > 0, "no crash round"
