"""The handler outcomes no other parity run enters (DESIGN.md section 6,
"What no parity run reaches"): each scenario of the registry's RARE table was
written for one branch outcome of the oracle -- tests/test_oracle_coverage.py
shows on the CPU that it takes it, and that no older run does -- and runs here
GPU == oracle, bit for bit: every round's stats and digest, and every node's
final state.  On one shard and on 3 virtual shards (full-membership handles
have one shard: psim_create refuses more), and the Plumtree ones under
PSIM_PTL_GRID=x1 as well, where k_pt alone runs the Plumtree phase (a child
process, tests/_rare_branch_run.py: the knob is read once per process).
The oracle's run of a scenario is computed once and left unchanged."""
import functools
import os
import subprocess
import sys

import pytest

import _parity_registry as P
import _scenarios as S
from _oracle import Oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu(shards):
    def make(cfg):
        from partisan_amd import Simulator
        cfg.n_shards = shards
        return Simulator(cfg)
    return make


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return P.RARE[name](Oracle)


def _is_full(name):
    return name.startswith("full_")


CASES = [(name, shards) for name in P.RARE for shards in (1, 3) if not (shards > 1 and _is_full(name))]


@pytest.mark.parametrize("name,shards", CASES, ids=[f"{n}-{s}" for n, s in CASES])
def test_rare_branch_parity(name, shards):
    os_, ost = _oracle(name)[:2]
    gs, gst = P.RARE[name](_gpu(shards))[:2]
    try:
        S.compare_stats(gst, ost)
        if P.RARE_KIND[name] == "pl":
            n = gs.cfg.n_nodes
            S.compare_strategy(gs, os_, full_bits=[0, 1, n // 2, n - 1] if _is_full(name) else None)
        else:
            S.compare_nodes(gs.nodes(), os_.nodes())
    finally:
        gs.close()


def test_the_scenarios_count_what_they_are_for():
    """the overflow kinds of the stats say on their own that the stale-slot
    and full-pool paths ran (OVF_PT), and pending_keep's view overflowed
    (OVF_STRATEGY): the figures the GPU is compared on above"""
    import _config_cases as CC
    for name, kind in (("retired_ids", CC.OVF_PT), ("set_pool_full", CC.OVF_PT), ("pending_keep", CC.OVF_STRATEGY)):
        assert int(_oracle(name)[1]["overflow_by"][:, kind].sum()) > 0, name


@pytest.mark.parametrize("name", sorted(P.RARE_PLUMTREE))
def test_rare_branch_parity_k_pt_fallback(name):
    env = dict(os.environ, PSIM_PTL_GRID="x1")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_rare_branch_run.py"), name], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout
