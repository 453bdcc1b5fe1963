"""psim_get_strategy_histograms on the GPU: every field of the struct against
the numpy reference (tests/_strategy_stats.py) applied to the CPU oracle's
views of the same scenario -- the expected values never come from the engine.
One shard, virtual shards and loopback ranks; views of 128 ids, a crashed
tenth, a partition, SCAMP v1's set order, the full strategy's member sets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _scenarios as S
import _strategy_stats as R
from _oracle import Oracle
from partisan_amd import workloads as W
from partisan_amd.sim import SimError, _Driver, default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu(cfg):
    from partisan_amd import Simulator
    return Simulator(cfg)


def _vshards(g):
    def mk(cfg):
        from partisan_amd import Simulator
        c = type(cfg).from_buffer_copy(cfg)
        c.n_shards = g
        return Simulator(c)
    return mk


def _loop(world):
    def mk(cfg):
        from _loopback import LoopbackRanks
        return LoopbackRanks(cfg, world)
    return mk


def _stats(sim):
    """strategy_histograms() of a handle; of loopback ranks: one thread per
    rank (a collective), every rank the same answer"""
    if hasattr(sim, "ranks"):
        hs = sim._threads("strategy_histograms")
        for h in hs[1:]:
            assert all(np.array_equal(h[k], hs[0][k]) for k in h), "ranks disagree on the overlay statistics"
        return hs[0]
    return sim.strategy_histograms()


_REF = {}


def _want(key, run, strategy):
    """the reference over the oracle's views of a scenario, computed once"""
    if key not in _REF:
        o = run(Oracle)[0]
        _REF[key] = R.reference(o.strategy_nodes(), strategy)
        o.close()
    return _REF[key]


def _check(make, key, run, strategy):
    want = _want(key, run, strategy)
    g = run(make)[0]
    try:
        R.compare(_stats(g), want)
    finally:
        g.close()
    return want


def _crashed(n, rounds):
    return lambda make: S.pl_doubling(make, n=n, seed=13, rounds=rounds, strategy=2, crash_at=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(4)], ids=["gpu", "4-shards"])
def test_v2_crashed_tenth(make):
    w = _check(make, "crash33", _crashed(2048, 33), 2)
    assert (w["n_up"], w["dangling_links"], w["components"], w["largest_component"]) == (1844, 309, 115, 1466)


def test_v2_full_row_and_saturating_bins():
    w = _check(_gpu, "crash50", _crashed(2048, 50), 2)
    assert w["view_max"] == 128 and w["in_degree_max"] == 216 and w["view_fill"][63] == 1
    assert (w["components"], w["largest_component"]) == (1, 2048)


@pytest.mark.parametrize("make", [_vshards(3), _loop(2)], ids=["3-shards", "loopback-2"])
def test_v2_uneven_shards(make):
    w = _check(make, "crash203", _crashed(203, 33), 2)
    assert (w["n_up"], w["components"], w["dangling_links"]) == (183, 15, 30)


@pytest.mark.parametrize("make", [_gpu, _loop(2)], ids=["gpu", "loopback-2"])
def test_v1_large_view(make):
    w = _check(make, "v1", lambda mk: S.pl_v1_large_view(mk, leave_from=10**9, leave_to=0, rounds=40), 1)
    assert w["view_max"] > 100 and w["in_degree_max"] == 179 and not w["in_fill"].any()


def test_v2_partition():
    w = _check(_gpu, "part", lambda mk: S.pl_doubling(mk, n=2048, seed=13, rounds=40, strategy=2, part_at=12), 2)
    assert (w["components"], w["largest_component"], w["isolated"]) == (1025, 1024, 1024)


def _full_ref(o):
    return R.reference(o.strategy_nodes(), 0, [o.member_bits(i) for i in range(o.n)])


def test_full_membership_agreement():
    """the full strategy (fanout 5, 200 nodes): a round before convergence
    (0 < agreeing < n_up on the oracle), one after, and one after leave/1
    removals, where the remove rows count"""
    n, seed = 200, 13
    cfg = dict(n_nodes=n, seed=seed, manager=1, strategy=0, fanout=5)
    o, g = Oracle(default_config(**cfg)), _gpu(default_config(**cfg))
    sched = W.doubling_join(n, seed)
    seen = []
    for until in (16, 30):
        o.run_schedule(sched, until)
        g.run_schedule(sched, until)
        want = _full_ref(o)
        R.compare(g.strategy_histograms(), want)
        seen.append((want["agreeing"], want["n_up"]))
    assert 0 < seen[0][0] < seen[0][1] and seen[1][0] == seen[1][1] == n
    o.close(); g.close()
    o, _, actors, targets = S.pl_leave_remote(Oracle, n=n, seed=seed, rounds=50, strategy=0, leave_at=40, k=4, fanout=5)
    g, _ = S.pl_leave_fixed(_gpu, n=n, seed=seed, rounds=50, strategy=0, leave_at=40, actors=actors,
                            targets=targets, fanout=5)
    want = _full_ref(o)
    assert want["members_min"] < n and 0 < want["agreeing"]
    got = g.strategy_histograms()
    R.compare(got, want)
    for k in R.HISTS:
        assert not got[k].any()
    o.close(); g.close()


def test_error_paths_and_empty_handle():
    from partisan_amd import _abi
    hv = _gpu(default_config(n_nodes=64, seed=1))
    with pytest.raises(SimError, match="unsupported"):
        hv.strategy_histograms()
    assert hv._extra["get_strategy_histograms"](hv._h, None) == -1        # PSIM_EINVAL
    assert hv._extra["get_strategy_histograms"](None, _abi.PsimStrategyHistograms()) == -1
    hv.close()
    for strategy in (0, 1, 2):
        s = _gpu(default_config(n_nodes=300, seed=1, manager=1, strategy=strategy))
        for rounds in (0, 2):                # no node ever started: before and after empty rounds
            if rounds:
                s.step(rounds)
            h = s.strategy_histograms()
            assert all(not np.any(v) for v in h.values()), h
        s.close()


class _CallAt:
    """a handle that takes its statistics once, before the step of round `at`"""
    run_schedule = _Driver.run_schedule

    def __init__(self, sim, at):
        self._sim, self._at, self.seen = sim, at, []

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def step(self, k=1):
        if self._sim.round == self._at and not self.seen:
            self.seen.append(self._sim.strategy_histograms())
        return self._sim.step(k)


def test_read_only():
    """a call in the middle of a run changes no later round"""
    o, ost = _crashed(2048, 33)(Oracle)
    box = []

    def make(cfg):
        box.append(_CallAt(_gpu(cfg), 20))
        return box[0]
    g, gst = _crashed(2048, 33)(make)
    assert g.seen and g.seen[0]["n_up"] == 2048
    S.compare_stats(gst, ost)
    S.compare_strategy(g, o)
    R.compare(g.strategy_histograms(), _want("crash33", _crashed(2048, 33), 2))
    g.close(); o.close()


def test_overlay_report(tmp_path):
    r = subprocess.run([sys.executable, "-m", "partisan_amd.overlay_report", "--nodes", str(1 << 12), "--seed", "31",
                        "--out", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    stem = f"d_compare_n{1 << 12}_s31"
    rep = json.loads((tmp_path / (stem + ".json")).read_text())
    md = (tmp_path / (stem + ".md")).read_text()
    assert rep["hyparview"]["n_up"] == rep["scamp_v2"]["n_up"] == 1 << 12
    assert rep["hyparview"]["rounds"] == rep["scamp_v2"]["rounds"]
    assert rep["scamp_v2"]["links"] > 0 and rep["hyparview"]["links"] > 0
    assert "| components |" in md and "In-degree histogram" in md
