"""psim_get_resilience on the GPU: every field of the struct, exactly, against
the reference (tests/_resilience.py) applied to the CPU oracle's rows of the
same scenario -- the expected values never come from the engine.  HyParView,
X-BOT, SCAMP v1 and v2; one shard, virtual shards and loopback ranks; the
64-case grid of the report, nested failure sets from one source, a level cap,
dead sources, views of 128 ids, agreement with graph_metrics(), the error
paths, empty handles, read-only, and the report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _graph_metrics as G
import _resilience as R
import _scenarios as S
from _oracle import Oracle
from partisan_amd.sim import SimError, _Driver, default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 0xFFFFFFFF


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


def _call(sim, cases, fail_seed=0, max_levels=0):
    """resilience() of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    src, thr, salt = ([c[k] for c in cases] for k in range(3))
    if hasattr(sim, "ranks"):
        ms = sim._threads("resilience", src, thr, salt, fail_seed, max_levels)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), "ranks disagree on the resilience struct"
        return ms[0]
    return sim.resilience(src, thr, salt, fail_seed=fail_seed, max_levels=max_levels)


_ROWS = {}


def _rows(key, run, kind):
    """the oracle's rows of a scenario, taken once"""
    if key not in _ROWS:
        o = run(Oracle)[0]
        _ROWS[key] = o.nodes() if kind == "hv" else o.strategy_nodes()
        o.close()
    return _ROWS[key]


_REF = {}


def _want(key, run, kind, cases, fail_seed=0, max_levels=0):
    k = (key, tuple(cases), fail_seed, max_levels)
    if k not in _REF:
        _REF[k] = R.reference_rows(G.rows_of(_rows(key, run, kind), kind), cases, fail_seed, max_levels)
    return _REF[k]


def _check(make, key, run, kind, cases, fail_seed=0, max_levels=0):
    """a scenario on the engine against the reference over the oracle's rows"""
    want = _want(key, run, kind, cases, fail_seed, max_levels)
    g = run(make)[0]
    try:
        R.compare(_call(g, cases, fail_seed, max_levels), want)
    finally:
        g.close()
    return want


def _seeded(n, seed, salt=0x6d, k=64):
    return np.random.Generator(np.random.PCG64([seed, salt])).choice(n, size=k, replace=False).astype(np.uint32)


def _spread(sources, seed):
    """64 cases over the sources given: thresholds over the whole range, 5 salts"""
    rng = np.random.Generator(np.random.PCG64([seed, 0x72]))
    thr = rng.integers(0, 1 << 31, size=len(sources))
    return [(int(s), int(t), j % 5) for j, (s, t) in enumerate(zip(sources, thr))]


# ---- HyParView, 203 nodes (N no multiple of 64)
def _hv203(make):
    return S.doubling(make, n=203, seed=3, rounds=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(3), _loop(2)], ids=["gpu", "3-shards", "loopback-2"])
def test_hv_grid(make):
    """anchor A's 64-case grid"""
    want = _check(make, "hv203", _hv203, "hv", R.grid(R.SRC_A), fail_seed=7)
    assert (want["n_up"], want["links"], want["cases_live"]) == (203, 790, 64)
    for q, (alive, links_alive, reached, hop_sum, no_in, _) in R.GRID_A.items():
        s = slice(8 * q, 8 * q + 8)
        assert (want["alive"][s].sum(), want["links_alive"][s].sum(), want["reached"][s].sum(),
                want["hop_sum"][s].sum(), want["no_in"][s].sum()) == (alive, links_alive, reached, hop_sum, no_in)


def test_hv_one_source_nested_sets():
    """64 cases from source 5 with salt 0: the failed sets are nested"""
    cases = [(5, (j * FULL) // 63, 0) for j in range(64)]
    want = _check(_gpu, "hv203", _hv203, "hv", cases, fail_seed=7)
    assert want["alive"][0] == 203 and want["alive"][63] == 1 and (np.diff(want["alive"].astype(np.int64)) <= 0).all()
    assert want["reached"][0] == 202 and want["reached"][63] == 0


def test_hv_level_cap():
    want = _check(_gpu, "hv203", _hv203, "hv", R.grid(R.SRC_A), fail_seed=7, max_levels=3)
    assert (want["levels"], want["truncated"], want["ecc_max"]) == (3, 1, 3)
    one = _want("hv203", _hv203, "hv", [(5, 0, 0)], 7, 3)
    assert (one["reached"][0], one["hop_sum"][0]) == (57, 146)
    g = _hv203(_gpu)[0]
    try:
        R.compare(_call(g, [(5, 0, 0)], 7, 3), one)
        # a cap past the largest is clamped to it
        R.compare(_call(g, R.grid(R.SRC_A), 7, 1 << 20), _want("hv203", _hv203, "hv", R.grid(R.SRC_A), 7))
    finally:
        g.close()


def test_hv_dead_sources():
    """crash_only: 4 of the 64 seeded sources are down; their slots read 0"""
    def run(mk):
        return S.crash_only(mk)[:2]
    src = _seeded(1024, 2, salt=99)
    want = _check(_gpu, "crash_only", run, "hv", _spread(src, 1), fail_seed=3)
    dead = [j for j, s in enumerate(src) if not _rows("crash_only", run, "hv")["up"][s]]
    assert len(dead) == 4 and want["cases_live"] == 60
    assert all(not (want["live_mask"] >> j) & 1 for j in dead)
    assert not any(want[k][dead].any() for k in R.ARRAYS)
    assert want["alive"][[j for j in range(64) if j not in dead]].all()


def test_xbot_churn():
    def run(mk):
        return S.xbot_churn(mk)
    want = _check(_vshards(2), "xbot", run, "hv", _spread(_seeded(2048, 0), 2), fail_seed=11)
    assert want["cases_live"] > 0 and want["reached"].any() and want["no_in"].any()


# ---- SCAMP
def _crashed(make):
    return S.pl_doubling(make, n=2048, seed=13, rounds=33, strategy=2, crash_at=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(4)], ids=["gpu", "4-shards"])
def test_v2_grid(make):
    """anchor B: a directed overlay with dead nodes"""
    want = _check(make, "crash33", _crashed, "scamp", R.grid(R.SRC_B), fail_seed=7)
    assert want["n_up"] == 1844 and want["cases_live"] == 64
    assert (want["alive"][:8].sum(), want["reached"][:8].sum(), want["hop_sum"][:8].sum()) == (14752, 1975, 15260)
    assert (want["no_in"][24:32].sum(), want["no_out"][24:32].sum()) == (3761, 2656)


@pytest.mark.parametrize("make", [_gpu, _loop(2)], ids=["gpu", "loopback-2"])
def test_v1_large_view(make):
    """views of more than 100 ids: the link counters past one bit plane"""
    def run(mk):
        return S.pl_v1_large_view(mk, leave_from=10**9, leave_to=0, rounds=40)
    assert _rows("v1", run, "scamp")["view_n"].max() > 100
    src = _seeded(180, 4)
    want = _check(make, "v1", run, "scamp", [(int(s), (j % 8 << 32) // 10, j % 3) for j, s in enumerate(src)],
                  fail_seed=5)
    assert want["links_alive"].max() == want["links"] > 400 and want["reached"].any()


# ---- agreement with the existing call
@pytest.mark.parametrize("kind", ["hv", "scamp"])
def test_agrees_with_graph_metrics(kind):
    run, n = (_hv203, 203) if kind == "hv" else (_crashed, 2048)
    src = _seeded(n, 6)
    g = run(_gpu)[0]
    try:
        gm = g.graph_metrics(src)
        m = g.resilience(src, np.zeros(64, np.uint32), np.arange(64), fail_seed=9)
    finally:
        g.close()
    live = np.array([(m["live_mask"] >> j) & 1 for j in range(64)], np.uint64)
    assert m["cases_live"] == gm["sources_live"] and (kind == "hv" or 0 < m["cases_live"] < 64)
    assert np.array_equal(m["reached"], gm["reach"]) and np.array_equal(m["ecc"], gm["ecc"])
    assert int(m["hop_sum"].sum()) == gm["dist_sum"]
    assert np.array_equal(m["alive"], live * np.uint64(gm["n_up"]))
    assert np.array_equal(m["links_alive"], live * np.uint64(gm["links"]))
    assert (m["n_up"], m["links"], m["ecc_max"], m["levels"], m["truncated"]) == (
        gm["n_up"], gm["links"], gm["ecc_max"], gm["levels"], gm["truncated"])


# ---- arguments, errors, empty handles
def test_error_paths():
    from partisan_amd import HostSim, _abi
    hv = _gpu(default_config(n_nodes=64, seed=1))
    fn, m = hv._extra["get_resilience"], _abi.PsimResilience()
    cs = (_abi.PsimFailureCase * 65)()
    assert fn(hv._h, None, 0, 0, 0, None) == -1                       # PSIM_EINVAL: null out
    assert fn(None, None, 0, 0, 0, m) == -1                           # null handle
    assert fn(hv._h, None, 3, 0, 0, m) == -1                          # null cases, n_cases > 0
    assert fn(hv._h, cs, 65, 0, 0, m) == -1                           # 65 cases
    assert fn(hv._h, cs, 64, 0, 0, m) == 0
    cs[2].reserved, cs[1].source = 1, 64
    assert fn(hv._h, cs, 3, 0, 0, m) == -1                            # a non-zero reserved, before the range
    cs[2].reserved = 0
    assert fn(hv._h, cs, 3, 0, 0, m) == -5                            # PSIM_ERANGE: a source == n_nodes
    with pytest.raises(SimError) as e:
        hv.resilience([64], [0])
    assert e.value.rc == -5
    with pytest.raises(SimError) as e:
        hv.resilience(np.zeros(65), np.zeros(65))
    assert e.value.rc == -1
    with pytest.raises(ValueError):
        hv.resilience([1, 2], [0])
    hv.resilience([5, 5], [0, 0])                                     # a repeated source is legal
    hv.close()
    full = _gpu(default_config(n_nodes=64, seed=1, manager=1, strategy=0))
    with pytest.raises(SimError) as e:
        full.resilience([1], [0])
    assert e.value.rc == -7                                           # PSIM_EUNSUPPORTED
    assert full._extra["get_resilience"](full._h, cs, 65, 0, 0, m) == -1     # (EINVAL comes first)
    full.close()
    host = HostSim(default_config(n_nodes=64, seed=1), 16, 48)
    with pytest.raises(SimError) as e:
        host.resilience([20], [0])
    assert e.value.rc == -7
    # (PSIM_ESTATE: only a host-exchange handle can hold a round open, and it answers unsupported first)
    host.close()


def test_no_cases_fills_the_counts():
    want = _want("hv203", _hv203, "hv", [])
    assert (want["n_up"], want["links"], want["levels"]) == (203, 790, 0)
    g = _hv203(_gpu)[0]
    try:
        R.compare(g.resilience([], []), want)
    finally:
        g.close()


@pytest.mark.parametrize("cfg", [dict(), dict(manager=2), dict(manager=1, strategy=1), dict(manager=1, strategy=2)],
                         ids=["hyparview", "xbot", "scamp-v1", "scamp-v2"])
def test_no_node_ever_started(cfg):
    for n in (300, 37):
        s = _gpu(default_config(n_nodes=n, seed=1, **cfg))
        for rounds in (0, 2):
            if rounds:
                s.step(rounds)
            for src in ([], [0, n - 1, 17, 17]):
                m = s.resilience(src, [0] * len(src))
                assert all(not np.any(v) for v in m.values()), m
        s.close()


def test_fewer_than_64_nodes():
    def run(mk):
        return S.doubling(mk, n=37, seed=3, rounds=20)
    src = np.arange(64) % 37
    want = _check(_gpu, "hv37", run, "hv", _spread(src, 3), fail_seed=1)
    assert want["n_up"] == 37 and want["cases_live"] == 64 and want["reached"].any()


# ---- read-only
class _CallAt:
    """a handle that takes its resilience struct once, before the step of round `at`"""
    run_schedule = _Driver.run_schedule

    def __init__(self, sim, at):
        self._sim, self._at, self.seen = sim, at, []

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def step(self, k=1):
        if self._sim.round == self._at and not self.seen:
            src = _seeded(2048, 5)
            self.seen.append(self._sim.resilience(src, np.full(64, 1 << 30), np.arange(64) % 4, fail_seed=2))
        return self._sim.step(k)


def test_read_only():
    """a call in the middle of churn_partition changes no later round"""
    o, ost = S.churn_partition(Oracle)
    box = []

    def make(cfg):
        box.append(_CallAt(_gpu(cfg), 95))       # (inside the partition, after the churn)
        return box[0]
    g, gst = S.churn_partition(make)
    assert g.seen and g.seen[0]["n_up"] == 2048 and g.seen[0]["reached"].any()
    S.compare_stats(gst, ost)
    S.compare_nodes(g.nodes(), o.nodes())
    cases = _spread(_seeded(2048, 5), 4)
    R.compare(_call(g, cases, 2), R.reference_rows(G.rows_of(o.nodes(), "hv"), cases, 2))
    g.close(); o.close()


# ---- the report
def test_resilience_report(tmp_path):
    from partisan_amd import resilience_report as P
    from partisan_amd import workloads as W
    n, seed = 1 << 12, 31
    r = subprocess.run([sys.executable, "-m", "partisan_amd.resilience_report", "--nodes", str(n), "--seed", str(seed),
                        "--out", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads((tmp_path / f"report_n{n}.json").read_text())
    assert json.loads(json.dumps(rep, indent=1, sort_keys=True)) == rep
    md = (tmp_path / f"report_n{n}.md").read_text()
    assert sum(1 for line in md.splitlines() if line.startswith("| 0% |")) == 2
    assert sum(1 for line in md.splitlines() if line.startswith("| 70% |")) == 2
    sched = W.doubling_join(n, seed)
    for key, _, extra in P.SIDES:
        x = rep[key]
        assert len(x["rows"]) == 8 and len(x["sources"]) == 8 and [w["failed_share"] for w in x["rows"]] == [
            q / 10 for q in range(8)]
        # the q = 0 row is what graph_metrics() gives for the same 8 sources
        with _gpu(default_config(n_nodes=n, seed=seed, **extra)) as g:
            g.run_schedule(sched, rep["round"])
            gm = g.graph_metrics(x["sources"])
        r0 = x["rows"][0]
        assert (x["n_up"], x["links"]) == (gm["n_up"], gm["links"])
        assert (r0["cases"], r0["alive"], r0["reached"], r0["hop_sum"], r0["ecc_max"]) == (
            8, 8 * gm["n_up"], int(gm["reach"].sum()), gm["dist_sum"], gm["ecc_max"])
        assert r0["reliability"] == r0["reached"] / (r0["alive"] - 8)
        rel = [w["reliability"] for w in x["rows"]]
        assert rel[0] >= rel[-1] and all(0 <= v <= 1 for v in rel)
