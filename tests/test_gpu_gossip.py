"""psim_get_gossip_reach on the GPU: every field of the struct, exactly, against
the reference (tests/_gossip.py) applied to the CPU oracle's rows of the same
scenario -- the expected values never come from the engine.  HyParView, X-BOT,
SCAMP v1 and v2; one shard, virtual shards and loopback ranks; the report's
64-case grids, single cases, a level cap, views past 100 ids, dead sources,
agreement with resilience(), the error paths, empty handles, read-only, and the
report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _gossip as P
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
    """gossip_reach() of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    src, thr, salt, fan = ([c[k] for c in cases] for k in range(4))
    if hasattr(sim, "ranks"):
        ms = sim._threads("gossip_reach", src, fan, thr, salt, fail_seed, max_levels)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), "ranks disagree on the gossip struct"
        return ms[0]
    return sim.gossip_reach(src, fan, thr, salt, fail_seed=fail_seed, max_levels=max_levels)


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
        _REF[k] = P.reference_rows(G.rows_of(_rows(key, run, kind), kind), cases, fail_seed, max_levels)
    return _REF[k]


def _check(make, key, run, kind, case_sets, fail_seed=0, max_levels=0):
    """a scenario on the engine, one call per case set, each against the
    reference over the oracle's rows"""
    wants = [_want(key, run, kind, cases, fail_seed, max_levels) for cases in case_sets]
    g = run(make)[0]
    try:
        for cases, want in zip(case_sets, wants):
            P.compare(_call(g, cases, fail_seed, max_levels), want)
    finally:
        g.close()
    return wants


def _seeded(n, seed, salt=0x6d, k=64):
    return np.random.Generator(np.random.PCG64([seed, salt])).choice(n, size=k, replace=False).astype(np.uint32)


def _spread(sources, seed):
    """64 cases over the sources given: thresholds over half the range, 5 salts, fanouts 0 .. 9"""
    rng = np.random.Generator(np.random.PCG64([seed, 0x67]))
    thr = rng.integers(0, 1 << 31, size=len(sources))
    fan = rng.integers(0, 10, size=len(sources))
    return [(int(s), int(t), j % 5, int(f)) for j, (s, t, f) in enumerate(zip(sources, thr, fan))]


def _sums(m, s):
    return tuple(int(m[k][s].sum()) for k in ("alive", "reached", "hop_sum", "sent", "lost")) + (int(m["ecc"][s].max()),)


# ---- HyParView, 203 nodes (N no multiple of 64)
def _hv203(make):
    return S.doubling(make, n=203, seed=3, rounds=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(3), _loop(2)], ids=["gpu", "3-shards", "loopback-2"])
def test_hv_grids(make):
    """anchor A: the report's three 64-case grids"""
    wants = _check(make, "hv203", _hv203, "hv", [P.grid(R.SRC_A, q) for q in (0, 3, 5)], fail_seed=7)
    for q, want in zip((0, 3, 5), wants):
        assert (want["n_up"], want["links"], want["cases_live"]) == (203, 790, 64)
        for fi in range(8):
            assert _sums(want, slice(8 * fi, 8 * fi + 8)) == P.ANCHOR_A[q][min(fi, 4)]


def test_hv_single_cases_and_cap():
    sets = [[(5, 0, 0, f)] for f in (2, 3, 0)]
    g = _hv203(_gpu)[0]
    try:
        for cases, x in zip(sets, [(131, 1602, 21, 264), (198, 1261, 12, 574), (202, 831, 7, 790)]):
            want = _want("hv203", _hv203, "hv", cases, 7)
            assert tuple(int(want[k][0]) for k in ("reached", "hop_sum", "ecc", "sent")) == x
            P.compare(_call(g, cases, 7), want)
        # the cap: the nodes found at level 3 do not send
        want = _want("hv203", _hv203, "hv", [(5, 0, 0, 2)], 7, 3)
        assert (want["reached"][0], want["hop_sum"][0], want["sent"][0], want["truncated"]) == (7, 15, 10, 1)
        P.compare(_call(g, [(5, 0, 0, 2)], 7, 3), want)
        grid = P.grid(R.SRC_A, 3)
        want = _want("hv203", _hv203, "hv", grid, 7, 3)
        assert (want["levels"], want["truncated"], want["ecc_max"]) == (3, 1, 3)
        P.compare(_call(g, grid, 7, 3), want)
        # a cap past the largest is clamped to it
        P.compare(_call(g, grid, 7, 1 << 20), _want("hv203", _hv203, "hv", grid, 7))
    finally:
        g.close()


def test_hv_dead_sources():
    """crash_only: 4 of the 64 seeded sources are down; their slots read 0"""
    def run(mk):
        return S.crash_only(mk)[:2]
    src = _seeded(1024, 2, salt=99)
    want = _check(_gpu, "crash_only", run, "hv", [_spread(src, 1)], fail_seed=3)[0]
    dead = [j for j, s in enumerate(src) if not _rows("crash_only", run, "hv")["up"][s]]
    assert len(dead) == 4 and want["cases_live"] == 60
    assert all(not (want["live_mask"] >> j) & 1 for j in dead)
    assert not any(want[k][dead].any() for k in P.ARRAYS)
    assert want["alive"][[j for j in range(64) if j not in dead]].all() and want["lost"].any()


def test_xbot_churn():
    def run(mk):
        return S.xbot_churn(mk)
    want = _check(_vshards(2), "xbot", run, "hv", [_spread(_seeded(2048, 0), 2)], fail_seed=11)[0]
    assert want["cases_live"] > 0 and want["reached"].any() and want["lost"].any()


def test_fewer_than_64_nodes():
    def run(mk):
        return S.doubling(mk, n=37, seed=3, rounds=20)
    src = np.arange(64) % 37
    want = _check(_gpu, "hv37", run, "hv", [_spread(src, 3)], fail_seed=1)[0]
    assert want["n_up"] == 37 and want["cases_live"] == 64 and want["reached"].any()


# ---- SCAMP
def _crashed(make):
    return S.pl_doubling(make, n=2048, seed=13, rounds=33, strategy=2, crash_at=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(4)], ids=["gpu", "4-shards"])
def test_v2_grid(make):
    """anchor B: a directed overlay with dead nodes"""
    # the 16 longest rows as sources: 8 and 9 links (a thread / 16 lanes a node), up to 24 (two entries a lane)
    nb = G.links_of(G.rows_of(_rows("crash33", _crashed, "scamp"), "scamp"))
    longest = sorted(nb, key=lambda i: (-len(nb[i]), i))[:16]
    assert {8, 9, 14, 24} <= {len(nb[i]) for i in longest}
    long_cases = [(s, (k % 3 << 32) // 10, k % 4, f) for k, s in enumerate(longest) for f in (1, 3, 8, 9)]
    want, _, w3 = _check(make, "crash33", _crashed, "scamp", [P.b_cases(), _spread(_seeded(2048, 8), 5), long_cases],
                         fail_seed=7)
    assert want["n_up"] == 1844 and want["cases_live"] == 32
    for fi, f in enumerate(P.ANCHOR_B):
        assert _sums(want, slice(8 * fi, 8 * fi + 8))[:5] == P.ANCHOR_B[f]
    assert w3["cases_live"] == 64 and w3["sent"].min() >= 1 and w3["lost"].any()


@pytest.mark.parametrize("make", [_gpu, _loop(2)], ids=["gpu", "loopback-2"])
def test_v1_large_view(make):
    """views of more than 100 ids: ranks past one 64-lane register, counts past one bit plane"""
    def run(mk):
        return S.pl_v1_large_view(mk, leave_from=10**9, leave_to=0, rounds=40)
    assert _rows("v1", run, "scamp")["view_n"].max() > 100
    failing = [(s, (3 << 32) // 10, 2, f) for f in (1, 8, 64, 100, 0) for s in P.V1_SOURCES]
    # the smallest fanout 64: every row but the longest is chosen whole without a rank
    wide = [(s, (k << 32) // 10, k, f) for f in (64, 100, 107, 0) for k, s in enumerate(P.V1_SOURCES)]
    want, w2, _ = _check(make, "v1", run, "scamp", [P.v1_cases(), failing, wide], fail_seed=5)
    assert (want["n_up"], want["links"]) == (180, 424)
    got = [(int(want["reached"][j]), int(want["sent"][j]), int(want["ecc"][j])) for j in range(28)]
    assert got == [x for f in P.ANCHOR_V1 for x in P.ANCHOR_V1[f]]
    assert w2["lost"].any() and want["sent"].max() > 128


# ---- agreement with the existing call, engine against engine
@pytest.mark.parametrize("kind", ["hv", "scamp", "v1"])
def test_agrees_with_resilience(kind):
    run, n = {"hv": (_hv203, 203), "scamp": (_crashed, 2048),
              "v1": (lambda mk: S.pl_v1_large_view(mk, leave_from=10**9, leave_to=0, rounds=40), 180)}[kind]
    src = _seeded(n, 6)
    thr = np.arange(64, dtype=np.uint64) * (1 << 25)
    salt = np.arange(64) % 6
    g = run(_gpu)[0]
    try:
        for cap in (0, 2):
            r = g.resilience(src, thr, salt, fail_seed=9, max_levels=cap)
            for fan in (0, 128):
                m = g.gossip_reach(src, np.full(64, fan), thr, salt, fail_seed=9, max_levels=cap)
                for k in ("alive", "reached", "hop_sum", "ecc"):
                    assert np.array_equal(m[k], r[k]), (kind, fan, k)
                for k in ("levels", "truncated", "n_up", "links", "live_mask", "cases_live", "ecc_max"):
                    assert m[k] == r[k], (kind, fan, k)
        assert r["reached"].any()
    finally:
        g.close()


# ---- arguments, errors, empty handles
def test_error_paths():
    from partisan_amd import HostSim, _abi
    hv = _gpu(default_config(n_nodes=64, seed=1))
    fn, m = hv._extra["get_gossip_reach"], _abi.PsimGossipReach()
    cs = (_abi.PsimGossipCase * 65)()
    assert fn(hv._h, None, 0, 0, 0, None) == -1                       # PSIM_EINVAL: null out
    assert fn(None, None, 0, 0, 0, m) == -1                           # null handle
    assert fn(hv._h, None, 3, 0, 0, m) == -1                          # null cases, n_cases > 0
    cs[1].source = 64
    assert fn(hv._h, cs, 65, 0, 0, m) == -1                           # 65 cases, before the range
    assert fn(hv._h, cs, 3, 0, 0, m) == -5                            # PSIM_ERANGE: a source == n_nodes
    cs[1].source, cs[1].fanout, cs[2].fanout = 0, FULL, 1 << 31
    assert fn(hv._h, cs, 64, 0, 0, m) == 0                            # any fanout is legal
    with pytest.raises(SimError) as e:
        hv.gossip_reach([64], [0])
    assert e.value.rc == -5
    with pytest.raises(SimError) as e:
        hv.gossip_reach(np.zeros(65), np.zeros(65))
    assert e.value.rc == -1
    for bad in (([1, 2], [0]), ([1, 2], [0, 0], [0]), ([1, 2], [0, 0], None, [0])):
        with pytest.raises(ValueError):
            hv.gossip_reach(*bad)
    hv.gossip_reach([5, 5], [2, 2])                                   # a repeated source is legal
    hv.close()
    full = _gpu(default_config(n_nodes=64, seed=1, manager=1, strategy=0))
    with pytest.raises(SimError) as e:
        full.gossip_reach([1], [0])
    assert e.value.rc == -7                                           # PSIM_EUNSUPPORTED
    assert full._extra["get_gossip_reach"](full._h, cs, 65, 0, 0, m) == -1   # (EINVAL comes first)
    cs[1].source = 64
    assert full._extra["get_gossip_reach"](full._h, cs, 3, 0, 0, m) == -7    # (and the range last)
    full.close()
    host = HostSim(default_config(n_nodes=64, seed=1), 16, 48)
    with pytest.raises(SimError) as e:
        host.gossip_reach([20], [0])
    assert e.value.rc == -7
    # (PSIM_ESTATE: only a host-exchange handle can hold a round open, and it answers unsupported first)
    host.close()


def test_no_cases_fills_the_counts():
    want = _want("hv203", _hv203, "hv", [])
    assert (want["n_up"], want["links"], want["levels"]) == (203, 790, 0)
    g = _hv203(_gpu)[0]
    try:
        P.compare(g.gossip_reach([], []), want)
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
                m = s.gossip_reach(src, [2, 0, 1, 9][: len(src)])
                assert all(not np.any(v) for v in m.values()), m
        s.close()


# ---- read-only
class _CallAt:
    """a handle that takes its gossip struct once, before the step of round `at`"""
    run_schedule = _Driver.run_schedule

    def __init__(self, sim, at):
        self._sim, self._at, self.seen = sim, at, []

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def step(self, k=1):
        if self._sim.round == self._at and not self.seen:
            src = _seeded(2048, 5)
            self.seen.append(self._sim.gossip_reach(src, np.arange(64) % 7, np.full(64, 1 << 30), np.arange(64) % 4,
                                                    fail_seed=2))
        return self._sim.step(k)


def test_read_only():
    """a call in the middle of churn_partition changes no later round"""
    o, ost = S.churn_partition(Oracle)
    box = []

    def make(cfg):
        box.append(_CallAt(_gpu(cfg), 95))       # (inside the partition, after the churn)
        return box[0]
    g, gst = S.churn_partition(make)
    assert g.seen and g.seen[0]["n_up"] == 2048 and g.seen[0]["reached"].any() and g.seen[0]["lost"].any()
    S.compare_stats(gst, ost)
    S.compare_nodes(g.nodes(), o.nodes())
    cases = _spread(_seeded(2048, 5), 4)
    P.compare(_call(g, cases, 2), P.reference_rows(G.rows_of(o.nodes(), "hv"), cases, 2))
    g.close(); o.close()


# ---- the report
def test_gossip_report(tmp_path):
    from partisan_amd import gossip_report as Q
    from partisan_amd import resilience_report as RR
    from partisan_amd import workloads as W
    n, seed = 1 << 12, 31
    r = subprocess.run([sys.executable, "-m", "partisan_amd.gossip_report", "--nodes", str(n), "--seed", str(seed),
                        "--out", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads((tmp_path / f"report_n{n}.json").read_text())
    assert json.loads(json.dumps(rep, indent=1, sort_keys=True)) == rep
    md = (tmp_path / f"report_n{n}.md").read_text()
    assert sum(1 for line in md.splitlines() if line.startswith("| 30% | all |")) == 2
    assert sum(1 for line in md.splitlines() if line.startswith("| 50% |")) == 16
    assert list(Q.FANOUTS) == P.FANOUTS and rep["fanouts"] == P.FANOUTS and rep["shares"] == [0.0, 0.3, 0.5]
    sched = W.doubling_join(n, seed)
    for key, _, extra in RR.SIDES:
        x = rep[key]
        assert len(x["rows"]) == 24 and len(x["sources"]) == 8
        assert [(w["failed_share"], w["fanout"]) for w in x["rows"]] == [(q / 10, f) for q in (0, 3, 5) for f in P.FANOUTS]
        # the fanout-0 rows are what resilience() gives for the same cases
        with _gpu(default_config(n_nodes=n, seed=seed, **extra)) as g:
            g.run_schedule(sched, rep["round"])
            thr = [(q << 32) // 10 for q in (0, 3, 5) for _ in range(8)]
            rs = g.resilience(x["sources"] * 3, thr, list(range(8)) * 3, fail_seed=rep["fail_seed"])
        assert (x["n_up"], x["links"]) == (rs["n_up"], rs["links"])
        for qi, q in enumerate((0, 3, 5)):
            w, s = x["rows"][8 * qi + 7], slice(8 * qi, 8 * qi + 8)
            assert (w["failed_share"], w["fanout"], w["cases"]) == (q / 10, 0, 8)
            assert (w["alive"], w["reached"], w["hop_sum"], w["ecc_max"]) == (
                int(rs["alive"][s].sum()), int(rs["reached"][s].sum()), int(rs["hop_sum"][s].sum()),
                int(rs["ecc"][s].max()))
            assert w["reliability"] == w["reached"] / (w["alive"] - 8)
        for w in x["rows"]:
            assert 0 <= w["reliability"] <= 1 and 0 <= w["lost_share"] <= 1 and w["duplicates_per_delivery"] >= 0
            assert w["sent"] >= w["lost"] + w["reached"]
        # (equal salts choose nested sets as the fanout grows, so what a case reaches only grows)
        for qi in range(3):
            got = [w["reached"] for w in x["rows"][8 * qi: 8 * qi + 8]]
            assert got == sorted(got)
