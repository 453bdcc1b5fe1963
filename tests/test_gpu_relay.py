"""psim_get_relay_reach on the GPU: every field of the struct, exactly, against
the reference (tests/_relay.py) applied to the CPU oracle's rows of the same
scenario -- the expected values never come from the engine.  One shard,
virtual shards and loopback ranks; 64-case grids with mixed ttls, single cases,
a level cap, a small merge table and both lane layouts in fresh processes, the
restart cycle, dead ids, the error paths, empty handles, read-only, and the
report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _relay as P
import _scenarios as S
from _oracle import Oracle
from partisan_amd.sim import SimError, _Driver, default_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


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


def _call(sim, cases, max_levels=0):
    """relay_reach() of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    src, dst, ttl = ([c[k] for c in cases] for k in range(3))
    if hasattr(sim, "ranks"):
        ms = sim._threads("relay_reach", src, dst, ttl, max_levels)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), "ranks disagree on the relay struct"
        return ms[0]
    return sim.relay_reach(src, dst, ttl, max_levels=max_levels)


RUNS = {
    "a": lambda mk: S.doubling(mk, n=203, seed=3, rounds=30),            # N no multiple of 64 or 16
    "b": lambda mk: S.churn_partition(mk, n=512, rounds=60),
    "c": lambda mk: S.crash_only(mk)[:2],
}
_ROWS, _REF = {}, {}


def _rows(key):
    """the oracle's rows of a scenario, taken once"""
    if key not in _ROWS:
        o = RUNS[key](Oracle)[0]
        _ROWS[key] = P.rows_of(o.nodes())
        o.close()
    return _ROWS[key]


def _want(key, cases, max_levels=0):
    k = (key, tuple(cases), max_levels)
    if k not in _REF:
        _REF[k] = P.reference_rows(_rows(key), cases, max_levels)
    return _REF[k]


def _check(make, key, calls):
    """a scenario on the engine, one call per (cases, cap), each against the
    reference over the oracle's rows"""
    wants = [_want(key, cases, cap) for cases, cap in calls]
    g = RUNS[key](make)[0]
    try:
        for (cases, cap), want in zip(calls, wants):
            P.compare(_call(g, cases, cap), want)
    finally:
        g.close()
    return wants


A_SINGLE = [((5, 100, 5), 0), ((5, 100, 8), 0), ((0, 202, 3), 0), ((17, 64, 16), 0), ((17, 64, 16), 3), ((5, 50, 5), 0)]


@pytest.mark.parametrize("make", [_gpu, _vshards(3), _loop(2)], ids=["gpu", "3-shards", "loopback-2"])
def test_grids(make):
    """anchor A: three 64-case grids of seeded pairs, ttls 1 .. 16, a direct pair in each"""
    grids = [P.grid(_rows("a"), q) for q in (0, 3, 5)]
    wants = _check(make, "a", [(g, 0) for g in grids] + [(grids[1], 4)])
    for want in wants[:3]:
        assert [want[k] for k in P.CENSUS] == [203, 908, 790, 118, 0]
        assert want["cases_live"] == 64 and (want["direct_mask"] >> 7) & 1 and want["levels_max"] == 16
        assert want["delivered"].any() and want["expired"].any() and want["refused"].any()
        assert want["peak"].max() > 128                 # (most of the overlay on one level)
    assert wants[3]["truncated_mask"] and wants[3]["in_flight"].any() and wants[3]["levels_max"] == 4


def test_single_cases_and_cap():
    """the five anchor cases and the direct pair, one case a call"""
    wants = _check(_gpu, "a", [([c], cap) for c, cap in A_SINGLE])
    got = [tuple(int(w[k][0]) for k in ("delivered", "first_hop", "hop_sum", "relays", "refused", "expired", "levels"))
           + (w["truncated_mask"],) for w in wants]
    assert got[:5] == [(48, 2, 271, 1593, 175, 1170, 5, 0), (2400, 2, 20737, 108407, 12957, 80101, 8, 0),
                       (0, 0, 0, 41, 2, 31, 3, 0),
                       (45794999, 6, 764730062, 13597090566, 1011236305, 10394417266, 16, 0),
                       (0, 0, 0, 362, 55, 0, 3, 1)]
    assert wants[5]["direct_mask"] == 1 and got[5] == (1, 1, 1, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("lanes,slots", [("8", "16"), ("1", "16"), ("8", "")], ids=["group-16slots", "lane-16slots", "group"])
def test_small_table_and_lane_layouts(lanes, slots):
    """a fresh process a setting: a 16-slot table at the start (probes wrap,
    the table regrows level by level) and the 8-lane-group layout give the
    struct of the default call (a lane an entry, 2^16 slots)"""
    cases = P.grid(_rows("a"), 3)
    env = dict(os.environ, PSIM_RELAY_LANES=lanes)
    env.pop("PSIM_RELAY_SLOTS", None)
    if slots:
        env["PSIM_RELAY_SLOTS"] = slots
    for cs, cap in ((cases, 0), (cases, 4), ([A_SINGLE[3][0]], 0)):
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_relay_run.py"), json.dumps(cs), str(cap)], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        P.compare(json.loads(r.stdout.strip().splitlines()[-1]), _want("a", cs, cap))


@pytest.mark.parametrize("make", [_gpu, _vshards(2)], ids=["gpu", "2-shards"])
def test_restart_cycle(make):
    """anchor B: node 275 holds the target 119 as a member without a connection"""
    calls = [([(295, 119, ttl)], cap) for ttl, cap in ((1, 0), (3, 6), (5, 6), (5, 0))]
    wants = _check(make, "b", calls + [([(295, 119, t) for t in range(1, 17)] + P.grid(_rows("b"), 1, 48), 0)])
    got = [tuple(int(w[k][0]) for k in ("relays", "refused", "expired", "restarts", "levels")) + (w["truncated_mask"],)
           for w in wants[:4]]
    assert got == [(8, 1, 7, 1, 2, 0), (1706, 153, 568, 72, 6, 1), (9627, 590, 2215, 215, 6, 1),
                   (200105280, 12796992, 29688977, 4242794, 16, 1)]
    assert [wants[0][k] for k in P.CENSUS] == [512, 2072, 1962, 109, 1]
    assert not any(w["delivered"][0] for w in wants[:4]) and wants[4]["restarts"][:16].all()


def test_dead_ids():
    """anchor C: nodes 3, 20 and 37 are down; cases naming them are skipped"""
    cases = P.grid(_rows("c"), 2)
    for j, (s, d) in zip((0, 9, 18, 27, 36, 63), ((3, 100), (100, 20), (37, 3), (20, 500), (501, 37), (3, 20))):
        cases[j] = (s, d, cases[j][2])
    want = _check(_gpu, "c", [(cases, 0)])[0]
    assert [want[k] for k in P.CENSUS[:4]] == [963, 4256, 3842, 414]
    dead = [j for j, (s, d, _) in enumerate(cases) if not (_rows("c")[s][0] and _rows("c")[d][0])]
    assert {0, 9, 18, 27, 36, 63} <= set(dead) and want["cases_live"] == 64 - len(dead)
    assert all(not (want["live_mask"] >> j) & 1 for j in dead)
    assert not any(want[k][dead].any() for k in P.ARRAYS) and want["relays"].any()


def test_no_cases_fills_the_census():
    want = _want("a", [])
    assert [want[k] for k in P.CENSUS] == [203, 908, 790, 118, 0] and want["cases_live"] == 0
    g = RUNS["a"](_gpu)[0]
    try:
        P.compare(g.relay_reach([], [], []), want)
        P.compare(g.relay_reach([], [], 5), want)
    finally:
        g.close()


def test_no_node_ever_started():
    for n in (300, 37):
        s = _gpu(default_config(n_nodes=n, seed=1))
        for rounds in (0, 2):
            if rounds:
                s.step(rounds)
            for src, dst in (([], []), ([0, n - 1, 17, 17], [1, 0, 5, 5])):
                m = s.relay_reach(src, dst, 5)
                assert all(not np.any(v) for v in m.values()), m
        s.close()


# ---- arguments and errors, in the header's order
def test_error_paths():
    from partisan_amd import HostSim, _abi
    hv = _gpu(default_config(n_nodes=64, seed=1))
    fn, m = hv._extra["get_relay_reach"], _abi.PsimRelayReach()

    def cs(*cases, n=65):
        a = (_abi.PsimRelayCase * n)()
        for j in range(n):
            a[j].source, a[j].target, a[j].ttl, a[j].reserved = cases[j] if j < len(cases) else (0, 1, 5, 0)
        return a
    assert fn(hv._h, None, 0, 0, None) == -1                          # PSIM_EINVAL: null out
    assert fn(None, None, 0, 0, m) == -1                              # null handle
    assert fn(hv._h, None, 3, 0, m) == -1                             # null cases, n_cases > 0
    assert fn(hv._h, cs((64, 1, 5, 0)), 65, 0, m) == -1               # 65 cases, before the range
    assert fn(hv._h, cs((0, 1, 5, 1)), 3, 0, m) == -1                 # a non-zero reserved
    assert fn(hv._h, cs((0, 1, 0, 0)), 3, 0, m) == -1                 # ttl 0
    assert fn(hv._h, cs((0, 1, 17, 0)), 3, 0, m) == -1                # ttl above PSIM_RELAY_MAX_TTL
    assert fn(hv._h, cs((0, 1, 5, 0), (9, 9, 5, 0)), 3, 0, m) == -1   # source == target
    assert fn(hv._h, cs((64, 64, 5, 0)), 3, 0, m) == -1               # ... before the range
    assert fn(hv._h, cs((64, 1, 5, 0)), 3, 0, m) == -5                # PSIM_ERANGE: a source == n_nodes
    assert fn(hv._h, cs((0, 1, 5, 0), (1, 64, 16, 0)), 3, 0, m) == -5  # a target == n_nodes
    assert fn(hv._h, cs((0, 1, 16, 0)), 64, 99, m) == 0               # 64 equal cases, any cap
    with pytest.raises(SimError) as e:
        hv.relay_reach([64], [0], 5)
    assert e.value.rc == -5
    with pytest.raises(SimError) as e:
        hv.relay_reach(np.zeros(65), np.ones(65), 5)
    assert e.value.rc == -1
    for bad in (([1, 2], [0], 5), ([1, 2], [0, 0], [5])):
        with pytest.raises(ValueError):
            hv.relay_reach(*bad)
    hv.close()
    # PSIM_EUNSUPPORTED: after PSIM_EINVAL, before the range
    for cfg in (dict(manager=2), dict(manager=1, strategy=0), dict(manager=1, strategy=1), dict(manager=1, strategy=2),
                dict(plumtree=0)):
        s = _gpu(default_config(n_nodes=64, seed=1, **cfg))
        with pytest.raises(SimError) as e:
            s.relay_reach([1], [2], 5)
        assert e.value.rc == -7, cfg
        assert s._extra["get_relay_reach"](s._h, cs((0, 1, 0, 0)), 3, 0, m) == -1
        assert s._extra["get_relay_reach"](s._h, cs((64, 1, 5, 0)), 3, 0, m) == -7
        s.close()
    # a host-exchange handle, the only kind that can hold a round open: it
    # answers unsupported with and without one, so PSIM_ESTATE cannot be had
    # through the ABI (as with psim_get_gossip_reach)
    host = HostSim(default_config(n_nodes=64, seed=1), 16, 48)
    for opened in (False, True):
        if opened:
            host.emit()
        with pytest.raises(SimError) as e:
            host.relay_reach([20], [21], 5)
        assert e.value.rc == -7
    host.absorb(np.zeros((0, 16), np.uint32))
    host.close()


# ---- read-only
class _CallAt:
    """a handle that takes its relay struct once, before the step of round `at`"""
    run_schedule = _Driver.run_schedule

    def __init__(self, sim, at):
        self._sim, self._at, self.seen = sim, at, []

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def step(self, k=1):
        if self._sim.round == self._at and not self.seen:
            pairs = P.pairs(512, 5)
            self.seen.append(self._sim.relay_reach([p[0] for p in pairs], [p[1] for p in pairs], 1 + np.arange(64) % 8))
        return self._sim.step(k)


def test_read_only():
    """a call in the middle of churn_partition changes no later round"""
    o, ost = RUNS["b"](Oracle)
    box = []

    def make(cfg):
        box.append(_CallAt(_gpu(cfg), 45))
        return box[0]
    g, gst = RUNS["b"](make)
    assert g.seen and g.seen[0]["n_up"] > 0 and g.seen[0]["relays"].any()
    S.compare_stats(gst, ost)
    S.compare_nodes(g.nodes(), o.nodes())
    g.close(); o.close()


# ---- the report
def test_relay_report(tmp_path):
    from partisan_amd import relay_report as Q
    n = 1 << 12
    r = subprocess.run([sys.executable, "-m", "partisan_amd.relay_report", "--nodes", str(n), "--seed", "31",
                        "--out", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads((tmp_path / f"report_n{n}.json").read_text())
    md = (tmp_path / f"report_n{n}.md").read_text()
    assert [w["ttl"] for w in rep["rows"]] == list(Q.TTLS) == [1, 2, 3, 5, 8, 12, 16]
    for t in Q.TTLS:
        assert sum(1 for line in md.splitlines() if line.startswith(f"| {t} |")) == 1
    assert sum(1 for line in md.splitlines() if line.startswith("Census: ")) == 1
    assert rep["census"]["n_up"] == n and rep["census"]["out_usable"] <= rep["census"]["out_entries"]
    for w in rep["rows"]:
        assert w["cases"] == 64 and 0 <= w["delivered_share"] <= 1 and 0 <= w["refused_share"] <= 1
        assert w["messages_per_unicast"] * 64 == w["relays"] + w["delivered"]
    # a longer ttl walks every walk of a shorter one: nothing delivered is lost again
    got = [w["pairs_delivered"] for w in rep["rows"]]
    assert got == sorted(got) and rep["rows"][-1]["relays"] > rep["rows"][0]["relays"]
