"""psim_get_graph_metrics on the GPU: every field of the struct against the
reference (tests/_graph_metrics.py) applied to the CPU oracle's rows of the
same scenario -- the expected values never come from the engine.  HyParView,
X-BOT, SCAMP v1 and v2; one shard, virtual shards and loopback ranks; exact
all-pairs on a small overlay, dead sources, a level cap, overlays in parts,
views of 128 ids."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _graph_metrics as R
import _scenarios as S
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


def _call(sim, sources, max_levels=0):
    """graph_metrics() of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    if hasattr(sim, "ranks"):
        ms = sim._threads("graph_metrics", sources, 64, 0, max_levels)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), "ranks disagree on the graph metrics"
        return ms[0]
    return sim.graph_metrics(sources, max_levels=max_levels)


def _all_pairs(sim, n, max_levels=0):
    """every id a source, 64 a call, summed as the reference sums them"""
    out = None
    reach, ecc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for lo in range(0, n, 64):
        ids = np.arange(lo, min(n, lo + 64), dtype=np.uint32)
        m = _call(sim, ids, max_levels)
        assert not m["reach"][ids.size:].any() and not m["ecc"][ids.size:].any()
        reach[ids], ecc[ids] = m["reach"][: ids.size], m["ecc"][: ids.size]
        if out is None:
            out = m
            continue
        for f in R.PATH_SUMS:
            out[f] = out[f] + m[f]
        for f in ("ecc_max", "levels", "truncated"):
            out[f] = max(out[f], m[f])
    out["reach"], out["ecc"] = reach, ecc
    return out


def _seeded(n, seed, salt=0x6d, k=64):
    return np.random.Generator(np.random.PCG64([seed, salt])).choice(n, size=k, replace=False).astype(np.uint32)


_ROWS = {}


def _rows(key, run, kind):
    """the oracle's rows of a scenario, taken once"""
    if key not in _ROWS:
        o = run(Oracle)[0]
        _ROWS[key] = o.nodes() if kind == "hv" else o.strategy_nodes()
        o.close()
    return _ROWS[key]


_REF = {}


def _want(key, run, kind, sources, max_levels=0):
    k = (key, None if sources is None else tuple(int(s) for s in sources), max_levels)
    if k not in _REF:
        rows = _rows(key, run, kind)
        _REF[k] = (R.reference_all(rows, kind, max_levels) if sources is None
                   else R.reference(rows, kind, sources, max_levels))
    return _REF[k]


def _check(make, key, run, kind, sources, max_levels=0, links_of=None):
    """a scenario on the engine against the reference over the oracle's rows;
    links_of: the statistics call and field whose link count must agree"""
    want = _want(key, run, kind, sources, max_levels)
    g = run(make)[0]
    try:
        R.compare(_call(g, sources, max_levels), want)
        if links_of:
            fn, field = links_of
            stats = g._threads(fn)[0] if hasattr(g, "ranks") else getattr(g, fn)()
            assert stats[field] == want["links"]
    finally:
        g.close()
    return want


# ---- HyParView: exact all-pairs on a small overlay
def _hv203(make):
    return S.doubling(make, n=203, seed=3, rounds=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(3), _loop(2)], ids=["gpu", "3-shards", "loopback-2"])
def test_hv_all_pairs(make):
    """203 nodes, every id a source: four calls, the last with 11 sources"""
    want = _want("hv203", _hv203, "hv", None)
    assert want["n_up"] == 203 and want["sources_live"] == 203 and want["pairs_unreached"] == 0
    assert round(want["dist_sum"] / want["pairs_reached"], 2) == 4.70 and want["ecc_max"] == 10
    assert (want["cl_closed"], want["cl_pairs"]) == (150, 2504)
    g = _hv203(make)[0]
    try:
        R.compare(_all_pairs(g, 203), want)
        assert g.histograms()["active_links"] == want["links"]
        if not hasattr(g, "ranks"):
            R.compare(g.graph_metrics_all(), want)
    finally:
        g.close()


def test_hv_level_cap():
    want = _want("hv203", _hv203, "hv", None, 3)
    assert want["truncated"] == 1 and want["levels"] == 3 and want["ecc_max"] == 3
    assert not want["dist"][4:].any() and want["pairs_unreached"] > 0
    g = _hv203(_gpu)[0]
    try:
        got = _all_pairs(g, 203, 3)
        R.compare(got, want)
        assert not got["dist"][4:].any() and got["truncated"] == 1
        # a cap past the largest is clamped to it
        R.compare(g.graph_metrics(np.arange(64), max_levels=1 << 20),
                  _want("hv203", _hv203, "hv", np.arange(64)))
    finally:
        g.close()


def test_hv_dead_sources():
    """crash_only: 4 of the 64 seeded sources are down; their slots read 0"""
    def run(mk):
        return S.crash_only(mk)[:2]
    src = _seeded(1024, 2, salt=99)
    want = _check(_gpu, "crash_only", run, "hv", src, links_of=("histograms", "active_links"))
    dead = [j for j, s in enumerate(src) if not _rows("crash_only", run, "hv")["up"][s]]
    assert len(dead) == 4 and want["sources_live"] == 60
    assert not want["reach"][dead].any() and not want["ecc"][dead].any()
    assert want["reach"][[j for j in range(64) if j not in dead]].all()


def test_xbot_churn_unreached_pairs():
    def run(mk):
        return S.xbot_churn(mk)
    src = _seeded(2048, 0)
    want = _check(_vshards(2), "xbot", run, "hv", src, links_of=("histograms", "active_links"))
    assert want["pairs_unreached"] > 0 and want["cl_nodes"] < want["n_up"]
    # the default draw of Simulator.graph_metrics is this one
    g = run(_gpu)[0]
    try:
        R.compare(g.graph_metrics(seed=0), want)
    finally:
        g.close()


def _two_parts(make, n=203, cut=100, rounds=40):
    """ids below `cut` bootstrapped from node 0, the rest from node `cut`, ten
    of each part a round: two overlays that never meet"""
    sim = make(default_config(n_nodes=n, seed=11))
    sched = [(0, np.array([0, cut], np.uint32), np.array([W.NONE, W.NONE], np.uint32))]
    a, b = np.arange(1, cut, dtype=np.uint32), np.arange(cut + 1, n, dtype=np.uint32)
    for r in range(1, 1 + (max(a.size, b.size) + 9) // 10):
        x, y = a[(r - 1) * 10: r * 10], b[(r - 1) * 10: r * 10]
        sched.append((r, np.concatenate([x, y]),
                      np.concatenate([np.zeros(x.size, np.uint32), np.full(y.size, cut, np.uint32)])))
    return sim, sim.run_schedule(sched, rounds)


def test_hv_two_parts_never_meet():
    src = np.array([0, 150, 99, 100, 202, 7, 101], np.uint32)
    want = _check(_gpu, "parts", _two_parts, "hv", src, links_of=("histograms", "active_links"))
    assert want["n_up"] == 203 and want["sources_live"] == src.size
    for j, s in enumerate(src):
        assert 0 < want["reach"][j] <= (100 if s < 100 else 103) - 1
    assert want["pairs_unreached"] >= sum(103 if s < 100 else 100 for s in src)


# ---- SCAMP
def _crashed(n, rounds):
    return lambda make: S.pl_doubling(make, n=n, seed=13, rounds=rounds, strategy=2, crash_at=30)


@pytest.mark.parametrize("make", [_gpu, _vshards(4)], ids=["gpu", "4-shards"])
def test_v2_crashed_tenth(make):
    want = _check(make, "crash33", _crashed(2048, 33), "scamp", _seeded(2048, 1),
                  links_of=("strategy_histograms", "links"))
    assert want["n_up"] == 1844 and want["pairs_unreached"] > want["pairs_reached"]


def test_v2_full_row():
    """rounds = 50: a view of 128 ids, the full two-register row"""
    rows = _rows("crash50", _crashed(2048, 50), "scamp")
    assert rows["view_n"].max() == 128
    big = int(np.argmax(rows["view_n"]))
    src = np.unique(np.concatenate([_seeded(2048, 2)[:63], [big]])).astype(np.uint32)
    want = _check(_gpu, "crash50", _crashed(2048, 50), "scamp", src, links_of=("strategy_histograms", "links"))
    assert want["cl_closed"] > 0


def test_v2_partition():
    def run(mk):
        return S.pl_doubling(mk, n=2048, seed=13, rounds=40, strategy=2, part_at=12)
    want = _check(_gpu, "part", run, "scamp", _seeded(2048, 3), links_of=("strategy_histograms", "links"))
    assert want["pairs_unreached"] > 0


@pytest.mark.parametrize("make", [_gpu, _loop(2)], ids=["gpu", "loopback-2"])
def test_v1_large_view(make):
    def run(mk):
        return S.pl_v1_large_view(mk, leave_from=10**9, leave_to=0, rounds=40)
    want = _check(make, "v1", run, "scamp", _seeded(180, 4), links_of=("strategy_histograms", "links"))
    assert _rows("v1", run, "scamp")["view_n"].max() > 100
    assert (want["cl_closed"], want["cl_pairs"]) == (313, 11994)


# ---- arguments, errors, empty handles
def test_error_paths():
    from partisan_amd import HostSim, _abi
    hv = _gpu(default_config(n_nodes=64, seed=1))
    fn, m = hv._extra["get_graph_metrics"], _abi.PsimGraphMetrics()
    ids = np.arange(65, dtype=np.uint32) % 64
    assert fn(hv._h, None, 0, 0, None) == -1                          # PSIM_EINVAL: null out
    assert fn(None, None, 0, 0, m) == -1                              # null handle
    assert fn(hv._h, None, 3, 0, m) == -1                             # null sources, n_sources > 0
    assert fn(hv._h, _abi.u32p(ids), 65, 0, m) == -1                  # 65 sources
    with pytest.raises(SimError) as e:
        hv.graph_metrics([3, 9, 3])                                   # a repeated source
    assert e.value.rc == -1
    with pytest.raises(SimError) as e:
        hv.graph_metrics([64])                                        # a source == n_nodes
    assert e.value.rc == -5
    with pytest.raises(SimError) as e:
        hv.graph_metrics(np.arange(65))
    assert e.value.rc == -1
    with pytest.raises(SimError) as e:
        hv.graph_metrics([5, 5])
    assert e.value.rc == -1
    hv.close()
    full = _gpu(default_config(n_nodes=64, seed=1, manager=1, strategy=0))
    with pytest.raises(SimError) as e:
        full.graph_metrics([1])
    assert e.value.rc == -7
    full.close()
    host = HostSim(default_config(n_nodes=64, seed=1), 16, 48)
    with pytest.raises(SimError) as e:
        host.graph_metrics([20])
    assert e.value.rc == -7
    host.close()


@pytest.mark.parametrize("cfg", [dict(), dict(manager=2), dict(manager=1, strategy=1), dict(manager=1, strategy=2)],
                         ids=["hyparview", "xbot", "scamp-v1", "scamp-v2"])
def test_no_node_ever_started(cfg):
    s = _gpu(default_config(n_nodes=300, seed=1, **cfg))
    for rounds in (0, 2):
        if rounds:
            s.step(rounds)
        for src in ([], [0, 299, 17]):
            m = s.graph_metrics(src)
            assert all(not np.any(v) for v in m.values()), m
    s.close()


def test_no_sources_fills_the_clustering_half():
    want = _want("hv203", _hv203, "hv", [])
    assert want["cl_closed"] == 150 and want["levels"] == 0 and not want["dist"].any()
    g = _hv203(_gpu)[0]
    try:
        R.compare(g.graph_metrics([]), want)
    finally:
        g.close()


# ---- read-only
class _CallAt:
    """a handle that takes its graph metrics once, before the step of round `at`"""
    run_schedule = _Driver.run_schedule

    def __init__(self, sim, at):
        self._sim, self._at, self.seen = sim, at, []

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def step(self, k=1):
        if self._sim.round == self._at and not self.seen:
            self.seen.append(self._sim.graph_metrics(seed=5))
        return self._sim.step(k)


def test_read_only():
    """a call in the middle of churn_partition changes no later round"""
    o, ost = S.churn_partition(Oracle)
    box = []

    def make(cfg):
        box.append(_CallAt(_gpu(cfg), 95))       # (inside the partition, after the churn)
        return box[0]
    g, gst = S.churn_partition(make)
    assert g.seen and g.seen[0]["n_up"] == 2048 and g.seen[0]["pairs_reached"] > 0
    S.compare_stats(gst, ost)
    S.compare_nodes(g.nodes(), o.nodes())
    src = _seeded(2048, 5)
    R.compare(g.graph_metrics(src), R.reference(o.nodes(), "hv", src))
    g.close(); o.close()


# ---- the report
def test_overlay_report(tmp_path):
    r = subprocess.run([sys.executable, "-m", "partisan_amd.overlay_report", "--nodes", str(1 << 12), "--seed", "31",
                        "--out", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    stem = f"d_compare_n{1 << 12}_s31"
    rep = json.loads((tmp_path / (stem + ".json")).read_text())
    md = (tmp_path / (stem + ".md")).read_text()
    for side in ("hyparview", "scamp_v2"):
        x = rep[side]
        assert {"clustering_mean", "path_mean", "path_max", "pairs_unreached"} <= set(x)
        assert x["path_mean"] > 1 and 0 <= x["clustering_mean"] < 1 and x["path_max"] >= 2
    for row in ("| clustering_mean", "| path_mean", "| path_max"):
        assert sum(1 for line in md.splitlines() if line.startswith(row)) == 1
    assert "| components |" in md and "In-degree histogram" in md         # (the rows from before stay)
