"""psim_get_latency_metrics on the GPU: every field of the struct, exactly,
against the reference (tests/_latency.py) applied to the CPU oracle's rows of
the same scenario -- the expected values never come from the engine.  One
shard, virtual shards and loopback ranks; 64, 5, 1 and 0 sources; dead sources
and targets; a sweep cap; the SCAMP CSR with rows of more than 64 links; the
tree half on broadcasting, silent and dead roots and under X-BOT; both push
kernels and both forms of the weights; the error paths, empty handles, read-only, and
the report.  Each test first asserts on the reference that its scenario shows
what it is there for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _latency as P
import _scenarios as S
from _oracle import Oracle
from partisan_amd.sim import NONE, SimError, _Driver, default_config

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


MAKES = pytest.mark.parametrize("make", [_gpu, _vshards(3), _loop(2)], ids=["gpu", "3-shards", "loopback-2"])

# name: (scenario, kind of rows)
RUNS = {
    "a": (lambda mk: S.doubling(mk, n=203, seed=3, rounds=30), "hv"),            # N no multiple of 64 or 16
    "a_bcast": (lambda mk: S.doubling(mk, n=203, seed=3, rounds=60, bcast_period=10, bcast_first=30), "hv"),
    "config_a": (lambda mk: S.config_a(mk), "hv"),
    "xbot": (lambda mk: S.xbot_churn(mk, n=512, rounds=60), "hv"),
    "xbot80": (lambda mk: S.xbot_churn(mk, n=512, rounds=80), "hv"),
    "crash": (lambda mk: S.crash_only(mk), "hv"),
    "v2": (lambda mk: S.pl_doubling(mk, n=2048, seed=13, rounds=40, strategy=2, crash_at=30), "scamp"),
}
_VIEWS, _REF = {}, {}


def _views(key):
    """(the oracle's rows of a scenario, its seed), taken once"""
    if key not in _VIEWS:
        run, kind = RUNS[key]
        o = run(Oracle)[0]
        _VIEWS[key] = (o.nodes() if kind == "hv" else o.strategy_nodes(), int(o.cfg.seed))
        o.close()
    return _VIEWS[key]


def _want(key, sources, cap=0, root=None):
    k = (key, tuple(int(s) for s in sources), cap, root)
    if k not in _REF:
        views, seed = _views(key)
        _REF[k] = P.reference(views, seed, k[1], cap, root, RUNS[key][1])
    return _REF[k]


def _call(sim, sources, cap=0, root=None):
    """latency_metrics() of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    if hasattr(sim, "ranks"):
        ms = sim._threads("latency_metrics", list(sources), 64, 0, root, cap)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), "ranks disagree on the latency struct"
        return ms[0]
    return sim.latency_metrics(list(sources), tree_root=root, max_sweeps=cap)


def _check(make, key, calls):
    """a scenario on the engine, one call per (sources, cap, root), each
    against the reference over the oracle's rows"""
    wants = [_want(key, *c) for c in calls]
    g = RUNS[key][0](make)[0]
    try:
        for c, want in zip(calls, wants):
            P.compare(_call(g, *c), want)
    finally:
        g.close()
    return wants


def _seeded(n, k, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [int(x) for x in rng.choice(n, size=k, replace=False)]


ANCHORS = {0: (202, 513205, 3642, 10), 5: (202, 394997, 3103, 9), 202: (202, 452314, 3521, 11)}


@MAKES
def test_sources_64_5_1_0(make):
    """anchor A: 64 seeded sources, the three pinned ones among five, one, none"""
    s64 = _seeded(203, 64)
    calls = [(s64, 0, None), ([0, 5, 202, 100, 77], 0, None), ([202], 0, None), ([], 0, None), ([], 7, None)]
    w64, w5, w1, w0, _ = wants = _check(make, "a", calls)
    assert all((w["n_up"], w["links"], w["link_cost_sum"]) == (203, 790, 407750) for w in wants)
    assert w64["sources_live"] == 64 and w64["pairs_unreached"] == 0 and w64["truncated_mask"] == 0
    assert w64["sweeps"] == w64["last_sweep"].max() + 1
    for j, s in enumerate(ANCHORS):
        assert tuple(int(w5[k][j]) for k in P.SLOTS) == ANCHORS[s]
    assert tuple(int(w1[k][0]) for k in P.SLOTS) == ANCHORS[202] and w1["sweeps"] == 12 and w1["live_mask"] == 1
    assert w0["sources_live"] == 0 and w0["sweeps"] == 0 and not w0["lat"].any() and w0["links"] == 790


def test_xbot_churn_unreached_pairs():
    """512 nodes under X-BOT and churn: 8 of 511 nodes are out of source 0's reach"""
    w = _check(_gpu, "xbot", [([0], 0, None), (_seeded(512, 64), 0, None)])
    assert w[0]["reach"][0] == 503 and w[0]["pairs_unreached"] == 8 and w[0]["n_up"] == 512
    assert w[1]["pairs_unreached"] > 0 and w[1]["sources_live"] == 64


@MAKES
def test_dead_source_and_dead_targets(make):
    """crash_only: 963 of 1024 up; nodes 3, 20 and 1023 are down"""
    views = _views("crash")[0]
    assert not any(views["up"][i] for i in (3, 20, 1023)) and int(views["up"].sum()) == 963
    src = [0, 3, 1023, 17, 20] + _seeded(1024, 27, seed=5)
    w = _check(make, "crash", [(src, 0, None)])[0]
    dead = [j for j, s in enumerate(src) if not views["up"][s]]
    assert {1, 2, 4} <= set(dead) and w["sources_live"] == len(src) - len(dead)
    assert all(not (w["live_mask"] >> j) & 1 for j in dead) and not any(w[k][dead].any() for k in P.SLOTS)
    assert w["reach"][0] == 962 and w["n_up"] == 963 and w["pairs_unreached"] == 0


def test_sweep_cap():
    """the scenarios converge in 9 to 12 sweeps: a cap of 4 truncates every
    slot and gives the hop-bounded reference; a cap past the end gives the
    uncapped one"""
    s64 = _seeded(203, 64)
    w4, w99, w = _check(_gpu, "a", [(s64, 4, None), (s64, 99, None), (s64, 0, None)])
    assert w4["truncated_mask"] == (1 << 64) - 1 and w4["sweeps"] == 4 and (w4["last_sweep"] == 4).all()
    assert (w4["reach"] < 202).all() and w4["pairs_unreached"] > 0
    assert w99["truncated_mask"] == 0
    for k in P.SCALARS + P.ARRAYS:
        assert np.array_equal(w99[k], w[k]), k
    w4x = _check(_gpu, "xbot", [([0, 9], 4, None), ([0, 9], 1 << 20, None)])
    assert w4x[0]["truncated_mask"] == 3 and w4x[1]["truncated_mask"] == 0


def test_scamp_v2_csr_rows():
    """SCAMP v2 at 2048 nodes: the CSR path, rows of more than 8 and of more than 64 links"""
    nb = P.links_scamp(_views("v2")[0])
    assert sum(len(x) > 8 for x in nb.values()) > 8 and max(len(x) for x in nb.values()) > 64
    src = _seeded(2048, 16, seed=2)
    w = _check(_gpu, "v2", [(src, 0, None), (src[:3], 5, None)])
    assert w[0]["pairs_reached"] > 0 and w[0]["pairs_unreached"] > 0 and w[0]["sweeps"] > 8
    assert w[1]["truncated_mask"]


@pytest.mark.parametrize("make", [_vshards(3), _loop(2)], ids=["3-shards", "loopback-2"])
def test_scamp_v2_shards_and_ranks(make):
    _check(make, "v2", [(_seeded(2048, 5, seed=2), 0, None)])


# ---- the tree half
@MAKES
def test_tree_of_a_broadcasting_and_a_silent_root(make):
    """doubling(203) with three broadcasts from root 0; root 5 never broadcast:
    every node answers from its common eagers"""
    w0, w5, wc = _check(make, "a_bcast", [([0, 5], 0, 0), ([], 0, 5), ([7], 3, 0)])
    for w in (w0, w5):
        assert w["tree_root_live"] == 1 and w["tree_reached"] == 202 and w["tree_links"] == 908
        assert w["tree_lat_sum_both"] <= w["overlay_lat_sum_both"] and w["faster"] > 0
    assert w0["overlay_reached"] == w0["reach"][0] and w0["overlay_lat_sum_both"] == w0["lat_sum"][0]
    assert w5["sources_live"] == 0 and w5["overlay_lat_sum_both"] == w0["lat_sum"][1]
    assert wc["tree_truncated"] == 1 and wc["tree_sweeps"] == 3 and wc["truncated_mask"] == 1


def test_tree_of_config_a():
    w = _check(_gpu, "config_a", [([0], 0, 0)])[0]
    assert (w["n_up"], w["tree_reached"], w["overlay_reached"], w["faster"]) == (32, 31, 31, 5)


@MAKES
def test_tree_of_a_dead_root(make):
    w = _check(make, "crash", [([0], 0, 3), ([], 0, 1023), ([], 0, 0)])
    for dead in w[:2]:
        assert not any(dead[k] for k in P.TREE)
    assert w[0]["reach"][0] == 962 and w[1]["links"] == w[2]["links"] and w[2]["tree_reached"] == 962


@MAKES
def test_tree_under_xbot_is_slower_and_faster(make):
    """xbot_churn(512, 80 rounds): the one scenario here whose reference has
    both a node the tree reaches later than the overlay's cheapest path
    (slower = 1) and nodes it reaches sooner, over eager links to non-members
    (faster = 131)"""
    w = _check(make, "xbot80", [([0], 0, 0)])[0]
    assert (w["slower"], w["faster"]) == (1, 131) and w["tree_reached"] > w["overlay_reached"] == w["both_reached"]


# ---- the measured alternatives give the same struct
@pytest.mark.parametrize("push,cell", [("list", ""), ("", "cell"), ("list", "cell")])
def test_push_list_and_cell_array(push, cell):
    """a fresh process a setting: PSIM_LAT_PUSH=list (a wave a node of the
    compacted frontier) and PSIM_LAT_CELL=cell (the torus cells in an array)"""
    env = dict(os.environ, PSIM_LAT_PUSH=push, PSIM_LAT_CELL=cell)
    calls = [("a", _seeded(203, 64), 0, None), ("a", _seeded(203, 64), 4, None), ("xbot80", [0, 9], 0, 0)]
    for c in calls:
        r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_latency_run.py"), json.dumps(c)], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        P.compare(json.loads(r.stdout.strip().splitlines()[-1]), _want(*c))


# ---- empty handles
def test_no_node_ever_started():
    for n in (300, 37):
        s = _gpu(default_config(n_nodes=n, seed=1))
        for rounds in (0, 2):
            if rounds:
                s.step(rounds)
            for src, root in (([], None), ([0, n - 1, 17], None), ([5], 0)):
                m = s.latency_metrics(src, tree_root=root)
                assert all(not np.any(v) for v in m.values()), m
        s.close()


# ---- arguments and errors, in the header's order
def _errors(hv, scamp, full, noplum, n):
    """every error path on handles of the four kinds; `call(h, ...)` returns the code"""
    def rc(h, src, root=None, cap=0):
        try:
            _call(h, src, cap, root)
        except SimError as e:
            return e.rc
        return 0
    assert rc(hv, list(range(65))) == -1                                # PSIM_EINVAL: 65 sources
    assert rc(hv, list(range(64)) + [n]) == -1                          # ... before the range
    assert rc(hv, [n]) == -5                                            # PSIM_ERANGE: a source == n_nodes
    assert rc(hv, [0, 1], root=n) == -5                                 # the root == n_nodes
    assert rc(hv, [1, 2, 1]) == -1                                      # a repeated source
    assert rc(hv, [1, n, 1]) == -5                                      # ... after the range
    assert rc(hv, list(range(64)), root=n - 1, cap=1 << 30) == 0        # 64 sources, any cap, the last id a root
    assert rc(full, [1]) == -7 and rc(full, []) == -7                   # PSIM_EUNSUPPORTED: full membership
    assert rc(full, [n]) == -7                                          # ... before the range
    assert rc(scamp, [1]) == 0 and rc(scamp, [1], root=0) == -7         # a root on a pluggable handle
    assert rc(scamp, [n], root=0) == -7
    assert rc(noplum, [1]) == 0 and rc(noplum, [1], root=0) == -7       # ... with plumtree = 0
    assert rc(noplum, [], root=n) == -7


def _four(make, n=64):
    return [make(default_config(n_nodes=n, seed=1, **kw))
            for kw in (dict(), dict(manager=1, strategy=2), dict(manager=1, strategy=0), dict(plumtree=0))]


def test_error_paths():
    from partisan_amd import HostSim, _abi
    hs = _four(_gpu)
    hv = hs[0]
    fn, m = hv._extra["get_latency_metrics"], _abi.PsimLatencyMetrics()
    src = (np.arange(70, dtype=np.uint32)).ctypes.data_as(_abi._P32)
    assert fn(hv._h, None, 0, NONE, 0, None) == -1                      # PSIM_EINVAL: null out
    assert fn(None, None, 0, NONE, 0, m) == -1                          # null handle
    assert fn(hv._h, None, 3, NONE, 0, m) == -1                         # null sources, n_sources > 0
    assert fn(hv._h, src, 65, NONE, 0, m) == -1                         # 65 sources
    assert fn(hv._h, src, 64, NONE, 0, m) == 0 and fn(hv._h, None, 0, NONE, 0, m) == 0
    assert fn(hv._h, src, 70, 5, 0, m) == -1 and fn(hs[2]._h, None, 3, NONE, 0, m) == -1   # EINVAL comes first
    _errors(*hs, 64)
    x = _gpu(default_config(n_nodes=64, seed=1, manager=2, xbot_period=10))
    assert x.latency_metrics([1, 2], tree_root=0)["n_up"] == 0          # X-BOT: both halves supported
    for h in hs + [x]:
        h.close()
    # a host-exchange handle, the only kind that can hold a round open: it
    # answers unsupported with and without one, so PSIM_ESTATE cannot be had
    # through the ABI (as with psim_get_graph_metrics)
    host = HostSim(default_config(n_nodes=64, seed=1), 16, 48)
    for opened in (False, True):
        if opened:
            host.emit()
        with pytest.raises(SimError) as e:
            host.latency_metrics([20])
        assert e.value.rc == -7
    host.absorb(np.zeros((0, 16), np.uint32))
    host.close()


def test_error_paths_on_loopback_ranks():
    """every rank refuses with the same code (LoopbackRanks._threads raises
    the first rank's; _all checks that all agree)"""
    hs = _four(_loop(2))
    _errors(*hs, 64)
    for h, bad in ((hs[0], [64]), (hs[0], [3, 3]), (hs[2], [1])):
        with pytest.raises(SimError):
            h._all("latency_metrics", bad)
    for h in hs:
        h.close()


# ---- read-only
class _CallAt:
    """a handle that takes its latency struct once, before the step of round `at`"""
    run_schedule = _Driver.run_schedule

    def __init__(self, sim, at):
        self._sim, self._at, self.seen = sim, at, []

    def __getattr__(self, name):
        return getattr(self._sim, name)

    def step(self, k=1):
        if self._sim.round == self._at and not self.seen:
            self.seen.append(self._sim.latency_metrics(seed=3, tree_root=0))
        return self._sim.step(k)


def test_read_only():
    """a call, tree half included, in the middle of xbot_churn changes no later round"""
    o, ost = RUNS["xbot"][0](Oracle)
    box = []

    def make(cfg):
        box.append(_CallAt(_gpu(cfg), 45))
        return box[0]
    g, gst = RUNS["xbot"][0](make)
    assert g.seen and g.seen[0]["n_up"] > 0 and g.seen[0]["pairs_reached"] > 0 and g.seen[0]["tree_reached"] > 0
    S.compare_stats(gst, ost)
    S.compare_nodes(g.nodes(), o.nodes())
    g.close(); o.close()


# ---- the report
def test_latency_report(tmp_path):
    from partisan_amd import latency_report as Q
    from partisan_amd import workloads as W
    from partisan_amd.tree_report import complete_broadcast
    n, seed, rounds, period, bc = 256, 31, 25, 5, 2
    r = subprocess.run([sys.executable, "-m", "partisan_amd.latency_report", "--nodes", str(n), "--seed", str(seed),
                        "--rounds", str(rounds), "--xbot-period", str(period), "--broadcasts", str(bc),
                        "--json", str(tmp_path / "r.json"), "--out", str(tmp_path / "r.md")],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads((tmp_path / "r.json").read_text())
    md = (tmp_path / "r.md").read_text()
    assert md in r.stdout
    # the table parses: a row a label, three numbers each, the JSON's
    cells = {c[1].strip(): [x.strip() for x in c[2:5]] for c in (line.split("|") for line in md.splitlines())
             if len(c) == 6 and c[1].strip() and not set(c[1].strip()) <= set("-")}
    for label, key, fmt in Q.ROWS + Q.TREE_ROWS:
        a, b = rep["hyparview"][key], rep["xbot"][key]
        assert cells[label] == [f"{a:{fmt}}", f"{b:{fmt}}", f"{(b / a if a else 0.0):.4f}"], label
    # its numbers are those of direct calls on handles built the same way
    sched = W.doubling_join(n, seed)
    for name, kw in (("hyparview", {}), ("xbot", dict(manager=2, xbot_period=period))):
        s = _gpu(default_config(n_nodes=n, seed=seed, **kw))
        s.run_schedule(sched, sched[-1][0] + 1 + rounds)
        want = Q.columns(s.latency_metrics(seed=seed), s.graph_metrics(seed=seed))
        for k in range(1, bc + 1):
            complete_broadcast(s, 0, k)
        want.update(Q.tree_columns(s.latency_metrics([], tree_root=0)))
        s.close()
        got = rep[name]
        assert {k: got[k] for k in want} == want, name
        assert got["n_up"] == n and got["sources"] == 64 and got["tree_reached"] > 0 and got["latency_mean"] > 0
    assert rep["xbot"]["link_cost_mean"] < rep["hyparview"]["link_cost_mean"]
