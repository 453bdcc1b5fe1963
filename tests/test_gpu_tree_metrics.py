"""psim_get_tree_metrics on the GPU: every field of the struct against the
reference (tests/_tree_metrics.py) applied to the CPU oracle's rows of the same
scenario -- the expected values never come from the engine.  HyParView and
X-BOT; one shard, virtual shards and loopback ranks; roots with and without
slots, both-form links, dead peers, dead and isolated roots, a level cap.
Each test first asserts on the reference that its scenario shows what it is
there for."""
import numpy as np
import pytest

import _scenarios as S
import _tree_metrics as R
from _oracle import Oracle
from partisan_amd.sim import SimError, default_config

pytestmark = pytest.mark.gpu


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

SCENARIOS = {
    "config_a": lambda mk: S.config_a(mk),
    "d203": lambda mk: S.doubling(mk, n=203, seed=3, rounds=60, bcast_period=10, bcast_first=30),
    "roots4": lambda mk: S.multi_root(mk, n=512, seed=17, rounds=100),
    "roots6": lambda mk: S.multi_root(mk, n=512, seed=17, rounds=100, roots=6),
    "roots4_churn": lambda mk: S.multi_root(mk, n=512, seed=17, rounds=100, churn=True),
    "crash_only": lambda mk: S.crash_only(mk, rounds=42),
    "crash_revive": lambda mk: S.crash_revive(mk, rounds=53),
    "xbot_churn": lambda mk: S.xbot_churn(mk, n=512, rounds=80),
}


def _call(sim, root, max_levels=0):
    """tree_metrics() of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    if hasattr(sim, "ranks"):
        ms = sim._threads("tree_metrics", root, max_levels)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), "ranks disagree on the tree metrics"
        return ms[0]
    return sim.tree_metrics(root, max_levels=max_levels)


_ORACLE = {}


def _oracle(key):
    """(the oracle's rows, what the scenario returns past the handle and the
    stats: the roots / the victims), taken once"""
    if key not in _ORACLE:
        r = SCENARIOS[key](Oracle)
        _ORACLE[key] = (r[0].nodes(), r[2] if len(r) > 2 else None)
        r[0].close()
    return _ORACLE[key]


_REF = {}


def _want(key, root, max_levels=0):
    k = (key, int(root), max_levels)
    if k not in _REF:
        _REF[k] = R.reference(_oracle(key)[0], int(root), max_levels)
    return _REF[k]


def _check(make, key, roots, caps=(0,)):
    """the scenario on the engine, every (root, cap) against the reference;
    the overlay's half against the engine's own graph_metrics"""
    g = SCENARIOS[key](make)[0]
    try:
        for root in roots:
            for cap in caps:
                got = _call(g, int(root), cap)
                R.compare(got, _want(key, root, cap))
            if not hasattr(g, "ranks"):
                assert got["overlay_reached"] == g.graph_metrics([int(root)], max_levels=caps[-1])["reach"][0]
    finally:
        g.close()


@MAKES
def test_config_a(make):
    w = _want("config_a", 0)
    assert w["n_up"] == 32 and w["root_live"] == 1 and w["slot_nodes"] > 0 and w["unreached"] == 0
    _check(make, "config_a", [0])


@MAKES
def test_broadcasting_and_silent_root(make):
    """root 0 broadcast three times; root 5 never did: every node answers
    from its common set"""
    w0, w5 = _want("d203", 0), _want("d203", 5)
    assert w0["slot_nodes"] > 0 and w0["unreached"] == 0 and w0["reached"] == 202
    assert w5["slot_nodes"] == 0 and w5["lazy_links"] == 0 and w5["unreached"] == 0 and w5["eager_links"] > 0
    _check(make, "d203", [0, 5])


@MAKES
def test_four_roots_every_node_holds_every_slot(make):
    roots = _oracle("roots4")[1]
    assert len(roots) == 4
    for r in roots:
        w = _want("roots4", r)
        assert w["slot_nodes"] == w["n_up"] == 512
        assert 0 < w["both_links"] <= w["lazy_links"] and w["eager_both_forms"] > 0
    _check(make, "roots4", roots)


@MAKES
def test_six_roots_slots_and_common_sets_mixed(make):
    roots = _oracle("roots6")[1]
    assert len(roots) == 6
    for r in roots:
        w = _want("roots6", r)
        assert 0 < w["slot_nodes"] < w["n_up"]
    _check(make, "roots6", roots)


@MAKES
def test_churn_leaves_lazy_nonmembers(make):
    roots = _oracle("roots4_churn")[1]
    assert all(_want("roots4_churn", r)["lazy_nonmember"] > 0 for r in roots)
    _check(make, "roots4_churn", roots)


@MAKES
def test_crashes_leave_dead_entries_and_a_dead_root(make):
    victims = _oracle("crash_only")[1]
    assert 3 in victims
    w0, w3 = _want("crash_only", 0), _want("crash_only", 3)
    assert w0["eager_dead"] > 0 and w0["n_up"] == 1024 - len(victims) < 1024 and w0["root_live"] == 1
    assert w3["root_live"] == 0
    bfs = ("depth", "depth_sum", "depth_max", "reached", "unreached", "links_from_reached", "levels", "truncated",
           "overlay_reached", "both_reached", "depth_sum_both", "dist_sum_both", "deeper", "shallower")
    assert all(not np.any(w3[k]) for k in bfs)
    # nobody ever broadcast: both roots are answered from the common sets
    assert all(np.array_equal(w3[k], w0[k]) for k in R.DEGREE_FIELDS)
    _check(make, "crash_only", [0, 3])


@MAKES
def test_revived_nodes_are_unreached_and_reach_nobody(make):
    victims = _oracle("crash_revive")[1]
    assert 5 in victims
    w0, w5 = _want("crash_revive", 0), _want("crash_revive", 5)
    assert w0["unreached"] > 0 and w0["reached"] > 0
    assert w5["root_live"] == 1 and w5["reached"] == 0 and w5["unreached"] == w5["n_up"] - 1
    _check(make, "crash_revive", [0, 5])


@MAKES
def test_xbot_churn(make):
    w = _want("xbot_churn", 0)
    assert 0 < w["slot_nodes"] < w["n_up"] and w["unreached"] > 0
    _check(make, "xbot_churn", [0])


def test_wave_per_node_layout(monkeypatch):
    """PSIM_TREE_LANES=64, the A/B layout of the row kernel: the same struct"""
    monkeypatch.setenv("PSIM_TREE_LANES", "64")
    _check(_gpu, "roots4", _oracle("roots4")[1])
    _check(_vshards(3), "xbot_churn", [0])


def test_level_cap():
    w3, w = _want("d203", 0, 3), _want("d203", 0)
    assert w3["truncated"] == 1 and w3["levels"] == 3 and not w3["depth"][4:].any() and w3["unreached"] > 0
    assert w["truncated"] == 0 and 3 < w["depth_max"] < 60
    g = SCENARIOS["d203"](_gpu)[0]
    try:
        got = g.tree_metrics(0, max_levels=3)
        R.compare(got, w3)
        assert got["truncated"] == 1 and not got["depth"][4:].any()
        # a cap past the depth equals no cap; a cap past the largest is clamped to it
        R.compare(g.tree_metrics(0, max_levels=60), w)
        R.compare(g.tree_metrics(0, max_levels=1 << 20), w)
        R.compare(_want("d203", 0, 60), w)
    finally:
        g.close()


@pytest.mark.parametrize("make", [_gpu, _vshards(3)], ids=["gpu", "3-shards"])
def test_read_only(make):
    """calls change no byte of the state and no later round"""
    a, b = SCENARIOS["d203"](make)[0], SCENARIOS["d203"](make)[0]
    try:
        before = a.snapshot()
        for root, cap in ((0, 0), (5, 0), (0, 3), (202, 0)):
            a.tree_metrics(root, max_levels=cap)
        assert a.snapshot() == before
        sa, sb = a.step(10), b.step(10)
        S.compare_stats(sa, sb)
        S.compare_nodes(a.nodes(), b.nodes())
        R.compare(a.tree_metrics(0), b.tree_metrics(0))
    finally:
        a.close(); b.close()


def _rc(fn, *a):
    with pytest.raises(SimError) as e:
        fn(*a)
    return e.value.rc


def test_error_paths():
    from partisan_amd import HostSim, _abi
    hv = _gpu(default_config(n_nodes=64, seed=1))
    fn, m = hv._extra["get_tree_metrics"], _abi.PsimTreeMetrics()
    assert fn(hv._h, 0, 0, None) == -1                                # PSIM_EINVAL: null out
    assert fn(None, 0, 0, m) == -1                                    # null handle
    assert _rc(hv.tree_metrics, 64) == -5                             # PSIM_ERANGE: root == n_nodes
    assert hv.tree_metrics(63)["root_live"] == 0                      # (nobody started: legal, all zero)
    hv.close()
    for kw in (dict(manager=1, strategy=2), dict(manager=1, strategy=0), dict(plumtree=0),
               dict(manager=2, plumtree=0)):
        s = _gpu(default_config(n_nodes=64, seed=1, **kw))
        assert _rc(s.tree_metrics, 1) == -7, kw                       # PSIM_EUNSUPPORTED
        s.close()
    host = HostSim(default_config(n_nodes=64, seed=1), 16, 48)
    assert _rc(host.tree_metrics, 20) == -7
    host.close()


def test_error_paths_on_ranks():
    """every rank refuses with the same code, before any collective"""
    for kw, root, rc in ((dict(), 64, -5), (dict(plumtree=0), 1, -7)):
        lb = _loop(2)(default_config(n_nodes=64, seed=1, **kw))
        try:
            assert [_rc(s.tree_metrics, root) for s in lb.ranks] == [rc, rc]
        finally:
            lb.close()


def test_no_node_ever_started():
    for kw in (dict(), dict(manager=2)):
        s = _gpu(default_config(n_nodes=300, seed=1, **kw))
        for rounds in (0, 2):
            if rounds:
                s.step(rounds)
            for root in (0, 299):
                m = s.tree_metrics(root)
                assert all(not np.any(v) for v in m.values()), m
        s.close()
