"""The cases of tests/_config_cases.py on the oracle alone, so that a green
tests/test_gpu_config_matrix.py cannot have compared two runs in which the
case's key did nothing: every case differs from its default twin (the named
exemptions apart), still reaches what it is there for, counts no overflow but
the kind its table entry names, and stays cheap."""
import functools
import time

import numpy as np
import pytest

import _config_cases as CC
from _oracle import Oracle
from partisan_amd import _abi

T_MAX = 2.0     # seconds of oracle time a case may take


@functools.lru_cache(maxsize=None)
def _run(name):
    t = time.perf_counter()
    sim, st, rest = CC.run(Oracle, name)
    return sim, st, rest, time.perf_counter() - t


@functools.lru_cache(maxsize=None)
def _twin_digests(scn, args):
    """the default twin's digests, once per (scenario, arguments)"""
    c = CC.Case(scn, dict(args), {}, None, None)
    out = CC._scenario(c.scn)(Oracle, **c.args)
    out[0].close()
    return out[1]["digest"].copy(), out[1]["emitted"].sum(0)


def _twin(name):
    c = CC.CASES[name]
    return _twin_digests(c.scn, tuple(sorted(c.args.items())))


def _em(st):
    return [int(x) for x in st["emitted"].sum(0)]


@pytest.mark.parametrize("name", [k for k, c in CC.CASES.items() if c.cfg])
def test_differs_from_the_default_run(name):
    _, st, _, _ = _run(name)
    same = np.array_equal(st["digest"], _twin(name)[0])
    if name in CC.NOT_LIVE:
        # (an exemption that no longer holds should leave the list)
        assert same, f"{name} is live now: take it off NOT_LIVE ({CC.NOT_LIVE[name]})"
    else:
        assert not same, f"{name}: its overrides {CC.CASES[name].cfg} change nothing"


def test_exemptions_are_cases():
    assert set(CC.NOT_LIVE) <= set(CC.CASES)
    assert set(CC.OTHER_PATHS) <= set(CC.CASES)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_overflow_and_runtime(name):
    _, st, _, dt = _run(name)
    by = [int(x) for x in st["overflow_by"].sum(0)]
    print(name, "overflow_by", by, f"{dt:.3f} s", "messages", sum(_em(st)))
    assert CC.allowed_overflow(name, st), by
    for k in CC.CASES[name].ovf:
        assert by[k] > 0, f"{name} no longer counts the overflow it is kept for"
    assert int(st["overflow"].sum()) == sum(by)
    assert dt < T_MAX


# ---- reach: the assertion that says why the case exists
def test_reach_lazy_tick_period():
    em, base = _em(_run("lazy3")[1]), _twin("lazy3")[1]
    assert 0 < em[11] < 0.6 * base[11]               # a tick every third round: about half the IHAVEs
    em = _em(_run("lazy0")[1])
    assert em[11] == 0 and em[13] == 0 and em[9] > 0   # no tick: no IHAVE, so no GRAFT
    assert _em(_run("lazy7_shuf3")[1])[11] > 0


def test_reach_plumtree_off():
    for name in ("plumtree0", "batch_plumtree0"):
        em = _em(_run(name)[1])
        assert em[9:14] == [0] * 5 and em[7] > 0
        assert sum(_twin(name)[1][9:14]) > 0


def test_reach_shuffle_period():
    em = _em(_run("shuf0")[1])
    assert em[7] == 0 and em[8] == 0
    assert _em(_run("shuf1")[1])[7] > 5 * _twin("shuf1")[1][7]


def test_reach_promotion():
    assert _em(_run("promo1_min5")[1])[4] > 4 * _twin("promo1_min5")[1][4]    # NEIGHBOR_REQUEST
    assert _em(_run("nopromo")[1])[4] < _twin("nopromo")[1][4]


@pytest.mark.parametrize("name", ["act8_min8", "act2", "act3", "pas1_act2", "xbot_p10_lazy3_act4"])
def test_reach_active_size(name):
    sim = _run(name)[0]
    v = sim.nodes()
    assert int(v["act_n"].max()) == CC.CASES[name].cfg["max_active_size"]
    if "max_passive_size" in CC.CASES[name].cfg:
        assert int(v["pas_n"].max()) == CC.CASES[name].cfg["max_passive_size"]


def test_reach_walk_lengths():
    """arwl = 0: a FORWARD_JOIN stops at its first receiver, so there are
    few; prwl > arwl and the lengths between move the count"""
    base = _twin("arwl0")[1][1]
    a0, a1, a3 = (_em(_run(k)[1])[1] for k in ("arwl0", "arwl1_prwl3", "prwl_gt"))
    assert 0 < a0 < a1 < a3 < base


@pytest.mark.parametrize("name", ["quiet_lazy2", "quiet_lazy5", "quiet_lazy3_act8"])
def test_reach_quiet_nodes(name):
    """the node view has no flags word: quiet nodes show in the stats.  Under
    the partition (rounds 60-67) nodes hold outstanding entries they cannot
    push -- more failed sends a round than there are nodes -- while in a round
    between two ticks most nodes do not run at all; the heal then wakes them"""
    _, st, _, _ = _run(name)
    n = CC.CASES[name].args["n"]
    em = st["emitted"].sum(1)
    assert int(st["send_fail"][60:68].max()) > n
    assert int(st["nodes_processed"][60:68].min()) < n // 2
    assert int(em[68]) > 4 * int(em[67])


def test_reach_quiet_without_ticks():
    sim, st, _, _ = _run("quiet_lazy0")
    assert int(sim.nodes()["pt_out_n"].max()) > 64          # past one 64-entry register, never pushed
    assert _em(st)[11] == 0


def test_reach_xbot():
    assert sum(_em(_run("xbot_p1")[1])[16:22]) > 10 * sum(_twin("xbot_p1")[1][16:22])
    assert sum(_em(_run("xbot_p0")[1])[16:22]) == 0
    assert sum(_em(_run("xbot_p10_lazy3_act4")[1])[16:22]) > 0


def test_reach_small_overlays():
    _, st, _, _ = _run("hv_n1")
    assert sum(_em(st)) == 0 and int(st["nodes_processed"].sum()) == 21
    assert sum(_em(_run("hv_n2")[1])) == 78
    for name in CC.CASES:
        if name.endswith("_one_node"):
            _, st, _, _ = _run(name)
            assert sum(_em(st)) == 0 and (st["nodes_up"] == 1).all()
    for n in CC.SMALL_PL:
        for p in CC.STRATEGY_NAMES.values():
            assert sum(_em(_run(f"{p}_n{n}")[1])) > 0


def test_reach_scamp_view_at_the_cap():
    sim = _run("v1_pi3")[0]
    assert int(sim.strategy_nodes()["view_n"].max()) == _abi.SVIEW_CAP


def test_reach_periodic_interval():
    for p in ("v1", "v2"):
        assert _em(_run(f"{p}_pi0")[1])[4] == 0                # no periodic: no ping
        assert _em(_run(f"{p}_pi1")[1])[4] > 5 * _twin(f"{p}_pi1")[1][4]


def test_reach_scamp_c_picks():
    """pl_restart_contact: node 7's join draws from a view of many members"""
    for p in ("v1", "v2"):
        c3, c64, c5 = _em(_run(f"{p}_c3_restart")[1])[3], _em(_run(f"{p}_c64_restart")[1])[3], \
            _twin(f"{p}_c3_restart")[1][3]
        print(p, "forward_subscriptions with c = 3, 5, 64:", c3, c5, c64)
        assert len({c3, c5, c64}) == 3


@pytest.mark.parametrize("name", ["event_edges", "event_edges_lazy3", "event_edges_v2"])
def test_reach_event_edges(name):
    _, st, (outcomes,), _ = _run(name)
    refused = [(k, o) for k, o in enumerate(outcomes) if o[1] != 0]
    if CC.CASES[name].args.get("bcast", True):
        # the second broadcast of rounds 52 and 53
        assert [o for _, o in refused] == [("broadcast", -1)] * 2, refused
        calls = [o[0] for o in outcomes]
        for k, _ in refused:
            assert calls[k - 1] == "broadcast" and outcomes[k - 1][1] == 0
        assert _em(st)[11] > 0                                 # IHAVEs in flight among the events
    else:
        assert not refused
    assert int(st["nodes_up"][56]) == 1 and int(st["nodes_up"][99]) == 1021
    assert int(st["nodes_up"][44]) == 1021 - 20 and int(st["nodes_up"][54]) == 1021 - 7
