"""The host boundary (psim_round_emit / psim_get_outbound / psim_round_absorb):
the engine simulates part of the id space on a host-exchange handle and
oracle shards play the outside nodes on the rest (tests/_hybrid.py), records
crossing through the ABI.  Each round the engine's outbound list must equal,
word for word, what the same parties exchange when oracle shards play the
engine's range too; at the end the summed stats and the engine's node state
must equal the unsharded oracle's, with no overflow.  The shapes: an outside
side above only, below only, both; an uneven last range; sixteen outside
nodes beside 1008 simulated (the mixed-cluster shape); X-BOT's records and
the exchange lists' long ones; several Plumtree roots on both sides; SCAMP
v1 and v2, leave/0 across the boundary."""
import functools

import numpy as np
import pytest

import _scenarios as S
from _hybrid import Hybrid
from _oracle import Oracle
from partisan_amd import _abi, _lib, wire
from partisan_amd.sim import SimError, default_config

pytestmark = pytest.mark.gpu

CHURN = ("churn_partition", dict(n=1024, rounds=110))
SCENARIOS = {
    "above": (CHURN, 2, (0, 1)),
    "below": (CHURN, 2, (1, 2)),
    "uneven": (("churn_partition", dict(n=1000, rounds=110)), 8, (0, 7)),
    "mixed_cluster": (CHURN, 64, (0, 63)),
    "xbot": (("xbot_churn", dict(n=1024, rounds=110)), 4, (1, 3)),
    "multi_root": (("multi_root", dict(n=1024, rounds=100, churn=True)), 4, (0, 2)),
    "scamp_v1": (("pl_doubling", dict(n=512, seed=3, rounds=60, strategy=1, crash_at=30, part_at=45)), 4, (1, 3)),
    "scamp_v2": (("pl_doubling", dict(n=512, seed=3, rounds=60, strategy=2, crash_at=30, part_at=45)), 4, (1, 3)),
    "scamp_v2_leave": (("pl_doubling", dict(n=512, seed=3, rounds=60, strategy=2, leave=True, crash_at=30)), 2, (0, 1)),
}


def _key(scn):
    return scn[0], tuple(sorted(scn[1].items()))


@functools.lru_cache(maxsize=None)
def _unsharded(key):
    """the reference: the unsharded oracle's (handle, stats) of a scenario"""
    name, kw = key
    out = getattr(S, name)(Oracle, **dict(kw))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def _all_oracle(key, world, ranks):
    """the expected exchange: the same parties, the engine's ranks played by
    oracle shards -- its per-round trace; the run itself equals the reference"""
    name, kw = key
    out = getattr(S, name)(lambda cfg: Hybrid(cfg, world, ranks, engine=False), **dict(kw))
    S.compare_stats(out[1], _unsharded(key)[1])
    assert out[0].n_out > 0 or world == 1
    trace = out[0].trace
    out[0].close()
    return trace


def _pluggable(key):
    return key[0] == "pl_doubling"


def _hybrid(name, **kw):
    scn, world, ranks = SCENARIOS[name]
    key = _key(scn)
    expect = _all_oracle(key, world, ranks)
    out = getattr(S, scn[0])(lambda cfg: Hybrid(cfg, world, ranks, expect=expect, **kw), **scn[1])
    return out[0], out[1], key


def _check_final(hy, st, key):
    full, fst = _unsharded(key)
    S.compare_stats(st, fst)
    assert int(st["overflow"].sum()) == 0
    e = hy.engine
    if _pluggable(key):
        S.compare_nodes(e.strategy_nodes(), full.strategy_nodes(e.lo, e.hi - e.lo))
    else:
        S.compare_nodes(e.nodes(), full.nodes(e.lo, e.hi - e.lo))


@pytest.mark.parametrize("name", [k for k in SCENARIOS if k != "xbot"])
def test_hybrid_matches_unsharded_oracle(name):
    hy, st, key = _hybrid(name)
    try:
        _check_final(hy, st, key)
        assert hy.n_out > 0 and hy.n_in > 0
        # psim_get_exchange_stats: outbound and absorbed records, 64 B each
        assert hy.engine.exchange_stats() == (hy.n_out + hy.n_in, 64 * (hy.n_out + hy.n_in))
    finally:
        hy.close()


@functools.lru_cache(maxsize=None)
def _xbot_run():
    """shape 5, once: its outbound records kept for the wire round trip"""
    kept = []
    hy, st, key = _hybrid("xbot", on_outbound=lambda r, box: kept.append(box.copy()))
    try:
        _check_final(hy, st, key)
    finally:
        hy.close()
    return np.concatenate(kept)


def test_hybrid_xbot_both_sides():
    out = _xbot_run()
    types = set((out[:, 2] & 0xFF).tolist())
    assert types & {16, 17, 18, 19, 20, 21}, "no X-BOT record crossed the boundary"
    assert ((out[:, 2] >> 16) & 0xFF).any(), "no long record crossed the boundary"
    assert (out[:, 0] < 256).any() and (out[:, 0] >= 768).any()


def test_outbound_records_round_trip_the_wire():
    """encode then decode (dst passed in) gives the record back, seq zeroed;
    an IHAVE of a retired id has no frame (tests/test_wire.py skips it too)"""
    nm = wire.names(prefix="n", host="127.0.0.1", ip_base=(10 << 24), port=9090)
    k = 0
    for r in _xbot_run():
        if (r[2] & 0xFF) == 11 and r[6] == 0xFFFFFFFF:
            continue
        got, _ = wire.decode(wire.encode(r, nm), nm, int(r[0]))
        want = r.copy()
        want[3] = 0
        assert np.array_equal(got, want), (r, got)
        k += 1
    assert k > 1000


def test_snapshot_restore_between_rounds():
    """shape 1; after round 60 the engine's state moves, by psim_snapshot and
    psim_restore, into a fresh handle of the same range"""
    hy, st, key = _hybrid("above", resume_at=60)
    try:
        assert hy.resumed
        _check_final(hy, st, key)
    finally:
        hy.close()


def _raises(code, fn, *a):
    with pytest.raises(SimError) as e:
        fn(*a)
    assert code in str(e.value), e.value


def test_states_and_errors():
    """every rejection is host-side validation, before any device work"""
    from partisan_amd.sim import HostSim

    n = 1024
    with pytest.raises(SimError, match="unsupported"):
        HostSim(default_config(n_nodes=n, manager=1, strategy=0), 0, 512)
    with pytest.raises(SimError, match="invalid argument"):
        HostSim(default_config(n_nodes=n), 512, n + 1)
    with pytest.raises(SimError, match="invalid argument"):
        HostSim(default_config(n_nodes=n, n_shards=2), 0, 512)
    e = HostSim(default_config(n_nodes=n), 0, 512)
    none = np.zeros((0, 16), np.uint32)
    _raises("unsupported", e.step, 1)
    _raises("invalid state", e.absorb, none)
    _raises("invalid state", e.outbound)
    _raises("unsupported", e.histograms)
    e.emit()
    _raises("invalid state", e.emit)
    _raises("invalid state", e.nodes)
    _raises("invalid state", e.snapshot)
    e.crash(np.array([3], np.uint32))                  # (queues for the next emit)
    assert e.outbound().shape == (0, 16)
    e.absorb(none)
    assert e.round == 1 and e.nodes().shape == (512,)
    e.close()
    p = HostSim(default_config(n_nodes=n, manager=1, strategy=2), 0, 512)
    _raises("unsupported", p.leave_node, np.array([1], np.uint32), np.array([2], np.uint32))
    _raises("unsupported", p.strategy_histograms)
    p.close()
    # a plain handle has no boundary
    from partisan_amd import Simulator
    s = Simulator(default_config(n_nodes=64))
    emit = _abi.bind(_lib.load(), "psim_", _abi.HOST_BOUNDARY)["round_emit"]
    _raises("unsupported", lambda: s._check(emit(s._h), "round_emit"))
    s.close()

    tried = []

    def probe(eng, recs):
        assert len(recs) > 2
        bad = recs.copy()
        bad[0, 0] = 600                                # a dst outside [0, 512)
        _raises("out of range", eng.absorb, bad)
        bad = recs.copy()
        bad[1, 2] = (bad[1, 2] & 0xFF00FFFF) | (1 << 16)
        bad[1, 8] = n                                  # ex[0] = n
        _raises("out of range", eng.absorb, bad)
        bad = recs.copy()
        bad[2, 1], bad[2, 3] = bad[0, 1], bad[0, 3]    # (src, seq) twice
        _raises("invalid argument", eng.absorb, bad)
        _raises("invalid state", eng.nodes)            # still open
        tried.append(len(recs))

    hy, st, key = _hybrid("above", probes={50: probe})
    try:
        assert tried
        _check_final(hy, st, key)
    finally:
        hy.close()


def test_one_party_diagnostic():
    """lo = 0, hi = n: nothing is outside; emit and an empty absorb a round"""
    scn = SCENARIOS["above"][0]
    key = _key(scn)
    hy, st = S.churn_partition(lambda cfg: Hybrid(cfg, 1, (0, 1)), **scn[1])
    try:
        assert hy.n_out == 0 and hy.n_in == 0 and all(len(o) == 0 for o, _ in hy.trace)
        _check_final(hy, st, key)
    finally:
        hy.close()
