"""The config matrix (tests/_config_cases.py) on the GPU against the oracle,
bit for bit: config keys off their defaults (lazy_tick_period, plumtree,
the promotion and shuffle timers, view and walk sizes, X-BOT's period, the
pluggable manager's periodic_interval, scamp_c and fanout), overlays of one
to five, 63 and 65 nodes, and event calls at their edges.  Every round's
stats (overflow_by and digest among them), the final node state, and for
HyParView handles the histograms and the tracked delivery must be equal.
The same over three virtual shards and as a host-exchange handle for the
cases of CC.OTHER_PATHS.  tests/test_config_cases.py shows on the oracle
alone that each case's key does something."""
import functools

import numpy as np
import pytest

import _config_cases as CC
import _scenarios as S
from _hybrid import Hybrid
from _oracle import Oracle

pytestmark = pytest.mark.gpu


def _gpu(cfg):
    from partisan_amd import Simulator
    cfg.device = 0
    return Simulator(cfg)


def _gpu3(cfg):
    cfg.n_shards = 3
    return _gpu(cfg)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return CC.run(Oracle, name)


def _same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"histogram {k}: {a[k]} against {b[k]}"


def _check(name, make):
    gs, gst, grest = CC.run(make, name)
    os_, ost, orest = _oracle(name)
    try:
        S.compare_stats(gst, ost)
        assert grest == orest                       # (event_edges: every call's outcome)
        if CC.CASES[name].kind == "pl":
            S.compare_strategy(gs, os_, full_bits=CC.full_bits(name))
        else:
            S.compare_nodes(gs.nodes(), os_.nodes())
            _same_dict(gs.histograms(), os_.histograms())
            for g, o in zip(gs.delivery(), os_.delivery()):
                assert np.array_equal(g, o)
    finally:
        gs.close()


@pytest.mark.parametrize("name", list(CC.CASES))
def test_case(name):
    _check(name, _gpu)


@pytest.mark.parametrize("name", CC.OTHER_PATHS)
def test_case_three_shards(name):
    _check(name, _gpu3)


@functools.lru_cache(maxsize=None)
def _all_oracle_trace(name):
    """the expected exchange: the engine's ranks played by oracle shards; that
    run itself equals the unsharded oracle's"""
    world, ranks = CC.HYBRID
    hy, st, rest = CC.run(lambda cfg: Hybrid(cfg, world, ranks, engine=False), name)
    os_, ost, orest = _oracle(name)
    S.compare_stats(st, ost)
    assert rest == orest and hy.n_out > 0 and hy.n_in > 0
    trace = hy.trace
    hy.close()
    return trace


@pytest.mark.parametrize("name", CC.OTHER_PATHS)
def test_case_host_exchange(name):
    """the engine simulates ranks 1 and 2 of 4: each round's outbound records
    equal the all-oracle exchange's, the summed stats and the engine's node
    state the unsharded oracle's"""
    world, ranks = CC.HYBRID
    expect = _all_oracle_trace(name)
    hy, st, rest = CC.run(lambda cfg: Hybrid(cfg, world, ranks, expect=expect), name)
    os_, ost, orest = _oracle(name)
    try:
        S.compare_stats(st, ost)
        assert rest == orest
        e = hy.engine
        if CC.CASES[name].kind == "pl":
            S.compare_nodes(e.strategy_nodes(), os_.strategy_nodes(e.lo, e.hi - e.lo))
        else:
            S.compare_nodes(e.nodes(), os_.nodes(e.lo, e.hi - e.lo))
    finally:
        hy.close()
