"""The scenarios of tests/_lite_quarter_cases.py on the oracle alone: each
still reaches what the GPU tests of k_lite_quarter and k_lite_half need it to
reach, so that
a later change of defaults cannot empty those tests."""
import pytest

import _lite_quarter_cases as Q
from _oracle import Oracle


@pytest.mark.parametrize("name", list(Q.F_CASES))
def test_full_views_reached(name):
    sim, st = Q.run_f(Oracle, name)
    share = Q.full_share(sim, name)
    print(name, "share of full passive views", share)
    assert share >= 0.99
    assert int(st["overflow"].sum()) == 0


def test_deep_inboxes_reached():
    seen = {"largest": 0, "deep": 0, "deep32": 0}

    def each_round(sim, r):
        largest, deep = Q.inbox_depths(sim.inbox())
        seen["largest"] = max(seen["largest"], largest)
        seen["deep"] += deep
        seen["deep32"] += Q.inbox_depths(sim.inbox(), 32)[1]    # (the half kernel's chunk)
    sim, st = Q.run_d(Oracle, each_round)
    print("largest inbox", seen["largest"], "SHUFFLE / SHUFFLE_REPLY records at position >= 16", seen["deep"])
    print("... at position >= 32", seen["deep32"])
    assert seen["deep"] >= 1000
    assert seen["deep32"] >= 1000
    assert seen["largest"] > 32
    assert int(st["overflow"].sum()) == 0
