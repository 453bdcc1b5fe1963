"""The oracle's id windows (orc_create_range) and the id-shifting proxy, on the
CPU: the range oracle is the oracle, two ranges equal one, the proxy at base 0
is the identity, and the three windows the GPU file runs (tests/_high_ids.py:
the top of the id space, 2^26 and 2^24) are worth running -- every message
type the scenario sends is sent there too, every id seen lies in the window
and, where the window straddles a power of two, both sides of it talk to each
other."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _high_ids as H
import _scenarios as S
from _hybrid import ORACLE
from _oracle import Oracle
from partisan_amd.sim import SimError, default_config

NAMES = list(H.SCENARIOS)
SPACE, BASE = 4096, 3000


@functools.lru_cache(maxsize=None)
def _one_range(name):
    """one range oracle over [BASE, BASE + n) of SPACE ids"""
    return H.run(name, H.at_ids(H.one_party(ORACLE), BASE, SPACE))


@functools.lru_cache(maxsize=None)
def _plain(name):
    """the scenario as every other test runs it: ids from 0, unwrapped"""
    return H.run(name, Oracle)


@pytest.mark.parametrize("name", NAMES)
def test_range_oracle_is_the_oracle(name):
    """the unchanged unsharded oracle over all SPACE ids, of which only the
    window's are ever used, against a handle with rows for the window only"""
    whole = H.run(name, H.at_ids(H.whole_oracle, BASE, SPACE))
    try:
        H.compare_runs(name, _one_range(name), whole)
        rows = H.final(name, whole[0])
        ids = rows["strategy_nodes" if H.pluggable(name) else "nodes"]
        assert len(ids) == H.size_of(name)
    finally:
        whole[0].close()


@pytest.mark.parametrize("name", NAMES)
def test_two_ranges_equal_one(name):
    two = H.run(name, H.at_ids(H.split((ORACLE, ORACLE)), BASE, SPACE))
    try:
        H.compare_runs(name, two, _one_range(name))
        assert two[0].n_out > 0 and two[0].n_in > 0
    finally:
        two[0].close()


@pytest.mark.parametrize("name", NAMES)
def test_at_ids_at_base_0_is_the_identity(name):
    n = H.size_of(name)
    got = H.run(name, H.at_ids(H.whole_oracle, 0, n))
    try:
        H.compare_runs(name, got, _plain(name))
    finally:
        got[0].close()


def test_range_handle_refusals():
    """outside its range a range handle answers as a rank handle of the
    engine does; what needs every row it refuses"""
    cfg = default_config(n_nodes=SPACE)
    with pytest.raises(SimError, match="PSIM_EINVAL"):
        Oracle(cfg, 10, 10)
    with pytest.raises(SimError, match="PSIM_EINVAL"):
        Oracle(cfg, 10, SPACE + 1)
    with pytest.raises(SimError, match="PSIM_EUNSUPPORTED"):
        Oracle(default_config(n_nodes=SPACE, manager=1, strategy=0), 0, 10)
    full = Oracle(default_config(n_nodes=64, manager=1, strategy=0), 0, 64)     # (the whole space: no range)
    full.close()
    o = Oracle(cfg, 100, 200)
    try:
        assert o.nodes(100, 100).shape == (100,) and o.delivery(150, 50)[0].shape == (50,)
        for first, count in ((99, 2), (199, 2), (0, 1), (200, 1)):
            for get in (o.nodes, o.delivery):
                with pytest.raises(SimError, match="PSIM_ERANGE"):
                    get(first, count)
        with pytest.raises(SimError, match="PSIM_EUNSUPPORTED"):
            o.histograms()
    finally:
        o.close()
    p = Oracle(default_config(n_nodes=SPACE, manager=1, strategy=2), 100, 200)
    try:
        with pytest.raises(SimError, match="PSIM_ERANGE"):
            p.strategy_nodes(99, 2)
        with pytest.raises(SimError, match="PSIM_EUNSUPPORTED"):
            p.leave_node(np.array([100], np.uint32), np.array([101], np.uint32))
    finally:
        p.close()


# ---------------------------------------------------------------- the windows
def _ids_of(recs, pl):
    """the ids a round's records name: dst, src, the exchange list; a strategy
    record's a0 (PSIM_PL_FWD_SUB 3 .. PSIM_PL_BOOT_REMOVE 7: the node subscribed,
    pinging, kept or removed)"""
    out = [recs[:, 0], recs[:, 1]]
    nex = (recs[:, 2] >> 16) & 0xFF
    for k in range(8):
        out.append(recs[nex > k, 8 + k])
    if pl:
        t = recs[:, 2] & 0xFF
        out.append(recs[(t >= 3) & (t <= 7), 4])
    return np.concatenate(out)


def _view_ids(rows, pl):
    lists = (("view", "view_n"), ("in_view", "in_n")) if pl else (("act", "act_n"), ("pas", "pas_n"))
    out = []
    for f, n in lists:
        k = np.arange(rows[f].shape[1])[None, :] < rows[n][:, None]
        out.append(rows[f][k])
    return np.concatenate(out)


@pytest.mark.parametrize("window", ["top", "2^26", "2^24"])
@pytest.mark.parametrize("name", NAMES)
def test_high_window_is_worth_running(name, window):
    """On the oracle alone.  The partition check: `both groups on both sides`
    holds where the scenario's groups are by id modulo (event_edges).  The
    half/half partition of churn_partition, xbot_churn and the SCAMP runs cuts
    at n / 2, which is where the windows put the power of two: there each
    group lies on one side, and the check is that the cut and the power
    coincide -- every message between the groups then crosses the power."""
    n, pl = H.size_of(name), H.pluggable(name)
    space, base = H.windows(n)[window]
    seen = {"src": [], "dst": [], "all": []}

    def on_records(r, recs):
        seen["src"].append(recs[:, 1].copy())
        seen["dst"].append(recs[:, 0].copy())
        seen["all"].append(_ids_of(recs, pl))

    out = H.run(name, H.at_ids(H.one_party(ORACLE, on_records=on_records), base, space))
    sim = out[0]
    try:
        st = out[1]
        for t in H.SENDS[name]:
            assert st["emitted"][:, t].sum() > 0 and st["delivered"][:, t].sum() > 0, f"message type {t}"
        rows = sim.strategy_nodes() if pl else sim.nodes()
        views = _view_ids(rows, pl)
        ids = np.concatenate(seen["all"] + [views])
        assert len(views) > n and ids.min() >= base and ids.max() < base + n
        if window == "top":
            assert ids.max() == H.TOP - 1 and (np.concatenate(seen["src"]) == H.TOP - 1).any()
            return
        power = 1 << int(window[2:])
        assert base < power < base + n
        src, dst = np.concatenate(seen["src"]), np.concatenate(seen["dst"])
        for what, x in (("source", src), ("destination", dst), ("view member", views)):
            assert (x < power).any() and (x >= power).any(), what
        assert ((src < power) & (dst >= power)).any() and ((src >= power) & (dst < power)).any()
        if name == "multi_root":
            roots = np.array(sorted(sim.roots)) + base
            assert (roots < power).any() and (roots >= power).any(), "broadcast roots on one side only"
        side = np.arange(n) + base >= power
        for g in sim.partitions:
            split = [set(np.unique(g[~side]).tolist()), set(np.unique(g[side]).tolist())]
            if name == "event_edges":
                assert len(split[0]) > 1 and split[0] == split[1]
            else:
                assert split == [{0}, {1}]
    finally:
        sim.close()


# ---------------------------------------------------------------- no row per id
_CHILD = """
import resource, sys
resource.setrlimit(resource.RLIMIT_AS, (8 << 30, 8 << 30))
import _high_ids as H
n = 1024
out = H.run("churn_partition", H.at_ids(H.one_party(), H.TOP - n, H.TOP))
assert int(out[1]["nodes_up"][-1]) == n and int(out[1]["first_deliveries"].sum()) > n
out[0].close()
print("ran", len(out[1]), "rounds")
"""


def test_no_row_per_id():
    """a node row for each of 2^27 - 1 ids is several hundred GB, the
    byte-wide tables together about 1 GB: under an address-space limit of
    8 GiB the first cannot be created and the second runs"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=here, capture_output=True, text=True)
    assert r.returncode == 0 and "ran 110 rounds" in r.stdout, r.stderr[-2000:]
