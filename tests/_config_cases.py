"""The case tables of the config matrix: scenarios of tests/_scenarios.py under
config keys, overlay sizes and event orders that psim_create accepts and the
kernels branch on, shared by tests/test_config_cases.py (the oracle alone:
each case differs from the default run and still reaches what it is there
for) and tests/test_gpu_config_matrix.py (GPU against oracle, bit for bit).

A case is (scenario, its arguments, the config keys it overrides).  The
arguments name the run (n, seed, rounds, manager, strategy); the overrides
are what the case is about: the same scenario with the same arguments and no
override is the case's default twin (`twin`)."""
import collections

import numpy as np

import _scenarios as S
from partisan_amd import _abi
from partisan_amd import workloads as W
from partisan_amd.sim import default_config

OVF_IDMAP, OVF_PT_OUT, OVF_PT, OVF_STRATEGY, OVF_CONN = range(5)

# kind: "hv" (HyParView and X-BOT handles: psim_get_nodes, histograms,
# delivery) or "pl" (pluggable handles: psim_get_strategy_nodes);
# ovf: the overflow_by kinds the case may count (the fixed tables)
Case = collections.namedtuple("Case", "scn args cfg kind ovf")
CASES = {}


def _add(name, scn, args, cfg=None, kind="hv", ovf=()):
    assert name not in CASES, name
    CASES[name] = Case(scn, dict(args), dict(cfg or {}), kind, frozenset(ovf))


# ---- HyParView keys: churn, a partition and a broadcast every 10 rounds
CHURN = dict(n=1021, seed=5, rounds=110)
HV_KEYS = {
    "lazy3": dict(lazy_tick_period=3),
    "lazy7_shuf3": dict(lazy_tick_period=7, shuffle_period=3),
    "lazy0": dict(lazy_tick_period=0),
    "plumtree0": dict(plumtree=0),
    "nopromo": dict(random_promotion=0),
    "promo1_min5": dict(promotion_period=1, min_active_size=5),
    "act8_min8": dict(max_active_size=8, min_active_size=8, promotion_period=2),
    "act2": dict(max_active_size=2, min_active_size=2),
    "act3": dict(max_active_size=3, min_active_size=1),
    "arwl0": dict(arwl=0, prwl=0),
    "arwl1_prwl3": dict(arwl=1, prwl=3),
    "prwl_gt": dict(arwl=3, prwl=40),
    "k00": dict(k_active=0, k_passive=0),
    "k70": dict(k_active=7, k_passive=0),
    "k07": dict(k_active=0, k_passive=7),
    "shuf0": dict(shuffle_period=0),
    "shuf1": dict(shuffle_period=1),
    "pas1_act2": dict(max_active_size=2, max_passive_size=1),
}
HV_OVF = {"act2": (OVF_IDMAP,), "pas1_act2": (OVF_CONN,)}
for _k, _cfg in HV_KEYS.items():
    _add(_k, "churn_partition", CHURN, _cfg, ovf=HV_OVF.get(_k, ()))

# ---- the quiet-node path: heal_after_quiet steps several rounds a call
QUIET = dict(n=512, seed=3)
_add("quiet_lazy2", "heal_after_quiet", QUIET, dict(lazy_tick_period=2))
_add("quiet_lazy5", "heal_after_quiet", QUIET, dict(lazy_tick_period=5))
_add("quiet_lazy0", "heal_after_quiet", QUIET, dict(lazy_tick_period=0))
# (the outstanding tables overflow under an off-default period: counted alike)
_add("quiet_lazy3_act8", "heal_after_quiet", QUIET, dict(lazy_tick_period=3, max_active_size=8, min_active_size=5),
     ovf=(OVF_PT_OUT,))

# ---- the batch path
BATCH = dict(n=1500, seed=9)
_add("batch_lazy3", "multistep", BATCH, dict(lazy_tick_period=3))
_add("batch_plumtree0", "multistep", BATCH, dict(plumtree=0))
_add("batch_nopromo", "multistep", BATCH, dict(random_promotion=0))

# ---- X-BOT
XBOT = dict(CHURN, manager=2)
# (an optimization round every round floods: at 1021 nodes 1.8e6 messages and
# 1.6 s of oracle time, so this case runs at 509; the disconnect-id maps and
# the connection table overflow throughout -- counted alike on both sides)
_add("xbot_p1", "churn_partition", dict(XBOT, n=509), dict(xbot_period=1), ovf=(OVF_IDMAP, OVF_CONN))
_add("xbot_p0", "churn_partition", XBOT, dict(xbot_period=0))
_add("xbot_p10_lazy3_act4", "churn_partition", XBOT, dict(xbot_period=10, lazy_tick_period=3, max_active_size=4))

# ---- small overlays: one, two and three nodes; 63 and 65 (a wave row fewer, one more)
SMALL_HV = (1, 2, 3, 5, 63, 65)
for _n in SMALL_HV:
    _add(f"hv_n{_n}", "churn_partition", dict(n=_n, seed=5, rounds=110))
SMALL_PL = (2, 3, 5, 65, 509)
STRATEGY_NAMES = {0: "full", 1: "v1", 2: "v2"}
for _s in (0, 1, 2):
    for _n in SMALL_PL:
        # (the full strategy's gossip to every member floods past 32 nodes: DESIGN.md)
        _a = dict(n=_n, seed=11, rounds=60, strategy=_s, part_at=45, fanout=3 if _s == 0 and _n > 32 else 0)
        if _n > 10:
            _a["crash_at"] = 30
        _add(f"{STRATEGY_NAMES[_s]}_n{_n}", "pl_doubling", _a, kind="pl")
# (pl_doubling draws a victim among the ids from 1: one node is a case of its own)
_add("hv_one_node", "one_node", dict(manager=0))
for _s in (0, 1, 2):
    _add(f"{STRATEGY_NAMES[_s]}_one_node", "one_node", dict(manager=1, strategy=_s), kind="pl")

# ---- pluggable keys
PL = dict(n=1021, seed=11, rounds=90, crash_at=40, part_at=60)
# Cases whose run equals their twin's, each with its reason; every other case
# must differ.  scamp_c: scamp_join takes sublist(the joiner's view before
# the join, c), and every psim_join restarts the joiner with init/1's view,
# itself alone: in pl_doubling the sublist has one candidate, which v1 takes
# for every c >= 1 (c = 1 still differs: the sublist's draw order) and v2 for
# every c.  S.pl_restart_contact fills the joiner's view before its contact's
# state arrives: there c = 3 and c = 64 both differ from c = 5 (below).
NOT_LIVE = {
    "v1_c64": "pl_doubling: a joiner's view is itself alone, one candidate for every c >= 1",
    "v2_c1": "pl_doubling: v2's sublist of a view of the joiner alone changes no digest (measured: equal for c = 1..64)",
    "v2_c64": "pl_doubling: a joiner's view is itself alone, one candidate for every c >= 1",
    # multistep's two broadcasts come from two roots, each over eager links
    # alone: no node has a lazy peer, no IHAVE is sent under any period (the
    # engine still takes its period != 1 branches, in batches)
    "batch_lazy3": "multistep never sends an IHAVE: one broadcast a root",
}
for _s in (1, 2):
    _p = STRATEGY_NAMES[_s]
    _a = dict(PL, strategy=_s)
    _add(f"{_p}_pi1", "pl_doubling", _a, dict(periodic_interval=1), kind="pl")
    # (SCAMP v1: the only case with a view at PSIM_SVIEW_CAP)
    _add(f"{_p}_pi3", "pl_doubling", _a, dict(periodic_interval=3), kind="pl", ovf=(OVF_STRATEGY,) if _s == 1 else ())
    _add(f"{_p}_pi0", "pl_doubling", _a, dict(periodic_interval=0), kind="pl")
    _add(f"{_p}_c1", "pl_doubling", _a, dict(scamp_c=1), kind="pl")
    _add(f"{_p}_c64", "pl_doubling", _a, dict(scamp_c=64), kind="pl")
    # a join whose sublist has up to 64 candidates: c picks among them
    _r = dict(n=1021, seed=11, rounds=60, strategy=_s)
    _add(f"{_p}_c3_restart", "pl_restart_contact", _r, dict(scamp_c=3), kind="pl")
    _add(f"{_p}_c64_restart", "pl_restart_contact", _r, dict(scamp_c=64), kind="pl")
FULL = dict(n=509, seed=11, rounds=90, crash_at=40, part_at=60, strategy=0)
_add("full_pi1_f5", "pl_doubling", dict(FULL, fanout=5), dict(periodic_interval=1), kind="pl")
_add("full_pi3_f64", "pl_doubling", dict(FULL, fanout=64), dict(periodic_interval=3), kind="pl")
# (its twin is the same run with the smallest other fanout, 2: fanout 0 floods)
_add("full_f1", "pl_doubling", dict(FULL, fanout=2), dict(fanout=1), kind="pl")

# ---- event order inside one round
EDGES = dict(n=1021, seed=5, rounds=100)
_add("event_edges", "event_edges", EDGES)
_add("event_edges_v2", "event_edges", dict(EDGES, bcast=False, manager=1, strategy=2), kind="pl")
_add("event_edges_lazy3", "event_edges", EDGES, dict(lazy_tick_period=3))

# ---- other round paths: three virtual shards, and a host-exchange handle
OTHER_PATHS = ("event_edges", "lazy3", "plumtree0", "act2", "v2_pi1")
HYBRID = (4, (1, 3))


def one_node(make, manager=0, strategy=0, rounds=30):
    """A one-node overlay: node 0 starts with no contact and runs alone."""
    sim = make(default_config(n_nodes=1, seed=5, manager=manager, strategy=strategy))
    sim.join(np.array([0], np.uint32), np.array([W.NONE], np.uint32))
    return sim, sim.step(rounds)


def _scenario(scn):
    return one_node if scn == "one_node" else getattr(S, scn)


def run(make, name):
    """(handle, every round's stats, the scenario's further results)"""
    c = CASES[name]
    out = _scenario(c.scn)(make, **dict(c.args, **c.cfg))
    return out[0], out[1], out[2:]


def twin(make, name):
    """the same scenario and arguments without the case's overrides"""
    c = CASES[name]
    out = _scenario(c.scn)(make, **c.args)
    return out[0], out[1], out[2:]


def full_bits(name):
    """the nodes whose member bitsets a full-strategy case compares"""
    c = CASES[name]
    if c.kind != "pl" or c.args.get("strategy") != _abi.STRATEGY_FULL:
        return None
    n = c.args.get("n", 1)
    return sorted({0, n // 2, n - 1})


def allowed_overflow(name, st):
    """the overflow a case counts is of the kinds its table entry names"""
    by = st["overflow_by"].sum(0)
    return all(int(by[k]) == 0 for k in range(_abi.OVF_NKINDS) if k not in CASES[name].ovf)
