"""The registry of parity runs: every scenario a GPU parity file runs against
the oracle, by name, as a function of the backend (`make`).  The GPU tests
call these entries with the engine and with the oracle; the coverage tool
(tests/_oracle_coverage.py) calls the same entries with the oracle alone, so
what it reports as never taken is never taken by the runs the GPU is
compared on.  The 2^20-node runs are left out (the tool would spend minutes
on them; they repeat the 2^16 runs' schedule).

  PARITY   tests/test_gpu_parity.py
  RARE     tests/test_gpu_rare_branches.py (the scenarios written for one
           oracle outcome each; RARE_TARGETS names that outcome)
  config matrix, random-schedule corpus, sets v1: their own tables
           (_config_cases.CASES, _random_schedule.CORPUS, SETS_V1 below)

An entry returns what its scenario returns: (handle, stats, ...)."""
import numpy as np

import _config_cases as CC
import _high_ids as HI
import _random_schedule as R
import _scenarios as S
from _hybrid import Hybrid


def _then_broadcast(n, seed, rounds, tail):
    def run(make):
        sim, st = S.doubling(make, n, seed, rounds)
        sim.broadcast(0, 5)
        return sim, np.concatenate([st, sim.step(tail)])
    return run


def batch_regrow(make):
    sim, _ = S.doubling(make, 4096, 9, 30, bcast_period=0, bcast_first=0)
    sim.broadcast(7, 1)
    out = [sim.step(60)]                      # one step call: batches, growth inside
    sim.crash(np.arange(3, 4096, 37, dtype=np.uint32))
    out.append(sim.step(40))
    return sim, out


def histograms_run(make):
    sim, st = S.doubling(make, 2048, 3, 70, bcast_period=25, bcast_first=30)
    sim.crash(np.arange(5, 2048, 61, dtype=np.uint32))
    return sim, np.concatenate([st, sim.step(2)])


def _p(fn, *a, **kw):
    return lambda make: fn(make, *a, **kw)


PARITY = {
    "config_a": _p(S.config_a),
    "churn_partition": _p(S.churn_partition, n=2048),
    "churn_partition_4096": _p(S.churn_partition, n=4096),
    "out_tail": _p(S.out_tail),
    "out_tail_at_cap": _p(S.out_tail, period=1, snap_at=(60, 79)),
    "lingering_exits": _p(S.lingering_exits),
    "e_miniature": _p(S.e_miniature),
    "crash_only": _p(S.crash_only),
    "crash_revive": _p(S.crash_revive),
    "star_512": _p(S.star, n=512),
    "star_64k": _p(S.star, n=1 << 16),
    "variants": _p(S.churn_partition, n=1024, seed=13, rounds=110, **S.VARIANT),
    "doubling_64k": _then_broadcast(1 << 16, 21, 60, 40),
    "doubling_64k_shards": _then_broadcast(1 << 16, 21, 60, 30),
    "strategy_64k": _p(S.pl_doubling, 1 << 16, 13, 60, strategy=2),
    "route_regrow": _p(S.doubling, 1024, 4, 40, bcast_period=10, bcast_first=15),
    "batch_regrow": batch_regrow,
    "histograms": histograms_run,
    "multi_root_120": _p(S.multi_root, roots=4, rounds=120),
    "multi_root_512_6": _p(S.multi_root, n=512, roots=6, rounds=60),
    "heartbeat": _p(S.heartbeat),
    "xbot_64k": _p(S.doubling, 1 << 16, 31, 70, bcast_period=10, bcast_first=30, manager=2, xbot_period=12),
    "trace_churn_partition_1024": _p(S.churn_partition, n=1024),
    "trace_full_16_fanout0": _p(S.pl_doubling, 16, 11, 80, strategy=0, fanout=0, crash_at=40),
    "trace_full_1024_fanout5": _p(S.pl_doubling, 1024, 11, 80, strategy=0, fanout=5, part_at=50),
    "trace_scamp_v1_leave_1024": _p(S.pl_leave_remote, 1024, 7, 90, strategy=1, part_at=60),
    "trace_scamp_v2_leave_1024": _p(S.pl_leave_remote, 1024, 7, 90, strategy=2, part_at=60),
    "trace_full_leave_1024_fanout5": _p(S.pl_leave_remote, 1024, 8, 90, strategy=0, fanout=5, k=4),
    "buckets_config_a": lambda make: S.config_a(S.with_buckets(make, 11)),
    "buckets_churn_partition": lambda make: S.churn_partition(S.with_buckets(make, 12), n=2048),
    "buckets_doubling_64k": lambda make: _then_broadcast(1 << 16, 21, 60, 30)(S.with_buckets(make, 13)),
    "buckets_xbot": lambda make: S.xbot_churn(S.with_buckets(make, 14), n=1024, rounds=100),
    "buckets_scamp_v1": lambda make: S.pl_doubling(S.with_buckets(make, 15), 2048, 5, 60, 1, crash_at=30, part_at=40),
}
for _s in (1, 2, 3):
    PARITY[f"doubling_{_s}"] = _p(S.doubling, 1024, _s, 60, bcast_period=10, bcast_first=25)
for _s in (3, 4):
    PARITY[f"joiner_crash_{_s}"] = _p(S.joiner_crash, seed=_s, **S.VARIANT)
for _st, _n, _f in [(0, 16, 0), (0, 2048, 5), (1, 2048, 0), (2, 2048, 0)]:
    PARITY[f"strategy_{_st}_{_n}"] = _p(S.pl_doubling, _n, 11, 100, strategy=_st, fanout=_f, crash_at=40, part_at=60)
for _st, _n, _f in [(0, 32, 0), (0, 2048, 5), (1, 2048, 0), (2, 2048, 0)]:
    PARITY[f"omission_{_st}_{_n}"] = _p(S.pl_omission, _n, 23, 100, _st, _f)
for _st in (0, 1, 2):
    PARITY[f"strategy_leave_{_st}"] = _p(S.pl_doubling, 1024, 11, 90, strategy=_st, fanout=5 if _st == 0 else 0,
                                         crash_at=40, part_at=60, leave=True)
for _st in (1, 2):
    PARITY[f"remote_leave_{_st}"] = _p(S.pl_leave_remote, 2048, 7, 90, strategy=_st, part_at=60)
    PARITY[f"strategy_shards_{_st}"] = _p(S.pl_doubling, 4096, 12, 80, strategy=_st, crash_at=40)
    PARITY[f"trace_scamp_v{_st}_1024"] = _p(S.pl_doubling, 1024, 11, 100, strategy=_st, crash_at=40, part_at=60)
for _n, _f in [(32, 0), (2048, 5)]:
    PARITY[f"full_remote_leave_{_n}"] = _p(S.pl_leave_remote, _n, 8, 90, strategy=0, fanout=_f, k=4, part_at=60)
for _r, _rd, _c in [(4, 200, False), (4, 160, True), (6, 120, False)]:
    PARITY[f"multi_root_{_r}_{_rd}"] = _p(S.multi_root, roots=_r, rounds=_rd, churn=_c)
for _per in (35, 10, 20):
    PARITY[f"xbot_{_per}"] = _p(S.churn_partition, n=2048, manager=2, xbot_period=_per)

# tests/test_gpu_sets_v1.py: (n, per_round)
SETS_V1 = {"sets_v1_180": (180, 20), "sets_v1_200": (200, 10)}


def sets_v1(name):
    n, per_round = SETS_V1[name]
    return lambda make: S.pl_v1_large_view(S.with_phash(make, 3), n=n, per_round=per_round)


# tests/test_gpu_rare_branches.py.  kind: "hv" (compare_nodes) or "pl"
# (compare_strategy); plumtree: the run sends Plumtree messages (it runs under
# the k_pt fallback too).  RARE_TARGETS: the oracle outcomes the scenario was
# written for, as the coverage tool keys them (function, source text of the
# line, n-th condition on it, outcome).
RARE = {}
RARE_KIND = {}
RARE_PLUMTREE = set()
RARE_TARGETS = {}


def _rare(name, fn, targets, kind="hv", plumtree=False):
    RARE[name] = fn
    RARE_KIND[name] = kind
    RARE_TARGETS[name] = list(targets)
    if plumtree:
        RARE_PLUMTREE.add(name)


_HAVE = "pt_have | if (c->h->slot_msg[k] != msg) { ovf(c, PSIM_OVF_PT); return 1; } | 0: c->h->slot_msg[k] != msg | T"
_ROOT = ("msg_root | if (c->h->slot_msg[k] != msg) { ovf(c, PSIM_OVF_PT); return PSIM_NONE; } | "
         "0: c->h->slot_msg[k] != msg | T")
_ADD_W = "pt_add_out | (s->out_peer[i] == peer && s->out_msg[i] == msg && s->out_round[i] < rnd))) | "
_ADD_I = "pt_add_out | if (i < s->out_n && s->out_peer[i] == peer && s->out_msg[i] == msg && s->out_round[i] == rnd) | "
_ACK = "pt_ack_out | if (s->out_peer[i] == peer && s->out_msg[i] == msg && s->out_round[i] == rnd) { | "
_WAS = "full_leave | if (was) { b[h->W + (t >> 5)] |= 1u << (t & 31u); c->dirty = 1; } | 0: was | F"
_WAS_W = "full_leave | if (was && w == (t >> 5)) x |= 1u << (t & 31u); | "
_rare("retired_ids", _p(S.retired_ids), [_HAVE, _ROOT], plumtree=True)
_rare("same_id_again", _p(S.same_id_again),
      [_ADD_W + "1: s->out_msg[i] == msg | T", _ADD_W + "2: s->out_round[i] < rnd | T",
       _ADD_W + "2: s->out_round[i] < rnd | F", _ADD_I + "2: s->out_msg[i] == msg | T",
       _ADD_I + "3: s->out_round[i] == rnd | T", _ADD_I + "3: s->out_round[i] == rnd | F",
       _ACK + "2: s->out_round[i] == rnd | F",
       "pt_handle | if (pt_have(c, msg)) { #2 | 0: pt_have(c, msg) | F"], plumtree=True)
_rare("set_pool_full", _p(S.set_pool_full),
      ["pool_add | if (pool_n(n) >= PSIM_PT_SET_POOL) { ovf(c, PSIM_OVF_PT); return; } | "
       "0: pool_n(n) >= PSIM_PT_SET_POOL | T", _HAVE, _ROOT], plumtree=True)
_rare("epoch_refusal", _p(S.epoch_refusal),
      ["hv_handle | if (addable_epoch(c, pe, p) && !list_member(act0, n0, p)) { | 0: addable_epoch(c, pe, p) | F"],
      plumtree=True)
_rare("full_leave_absent_f0", _p(S.full_leave_absent), [_WAS, _WAS_W + "0: was | F"], kind="pl")
_rare("full_leave_absent_f0_w3", _p(S.full_leave_absent, n=72, started=24),
      [_WAS, _WAS_W + "0: was | F", _WAS_W + "1: w == (t >> 5) | F"], kind="pl")
_rare("full_leave_absent_f5", _p(S.full_leave_absent, n=72, started=64, fanout=5), [_WAS], kind="pl")
_rare("pending_keep", _p(S.pending_keep),
      ["pl_send | if (!connect_ok(c, dst) || !(full || pl_member(c, dst) || dst == snd(c->h, c->me)->pending)) { | "
       "3: dst == snd(c->h, c->me)->pending | T"], kind="pl")


def runs():
    """every run of the registry: name -> function of `make`"""
    out = {}
    for k, f in PARITY.items():
        out["parity:" + k] = f
    for k in CC.CASES:
        out["config:" + k] = (lambda k: lambda make: CC.run(make, k))(k)
    for kind, seed in R.CORPUS:
        out[f"random:{kind}-{seed}"] = (lambda kind, seed: lambda make: R.execute(make, R.generate(kind, seed)))(
            kind, seed)
    for kind in R.KINDS:
        if kind != "full":
            for seed in R.CORPUS_SEEDS[kind][:2]:
                out[f"random-host:{kind}-{seed}"] = (
                    lambda kind, seed: lambda make: R.execute(make, R.generate(kind, seed, host=True)))(kind, seed)
    # the all-oracle exchange the host-exchange tests expect (oracle shards
    # through orc_round_emit / orc_round_absorb): `make` is not used
    for k in CC.OTHER_PATHS:
        out["config-hybrid:" + k] = (lambda k: lambda make: CC.run(
            lambda cfg: Hybrid(cfg, CC.HYBRID[0], CC.HYBRID[1], engine=False), k))(k)
    for kind in R.KINDS:
        if kind != "full":
            for seed in R.CORPUS_SEEDS[kind][:2]:
                out[f"random-hybrid:{kind}-{seed}"] = (lambda kind, seed: lambda make: R.execute(
                    R.hybrid_make(engine=False), R.generate(kind, seed, host=True), R.path("oracle-sharded")[1]))(
                        kind, seed)
    # tests/test_gpu_high_ids.py: the range oracle (orc_create_range) the engine
    # is compared with in the id windows, as one party and as two that
    # exchange; `make` is not used
    for k in HI.SCENARIOS:
        for w in ("top", "2^26", "2^24"):
            out[f"high-ids:{k}@{w}"] = (lambda k, w: lambda make: HI.run(k, HI.at_ids(
                HI.one_party(), *reversed(HI.windows(HI.size_of(k))[w])), **HI.gpu_kw(k, w)))(k, w)
    for k in HI.BOUNDARY:
        out[f"high-ids-split:{k}"] = (lambda k: lambda make: HI.run(k, HI.at_ids(
            HI.split(("engine", "oracle"), engine=False), *reversed(HI.windows(HI.size_of(k))["top"])),
            **HI.gpu_kw(k, "top")))(k)
    out["high-ids:buckets@2^24"] = lambda make: HI.run("churn_partition", S.with_buckets(HI.at_ids(
        HI.one_party(), *reversed(HI.windows(1024)["2^24"])), 12))
    for kind in R.KINDS:
        if kind != "full":
            for seed in R.CORPUS_SEEDS[kind][:2]:
                out[f"high-ids-random:{kind}-{seed}"] = (lambda kind, seed: lambda make: R.execute(
                    HI.at_ids(HI.one_party(), HI.TOP - R.generate(kind, seed, host=True).n, HI.TOP),
                    R.generate(kind, seed, host=True, rounds=HI.RANDOM_TOP_ROUNDS),
                    R.path("oracle-sharded")[1]))(kind, seed)
    for k in SETS_V1:
        out["sets_v1:" + k] = sets_v1(k)
    for k, f in RARE.items():
        out["rare:" + k] = f
    return out
