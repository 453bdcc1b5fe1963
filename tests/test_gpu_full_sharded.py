"""The full-membership strategy over virtual shards and loopback ranks: a
sharded run must equal the unsharded CPU oracle bit for bit -- every round's
stats (state_bytes and digest included), strategy_nodes() and the member
bitsets of nodes 0, 1, n // 2 and n - 1.  A STATE or GOSSIP record that crosses
shards takes the ORSet rows it names along (the payload exchange, DESIGN.md
section 7); the cases pick what that can get wrong: leave/1 stops across
shards, faults, rows longer than one stride of the copy, ragged and tiny
ranges, snapshot/restore with rows in flight, the collective overlay
statistics, and the dedup of rows named by several records of one round.

Oracle runs are computed once per scenario and left unchanged."""
import functools

import numpy as np
import pytest

import _full_sharded as F
import _random_schedule as R
import _scenarios as S
import _strategy_stats as T
from _oracle import Oracle
from partisan_amd import workloads as W
from partisan_amd.sim import HostSim, SimError, default_config

pytestmark = pytest.mark.gpu


def _bits(n):
    return [0, 1, n // 2, n - 1]


@functools.lru_cache(maxsize=None)
def _ref(name, args, kw=()):
    """the oracle's run of scenario S.<name>: (sim, stats, ...), kept open"""
    return getattr(S, name)(Oracle, *args, **dict(kw))


def _same(got, want, n):
    g, o = got[0], want[0]
    try:
        S.compare_stats(got[1], want[1])
        S.compare_strategy(g, o, full_bits=_bits(n))
    finally:
        g.close()


# ---- 1. create
def test_create_sharded_and_hosted():
    from partisan_amd import Simulator
    s = Simulator(default_config(n_nodes=64, seed=3, manager=1, strategy=0, fanout=5, n_shards=3))
    st = s.run_schedule(W.doubling_join(64, 3), 12)
    assert st["emitted"].sum() > 0
    s.close()
    with pytest.raises(SimError) as e:
        HostSim(default_config(n_nodes=64, seed=3, manager=1, strategy=0), 16, 48)
    assert e.value.rc == -7


# ---- 2. flood, stop across shards
LEAVE32_KW = (("strategy", 0), ("fanout", 0), ("k", 4), ("part_at", 60))


@pytest.mark.parametrize("make", [F.vshards(3), F.loopback(3)], ids=["3-shards", "loopback-3"])
def test_flood_stops_across_shards(make):
    want = _ref("pl_leave_remote", (32, 8, 90), LEAVE32_KW)
    o, ost, actors, targets = want
    per = 11
    assert all(int(a) // per != int(t) // per for a, t in zip(actors, targets)), (actors, targets)
    assert [int(a) // per for a in actors] == [1, 0, 2, 0] and [int(t) // per for t in targets] == [0, 1, 0, 2]
    assert not o.strategy_nodes()["up"][targets].any(), "every target stops on the oracle"
    _same(S.pl_leave_remote(make, 32, 8, 90, strategy=0, fanout=0, k=4, part_at=60), want, 32)


# ---- 3. fanout 5 under faults, n = 2048
DOUBLING_KW = (("strategy", 0), ("fanout", 5), ("crash_at", 40), ("part_at", 60))


@pytest.mark.parametrize("make", [F.vshards(4), F.loopback(3)], ids=["4-shards", "loopback-3"])
def test_fanout_crash_partition(make):
    want = _ref("pl_doubling", (2048, 11, 100), DOUBLING_KW)
    _same(S.pl_doubling(make, 2048, 11, 100, strategy=0, fanout=5, crash_at=40, part_at=60), want, 2048)


def test_fanout_omission():
    want = _ref("pl_omission", (2048, 23, 100, 0, 5))
    _same(S.pl_omission(F.vshards(4), 2048, 23, 100, 0, 5), want, 2048)


# ---- 4. long rows with tombstones
LONG_KW = (("strategy", 0), ("fanout", 5), ("k", 4), ("leave_at", 28))


@pytest.mark.parametrize("make", [F.vshards(3), F.loopback(2)], ids=["3-shards", "loopback-2"])
def test_long_rows_with_tombstones(make):
    """n = 8448: fw = 264 words, a row longer than one 256-word stride of a
    64-lane uint4 copy; 528 words once the removes travel"""
    want = _ref("pl_leave_remote", (8448, 8, 70), LONG_KW)
    members = want[0].strategy_nodes()["members"]
    up = want[0].strategy_nodes()["up"].astype(bool)
    assert 8444 <= members[up].min() and members[up].max() <= 8446, (members[up].min(), members[up].max())
    _same(S.pl_leave_remote(make, 8448, 8, 70, strategy=0, fanout=5, k=4, leave_at=28), want, 8448)


# ---- 5. ragged ranges
@pytest.mark.parametrize("n,shards", [(257, 7), (17, 3)])
def test_ragged_ranges(n, shards):
    """257 over 7: per 37, the last shard 35; 17 over 3: rows of 4 words"""
    kw = (("strategy", 0), ("fanout", 5))
    want = _ref("pl_doubling", (n, 5, 60), kw)
    _same(S.pl_doubling(F.vshards(shards), n, 5, 60, strategy=0, fanout=5), want, n)


# ---- 6. the random-schedule corpus
@functools.lru_cache(maxsize=None)
def _corpus_ref(seed):
    sch = R.generate("full", seed)
    return sch, R.execute(R.oracle_make, sch)


FULL_SEEDS = [s for k, s in R.CORPUS if k == "full"]
CORPUS_PATHS = {"shards3": R.gpu_make(3), "shards7": R.gpu_make(7), "loopback3": F.loopback(3)}
# (7 shards: n >= 65 only; generating a schedule runs nothing)
CORPUS_CASES = [(s, p) for s in FULL_SEEDS for p in CORPUS_PATHS
                if p != "shards7" or R.generate("full", s).n >= 65]


@pytest.mark.parametrize("seed,path", CORPUS_CASES, ids=[f"{s}-{p}" for s, p in CORPUS_CASES])
def test_corpus(seed, path):
    sch, ref = _corpus_ref(seed)
    assert sch.n in (17, 65, 257)
    tr = R.execute(CORPUS_PATHS[path], sch, R.Opts(restore=R.resume_into_second_handle))
    R.compare(tr, ref)
    assert len(tr.probes) == len(ref.probes)
    assert tr.restored == sum(1 for s in sch.steps if s[0] == "snapshot_restore")


# ---- 7. overlay statistics
def _stats_run(make):
    """(sim, [histograms in the hook of round 20, after round 30]); the oracle
    answers with the numpy reference over its views and member rows"""
    n, seed = 1027, 11
    sim = make(default_config(n_nodes=n, seed=seed, manager=1, strategy=0, fanout=5))
    seen = []

    def take():
        if isinstance(sim, Oracle):
            seen.append(T.reference(sim.strategy_nodes(), 0, [sim.member_bits(i) for i in range(n)]))
        else:
            seen.append(sim.strategy_histograms())

    def hook(r):
        if r == 16:
            sim.crash(np.arange(400, dtype=np.uint32))
        if r == 20:
            take()
    sim.run_schedule(W.doubling_join(n, seed), 31, extra=hook)
    take()
    return sim, seen


@functools.lru_cache(maxsize=None)
def _stats_ref():
    o, seen = _stats_run(Oracle)
    o.close()
    return seen


@pytest.mark.parametrize("make", [F.vshards(3), F.loopback(3)], ids=["3-shards", "loopback-3"])
def test_overlay_statistics(make):
    """ids 0..399 crash: shard (rank) 0 of 3 holds no live node and the lowest
    live id, 400, lives in shard 1 -- its row must reach the others"""
    want = _stats_ref()
    assert want[0]["n_up"] == 627 and 1 < want[0]["agreeing"] < want[0]["n_up"], want[0]
    assert want[1]["agreeing"] == want[1]["n_up"] == 627, want[1]
    g, got = _stats_run(make)
    try:
        for a, b in zip(got, want):
            T.compare(a, b)
    finally:
        g.close()


# ---- 8. dedup and accounting
def test_rows_travel_once():
    """exchange bytes = 32 B a record + the rows shipped; a snapshot that
    several records of a round name for one shard travels there once: at most
    one row per node and round (2 shards: one other shard)"""
    n, rounds = 8448, 5
    fw = ((n + 31) // 32 + 3) & ~3
    assert fw == 264
    sim = F.vshards(2)(default_config(n_nodes=n, seed=8, manager=1, strategy=0, fanout=5, periodic_interval=1))
    try:
        sim.run_schedule(W.doubling_join(n, 8), 40)
        r0, b0 = sim.exchange_stats()
        sim.step(rounds)
        r1, b1 = sim.exchange_stats()
    finally:
        sim.close()
    recs, nbytes = r1 - r0, b1 - b0
    print(f"records {recs}, bytes {nbytes}, row bytes {nbytes - 32 * recs}")
    assert (nbytes - 32 * recs) % (4 * fw) == 0
    rows = (nbytes - 32 * recs) // (4 * fw)
    print(f"rows {rows}, bound {n * rounds}")
    assert recs > 1.5 * n * rounds                      # (expected 2.5 n rounds: the bound bites)
    assert 0 < rows <= n * rounds
