"""The message trace on the GPU (psim_trace_watch / psim_trace_read /
psim_trace_clear): every record of every round against the reference
(tests/_trace.py: a numpy filter over Oracle.inbox()), exactly, on all 16
words and the round -- under the full strategy STATE and GOSSIP records on
words 0-3, their payload words being arena references.  The oracle steps one
round at a time; the engine makes the step calls of each scenario."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _scenarios as S
import _trace as T
from partisan_amd import _abi
from partisan_amd import workloads as W
from partisan_amd.sim import SimError, default_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM, ESTATE, ERANGE, EUNSUPPORTED = -1, -2, -4, -5, -7
N_HP = 203
WATCH = [0, 31, 32, 63, 64, 202]
MID = 14                                        # scenario 2: the round of its mid-run call
SHUFFLE, PT_BROADCAST, PT_IHAVE = 7, 9, 11


def _gpu(cfg):
    from partisan_amd import Simulator

    cfg.device = 0
    return Simulator(cfg)


def armed(make=_gpu, **watch):
    """`make` whose handle has a watch armed before its first round"""
    def mk(cfg):
        sim = make(cfg)
        sim.trace_watch(**watch)
        return sim
    return mk


def sharded(k):
    def mk(cfg):
        cfg.n_shards = k
        return _gpu(cfg)
    return mk


def hp(make, mid=None, n=N_HP, seed=11, **cfg):
    """Scenario 2: HyParView + Plumtree at 203 nodes (no multiple of 32), 30
    rounds: the doubling bootstrap to round MID, mid(sim), a broadcast, 6
    rounds, a second broadcast (over the first one's lazy links: IHAVEs), 10
    rounds."""
    sim = make(default_config(n_nodes=n, seed=seed, **cfg))
    sim.run_schedule(W.doubling_join(n, seed), MID)
    if mid is not None:
        mid(sim)
    sim.broadcast(0, 5)
    sim.step(6)
    sim.broadcast(0, 6)
    sim.step(10)
    return sim


def many_blocks(make, n=4096, seed=9):
    """Scenario 3, in the shape of S.multistep: bootstrap, step(40), a
    broadcast, step(30), a crash wave, step(20).  Returns (sim, stats)."""
    sim = make(default_config(n_nodes=n, seed=seed))
    st = [sim.run_schedule(W.doubling_join(n, seed), 20)]
    st.append(sim.step(40))
    sim.broadcast(0, 1)
    st.append(sim.step(30))
    rng = np.random.Generator(np.random.PCG64([seed, 77]))
    victims = np.sort(rng.choice(np.arange(1, n, dtype=np.uint32), size=n // 20, replace=False)).astype(np.uint32)
    sim.crash(victims)
    st.append(sim.step(20))
    return sim, np.concatenate(st)


@pytest.fixture(scope="module")
def hp_tape():
    o = hp(T.TapedOracle)
    tape = o.tape
    o.close()
    assert [r for r, _ in tape] == list(range(30))
    return tape


def _total(tape):
    return sum(len(x) for _, x in tape)


# ---- 1. config A
def test_config_a_watch_all():
    o, _ = S.config_a(T.TapedOracle)
    c = o.counts()
    assert (c == 0).any() and (c == 1).any() and ((c > 1) & (c < 64)).any()
    g, _ = S.config_a(armed(capacity=int(c.sum()) + 1))
    T.assert_same(g.trace_read(), T.Reference(32).feed(o.tape).read())
    g.close()
    o.close()


# ---- 2. HyParView + Plumtree, 203 nodes
@pytest.mark.parametrize("to,frm", [(True, False), (False, True), (True, True)])
def test_watched_nodes_by_direction(hp_tape, to, frm):
    g = hp(armed(nodes=WATCH, to=to, frm=frm, capacity=1 << 14))
    want = T.Reference(N_HP, WATCH, to=to, frm=frm).feed(hp_tape).read()
    assert 0 < len(want[0]) < _total(hp_tape)
    T.assert_same(g.trace_read(), want)
    g.close()


def test_repeated_ids_are_a_set(hp_tape):
    g = hp(armed(nodes=WATCH + WATCH[::-1] + [31], capacity=1 << 14))
    T.assert_same(g.trace_read(), T.Reference(N_HP, WATCH).feed(hp_tape).read())
    g.close()


def test_type_mask(hp_tape):
    types = [SHUFFLE, PT_BROADCAST, PT_IHAVE]
    g = hp(armed(nodes=WATCH, types=types, capacity=1 << 14))
    want = T.Reference(N_HP, WATCH, type_mask=T.mask_of(types)).feed(hp_tape).read()
    assert set(np.unique(want[0][:, 2] & 0xFF)) == set(types)      # (each of the three occurs)
    T.assert_same(g.trace_read(), want)
    g.close()


def test_rearm_mid_run(hp_tape):
    """a second watch discards the first one's records and its lost count, and
    starts with the next round stepped"""
    g = hp(armed(capacity=50), mid=lambda sim: sim.trace_watch(nodes=WATCH, frm=False, capacity=1 << 14))
    assert _total([x for x in hp_tape if x[0] < MID]) > 50         # (the first watch had lost records)
    T.assert_same(g.trace_read(), T.Reference(N_HP, WATCH, frm=False).feed(hp_tape, first=MID).read())
    g.close()


# ---- 3. many blocks
def test_many_blocks_and_read_only():
    o, ost = many_blocks(T.TapedOracle)
    c = o.counts()
    assert ((c > 4096) & (c % 64 != 0)).any()                      # at least three blocks, a ragged last group
    g, gst = many_blocks(armed(capacity=int(c.sum()) + 1))
    T.assert_same(g.trace_read(), T.Reference(4096).feed(o.tape).read())
    # the armed run (single rounds) against an unarmed one (batches) of the same calls
    u, ust = many_blocks(_gpu)
    S.compare_stats(gst, ust)
    S.compare_stats(gst, ost)
    S.compare_nodes(g.nodes(), u.nodes())
    for x in (g, u, o):
        x.close()


# ---- 4. capacity
@pytest.mark.parametrize("shards", [1, 3])
def test_capacity(hp_tape, shards):
    got = []
    g = hp(armed(sharded(shards), capacity=100), mid=lambda sim: got.append(sim.trace_read()))
    got.append(g.trace_read())
    ref = T.Reference(N_HP, capacity=100).feed(hp_tape, last=MID)
    first = ref.read()
    second = ref.feed(hp_tape, first=MID).read()
    every = T.Reference(N_HP).feed(hp_tape).read()
    assert np.array_equal(first[0], every[0][:100]) and first[2] == _total([x for x in hp_tape if x[0] < MID]) - 100
    assert len(second[0]) == 100 and (second[1] >= MID).all() and first[2] + second[2] + 200 == len(every[0])
    T.assert_same(got[0], first)
    T.assert_same(got[1], second)                                  # (the buffer filled again from the next round)
    g.close()


# ---- 5. shards and ranks
@pytest.mark.parametrize("watch", [None, WATCH])
def test_three_shards(hp_tape, watch):
    g = hp(armed(sharded(3), nodes=watch, capacity=1 << 14))
    T.assert_same(g.trace_read(), T.Reference(N_HP, watch).feed(hp_tape).read())
    g.close()


def test_two_loopback_ranks(hp_tape):
    from _loopback import LoopbackRanks

    def mk(cfg):
        lr = LoopbackRanks(cfg, 2)
        lr._all("trace_watch", WATCH, True, True, None, 1 << 14)
        return lr
    lr = hp(mk)
    crossed = 0
    for r, sim in enumerate(lr.ranks):
        owned = (r * lr.per, min(N_HP, (r + 1) * lr.per))
        want = T.Reference(N_HP, WATCH, owned=owned).feed(hp_tape).read()
        T.assert_same(sim.trace_read(), want)
        src, dst = want[0][:, 1], want[0][:, 0]
        there = (src < owned[0]) | (src >= owned[1])
        crossed += int((there & np.isin(src, WATCH) & ~np.isin(dst, WATCH)).sum())
    assert crossed > 0                          # records FROM a watched src on the other rank
    lr.close()


# ---- 6. other managers
def _tape_of(run):
    out = run(T.TapedOracle)
    o = out[0]
    tape = o.tape
    o.close()
    return tape


def test_xbot():
    def run(make):
        return S.churn_partition(make, n=2048, rounds=60, manager=2, xbot_period=10)
    tape = _tape_of(run)
    types = np.concatenate([x[:, 2] & 0xFF for _, x in tape])
    assert np.isin(types, _abi.XBOT_TYPES).sum() > 100
    g = run(armed(capacity=_total(tape) + 1))[0]
    T.assert_same(g.trace_read(), T.Reference(2048).feed(tape).read())
    g.close()


def test_scamp_v2():
    def run(make):
        return S.pl_doubling(make, 2048, 11, 50, strategy=2, crash_at=40)
    tape = _tape_of(run)
    types = set(np.unique(np.concatenate([x[:, 2] & 0xFF for _, x in tape])))
    assert {3, 5} <= types                      # PSIM_PL_FWD_SUB, PSIM_PL_KEEP_SUB
    g = run(armed(capacity=_total(tape) + 1))[0]
    T.assert_same(g.trace_read(), T.Reference(2048).feed(tape).read())
    g.close()


def test_full_strategy():
    def run(make):
        return S.pl_doubling(make, 2048, 11, 30, strategy=0, fanout=5)
    tape = _tape_of(run)
    types = set(np.unique(np.concatenate([x[:, 2] & 0xFF for _, x in tape])))
    assert {T.PL_STATE, T.PL_GOSSIP} <= types
    g = run(armed(capacity=_total(tape) + 1))[0]
    T.assert_same(g.trace_read(), T.Reference(2048).feed(tape).read(), opaque_payload=True)
    g.close()


# ---- 7. error paths and lifecycle
def _watch(sim, nodes, n, dir_, mask, capacity):
    p = None if nodes is None else _abi.u32p(np.ascontiguousarray(nodes, np.uint32))
    return sim._extra["trace_watch"](sim._h, p, n, dir_, mask, capacity)


def test_error_paths_in_order():
    from partisan_amd.sim import HostSim

    sim = _gpu(default_config(n_nodes=64))
    fn = sim._extra["trace_watch"]
    ok = np.array([1, 2], np.uint32)
    assert fn(None, _abi.u32p(ok), 2, 3, 1, 10) == EINVAL
    assert _watch(sim, None, 2, 3, 1, 10) == EINVAL
    assert _watch(sim, ok, 2, 0, 1, 10) == EINVAL
    assert _watch(sim, ok, 2, 4, 1, 10) == EINVAL
    assert _watch(sim, ok, 2, 3, 0, 10) == EINVAL
    assert _watch(sim, ok, 2, 3, 1 << _abi.NTYPES, 10) == EINVAL
    assert _watch(sim, ok, 2, 3, 1, 0) == EINVAL
    assert _watch(sim, [1, 64], 2, 0, 1, 10) == EINVAL              # (EINVAL comes before ERANGE)
    assert _watch(sim, [1, 64], 2, 3, 1, 1 << 44) == ERANGE         # (and ERANGE before ENOMEM)
    # no watch yet: nothing to read, nothing to clear
    n, lost = C.c_size_t(), C.c_uint64()
    rd = sim._extra["trace_read"]
    assert rd(sim._h, None, None, 0, C.byref(n), C.byref(lost)) == ESTATE
    assert rd(None, None, None, 0, C.byref(n), C.byref(lost)) == EINVAL
    assert rd(sim._h, None, None, 0, None, C.byref(lost)) == EINVAL
    sim.trace_clear()
    assert sim._extra["trace_clear"](None) == EINVAL
    with pytest.raises(SimError) as e:
        sim.trace_read()
    assert e.value.rc == ESTATE
    # an allocation that cannot succeed leaves the old watch and its records
    sim.trace_watch(capacity=1 << 10)
    sim.run_schedule(W.sequential_join(8), 12)
    assert _watch(sim, ok, 2, 3, 1, 1 << 44) == ENOMEM
    buf = np.zeros((4, 16), np.uint32)
    assert rd(sim._h, _abi.u32p(buf), None, 4, C.byref(n), C.byref(lost)) == EINVAL   # (recs without rounds)
    assert rd(sim._h, None, None, 0, C.byref(n), C.byref(lost)) == 0 and n.value > 4
    few = np.zeros(4, np.uint32)
    k = n.value
    assert rd(sim._h, _abi.u32p(buf), _abi.u32p(few), 4, C.byref(n), C.byref(lost)) == 0   # (cap < n: the count only)
    assert n.value == k and not buf.any()
    recs, rounds, lost = sim.trace_read()
    assert len(recs) == k and lost == 0 and rounds.max() <= 11
    sim.step(3)                                 # still armed
    assert len(sim.trace_read()[0]) > 0
    sim.trace_clear()
    sim.trace_clear()
    with pytest.raises(SimError):
        sim.trace_read()
    sim.close()
    # a host-exchange handle has psim_get_outbound; EINVAL first, then EUNSUPPORTED, then ERANGE
    hs = HostSim(default_config(n_nodes=64), 16, 48)
    assert _watch(hs, ok, 2, 0, 1, 10) == EINVAL
    assert _watch(hs, [1, 64], 2, 3, 1, 10) == EUNSUPPORTED
    assert _watch(hs, None, 0, 3, 1, 10) == EUNSUPPORTED
    hs.close()


def test_snapshot_and_restore_leave_the_trace_alone(hp_tape):
    """the snapshot holds no trace, and a restore touches neither the watch nor
    the records buffered -- those of the rounds stepped since the snapshot
    included; the rounds after the restore are captured as they run again"""
    got = []

    def mid(sim):
        snap = sim.snapshot()
        sim.broadcast(0, 5)
        sim.step(3)
        sim.restore(snap)
        got.append(sim.trace_read())
    g = hp(armed(capacity=1 << 14), mid=mid)
    T.assert_same(got[0], T.Reference(N_HP).feed(hp_tape, last=MID + 3).read())
    T.assert_same(g.trace_read(), T.Reference(N_HP).feed(hp_tape, first=MID).read())
    g.close()


def test_trace_report_prints_a_timeline():
    r = subprocess.run([sys.executable, "-m", "partisan_amd.trace_report", "--nodes", "1024", "--watch", "7,1023",
                        "--device", "0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    for w in (7, 1023):
        block = out.split(f"node {w}:\n")[1].split("\n\n")[0].splitlines()
        lines = [x for x in block if x.startswith("  round ")]
        assert any("<-" in x and "PT_BROADCAST" in x for x in lines) and any("->" in x for x in lines)
        assert sum(x.startswith("  => first BROADCAST from node ") for x in block) == 1
        assert sum(x.startswith("  => active in-neighbours [") for x in block) == 1
