"""The Erlang NIF shim with the HIP library behind it: the driver program of
tests/nif_run linked against libpartisan_gpu_sim.so, one child process a
case, each with its own timeout, no sanitizer.  The expected side is the
oracle called directly (or tests/_strategy_stats.py and
tests/_graph_metrics.py over the oracle's rows), never the engine.  All cases
run at 65 or 257 nodes: past a 64-lane wave and a 256-thread block."""
import numpy as np
import pytest

import _graph_metrics as GM
import _nif_run as N
import _random_schedule as R
import _strategy_stats as SS
from _hybrid import OracleShard, canonical
from _oracle import Oracle
from partisan_amd.sim import SimError, default_config

pytestmark = pytest.mark.gpu
TIMEOUT = 120.0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return N.build(tmp_path_factory.mktemp("nif_run_gpu"), backend="gpu")


_WANT = {}


def _want(kind, seed, host=False):
    """the oracle's projected trace of a schedule, taken once"""
    key = (kind, seed, host)
    if key not in _WANT:
        sch = R.generate(kind, seed, host=host)
        assert sch.n in (65, 257)
        opts = R.Opts(drop=("histograms",), single_rounds=True) if host else None
        _WANT[key] = (sch, N.project(R.execute(R.oracle_make, sch, opts)))
    return _WANT[key]


# ---------------------------------------------------------------- equivalence
# three corpus entries a kind, at 65 and 257 nodes
ENTRIES = [("hv", 2), ("hv", 5), ("hv", 6), ("xbot", 2), ("xbot", 5), ("xbot", 11),
           ("scamp_v1", 2), ("scamp_v1", 5), ("scamp_v1", 9), ("scamp_v2", 2), ("scamp_v2", 5), ("scamp_v2", 9),
           ("full", 1), ("full", 4), ("full", 5)]


@pytest.mark.parametrize("kind,seed", ENTRIES, ids=[f"{k}-{s}" for k, s in ENTRIES])
def test_equivalence_and_restore(exe, kind, seed):
    """execute + project through the shim and the engine equals the oracle;
    at the schedule's restore points snapshot/1 goes into restore/2 of a
    second handle of the same program, and the rest of the trace still equals"""
    sch, want = _want(kind, seed)
    with N.Beam(exe, timeout=TIMEOUT) as b:
        got = R.execute(N.nif_make(b), sch, R.Opts(restore=N.restore_in_child))
        b.finish_clean()
    assert got.restored >= 1
    N.same(got, want)


# ---------------------------------------------------------------- device-only calls
def _grow(sim, n):
    """a doubling bootstrap, twenty rounds, two crashes, three rounds"""
    sim.join([0], [N.NONE])
    sim.step(1)
    lo = 1
    while lo < n:
        hi = min(2 * lo, n)
        sim.join(list(range(lo, hi)), [i % lo for i in range(hi - lo)])
        sim.step(2)
        lo = hi
    sim.step(20)
    sim.crash([3, 17])
    sim.step(3)


def _oracle_rows(cfg, pl):
    o = Oracle(type(cfg).from_buffer_copy(cfg))
    _grow(o, cfg.n_nodes)
    rows = o.strategy_nodes() if pl else o.nodes()
    bits = np.stack([o.member_bits(i) for i in range(cfg.n_nodes)]) if pl and cfg.strategy == 0 else None
    o.close()
    return rows, bits


@pytest.mark.parametrize("strategy,n", [(2, 257), (0, 65)])
def test_strategy_histograms(exe, strategy, n):
    cfg = default_config(n_nodes=n, seed=7, manager=1, strategy=strategy, fanout=3, periodic_interval=2)
    rows, bits = _oracle_rows(cfg, True)
    want = SS.reference(rows, strategy, bits)
    with N.Beam(exe, timeout=TIMEOUT) as b:
        sim = N.NifSim(b, cfg)
        _grow(sim, n)
        got = sim.strategy_histograms()
        b.finish_clean()
    assert sorted(got) == sorted(want)
    assert int(want["n_up"]) == n - 2 and (want["links"] > 0 or strategy == 0)
    SS.compare(got, want)


@pytest.mark.parametrize("manager,strategy,n", [(0, 0, 257), (1, 1, 65)])
def test_graph_metrics(exe, manager, strategy, n):
    """64 sources in an odd-address binary (a dead one among them), and []"""
    cfg = default_config(n_nodes=n, seed=7, manager=manager, strategy=strategy, periodic_interval=2)
    rows, _ = _oracle_rows(cfg, manager == 1)
    kind = "scamp" if manager == 1 else "hv"
    src = np.random.Generator(np.random.PCG64([n, 0x6d])).choice(n, size=64, replace=False).astype(np.uint32)
    src[5] = 17                    # (crashed)
    src = np.array(list(dict.fromkeys(int(x) for x in src)), np.uint32)
    with N.Beam(exe, timeout=TIMEOUT) as b:
        sim = N.NifSim(b, cfg)
        _grow(sim, n)
        got, got0 = sim.graph_metrics(src), sim.graph_metrics([])
        b.finish_clean()
    for g, w in ((got, GM.reference(rows, kind, [int(x) for x in src])), (got0, GM.reference(rows, kind, []))):
        assert sorted(g) == sorted(w)
        assert len(g["reach"]) == 64 and len(g["ecc"]) == 64 and len(g["dist"]) == 64
        GM.compare(g, w)
    assert got["pairs_reached"] > 0 and got["sources_live"] == len(src) - len({3, 17} & {int(x) for x in src}) and got["cl_pairs"] > 0
    assert got0["pairs_reached"] == 0 and got0["cl_pairs"] == got["cl_pairs"]


def test_device_only_calls_unsupported_where_the_header_says(exe):
    with N.Beam(exe, timeout=TIMEOUT) as b:
        unsupported = ("error", N.STRERROR[-7])
        for k, (cfg, sh, gm) in enumerate(((dict(manager=0), False, True), (dict(manager=2), False, True),
                                           (dict(manager=1, strategy=0), True, False),
                                           (dict(manager=1, strategy=2), True, True),
                                           (dict(manager=0, host_lo=16, host_hi=48), False, False))):
            ans = b.call(f"h{k} = create {N.erl(dict(cfg, n_nodes=65, seed=3))}")
            assert ans[0] == "ok", ans
            a = b.call(f"strategy_histograms $h{k}")
            assert (a[0] == "ok") if sh else (a == unsupported), (cfg, a)
            a = b.call(f"graph_metrics_nif $h{k} <<>> 0")
            assert (a[0] == "ok") if gm else (a == unsupported), (cfg, a)
        assert b.call("step $h4 1") == unsupported
        b.finish_clean()


# ---------------------------------------------------------------- snapshot and restore
def test_restore_refuses_a_broken_snapshot(exe):
    """a truncated and an empty binary: {error, 'invalid argument'}, and the
    handle steps on as its twin; snapshot/1's binary failing to allocate"""
    with N.Beam(exe, timeout=TIMEOUT) as b:
        cfg = default_config(n_nodes=65, seed=7)
        plain, tried = N.NifSim(b, cfg), N.NifSim(b, cfg)
        for s in (plain, tried):
            _grow(s, 65)
        assert b.call("!fail alloc_binary 1") == "ok"
        assert b.call(f"snapshot {tried.h}") == ("error", N.STRERROR[-2])
        assert b.live()[:2] == (0, 0)
        snap = b.call(f"snapshot {tried.h}")
        assert snap[0] == "ok" and len(snap[1]) > 65 * 64
        for broken in (snap[1][: len(snap[1]) // 2], snap[1][:-1], b""):
            assert b.call(f"restore {tried.h} {N.hexbin(broken)}") == ("error", N.STRERROR[-1])
        a, c = plain.step(5), tried.step(5)
        N._eq("stats", a, c)
        N._eq("nodes", plain.nodes(), tried.nodes())
        # the whole one still loads, and the rounds repeat
        assert b.call(f"restore {tried.h} {N.hexbin(snap[1])}") == "ok"
        N._eq("stats after restore", tried.step(5), a)
        b.finish_clean()


# ---------------------------------------------------------------- the host-exchange handle
WORLD, RANKS = 4, (1, 3)          # the engine plays ranks 1 and 2 of 4, as tests/_random_schedule.HYBRID


class _Shard:
    """an oracle shard answering in the projection's terms"""

    def __init__(self, cfg, rank):
        self.o = OracleShard(cfg, WORLD, rank)
        self.lo, self.hi = self.o.lo, self.o.hi

    def nodes(self, first, count): return N._node_rows(self.o.nodes(first, count), self.o.round)
    def strategy_nodes(self, first, count): return N._project("strategy_nodes", self.o.strategy_nodes(first, count), 0, False)
    def delivery(self, first, count): return self.o.delivery(first, count)


class NifHybrid:
    """The parties of tests/_hybrid.py's Hybrid with the engine party a
    host-exchange handle behind the shim (round_emit / outbound /
    round_absorb); every answer in the terms of N.project."""

    def __init__(self, beam, cfg):
        n = cfg.n_nodes
        self.beam, self.cfg, self.n = beam, cfg, n
        per = (n + WORLD - 1) // WORLD
        self.lo, self.hi = RANKS[0] * per, min(n, RANKS[1] * per)
        self.engine = self._engine()
        self.parties = [_Shard(cfg, r) for r in range(RANKS[0])] + [self.engine] + \
            [_Shard(cfg, r) for r in range(RANKS[1], WORLD)]
        self.tables = []
        self.n_out = self.n_in = 0

    def _engine(self):
        e = N.NifSim(self.beam, self.cfg, host_lo=self.lo, host_hi=self.hi)
        e.lo, e.hi = self.lo, self.hi
        return e

    def _all(self, name, *a):
        rcs = []
        for p in self.parties:
            try:
                getattr(p if p is self.engine else p.o, name)(*a)
                rcs.append(0)
            except SimError as e:
                rcs.append(e.rc if p is self.engine else N._rc(e.rc))
        assert len(set(rcs)) == 1, f"{name}: the parties disagree: {rcs}"
        if rcs[0] != 0:
            e = SimError(f"{name}: {rcs[0]}")
            e.rc = rcs[0]
            raise e

    def __getattr__(self, name):
        if name in R.ARG_TYPES:
            def call(*a):
                self._all(name, *a)
                if name in R.TABLE_CALLS:
                    self.tables.append((name, a))
            return call
        raise AttributeError(name)

    @property
    def round(self):
        return self.parties[0].o.round

    def _owned(self, name, first, count):
        out = []
        for p in self.parties:
            lo, hi = max(first, p.lo), min(first + count, p.hi)
            if lo < hi:
                out.append(getattr(p, name)(lo, hi - lo))
        return out

    def nodes(self, first, count): return [r for part in self._owned("nodes", first, count) for r in part]
    def strategy_nodes(self, first, count): return [r for part in self._owned("strategy_nodes", first, count) for r in part]

    def delivery(self, first, count):
        parts = self._owned("delivery", first, count)
        return tuple(np.concatenate([x[i] for x in parts]) for i in range(3))

    def msg_slots(self):
        return self.engine.msg_slots()

    def step(self, n_rounds=1):
        assert n_rounds == 1
        r = self.round
        for p in self.parties:
            (p if p is self.engine else p.o).emit()
        boxes = [(p if p is self.engine else p.o).outbound() for p in self.parties]
        mine = boxes[self.parties.index(self.engine)]
        inside = lambda ids: (ids >= self.lo) & (ids < self.hi)      # noqa: E731
        assert not inside(mine[:, 0]).any() and inside(mine[:, 1]).all()
        below, above = mine[mine[:, 0] < self.lo], mine[mine[:, 0] >= self.hi]
        assert np.array_equal(mine, np.concatenate([canonical(below), canonical(above)])), \
            f"round {r}: the outbound list is not in its promised order"
        every = np.concatenate(boxes)
        total = np.zeros(1, N.NIF_STATS_DTYPE)
        for k, p in enumerate(self.parties):
            recs = every[(every[:, 0] >= p.lo) & (every[:, 0] < p.hi)]
            if p is self.engine:
                recs = recs[~inside(recs[:, 1])]
                self.n_out, self.n_in = self.n_out + len(mine), self.n_in + len(recs)
            rng = np.random.Generator(np.random.PCG64([2024, r, k]))
            recs = np.ascontiguousarray(recs[rng.permutation(len(recs))])
            if p is self.engine:
                st = p.absorb(recs)
                assert int(st["round"][0]) == r
            else:
                full = p.o.absorb(recs)
                st = np.zeros(1, N.NIF_STATS_DTYPE)
                st["emitted"], st["delivered"] = full["emitted"].sum(), full["delivered"].sum()
                st["first_deliveries"] = full["first_deliveries"]
            for f in ("emitted", "delivered", "first_deliveries"):
                total[f] += st[f]
        total["round"] = r
        return total

    def close(self):
        for p in self.parties:
            if p is not self.engine:
                p.o.close()


def _hybrid_restore(hy, fresh):
    """the engine's state moves to a second host-exchange handle of the program"""
    snap = hy.engine.snapshot()
    other = hy._engine()
    for name, a in hy.tables:
        getattr(other, name)(*a)
    other.restore(snap)
    hy.parties[hy.parties.index(hy.engine)] = other
    hy.engine = other
    return hy


@pytest.mark.parametrize("kind,seed", [("hv", 2), ("scamp_v2", 2)])
def test_host_exchange_handle(exe, kind, seed):
    """a handle made with host_lo / host_hi, driven by round_emit / outbound /
    round_absorb among oracle shards, equals the unsharded oracle"""
    sch, want = _want(kind, seed, host=True)
    holder = []
    with N.Beam(exe, timeout=TIMEOUT) as b:
        def make(cfg):
            holder.append(NifHybrid(b, cfg))
            return holder[-1]
        got = R.execute(make, sch, R.Opts(drop=("histograms",), single_rounds=True, restore=_hybrid_restore))
        assert b.call(f"step {holder[0].engine.h} 1") == ("error", N.STRERROR[-7])
        b.finish_clean()
    assert got.restored >= 1 and holder[0].n_out > 0 and holder[0].n_in > 0
    N.same(got, want)


# ---------------------------------------------------------------- busy
def test_busy_with_a_step_on_a_second_thread(exe):
    with N.Beam(exe, timeout=TIMEOUT) as b:
        N.busy_two_threads(b, Oracle)
        b.finish_clean()
