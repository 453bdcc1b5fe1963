"""A party set over `world` equal id ranges, driven like one simulator (test
infrastructure of the host boundary, tests/test_gpu_host_exchange.py).

The id space is cut as orc_create cuts it for shard ranks: per = ceil(n /
world), rank r owns [r per, min(n, (r + 1) per)).  The engine -- one HostSim,
a host-exchange handle -- owns the ranks [r0, r1); every other rank is an
oracle shard (shard_world = world, shard_rank = r) playing the outside nodes.
engine=False plays the engine's ranks with oracle shards too: the expected
side of the exchange check, and the check that the protocol itself equals
the unsharded oracle.

Hybrid(cfg, parties=[(lo, hi, ENGINE | ORACLE), ...]) takes explicit ranges
instead (tests/_high_ids.py: id windows far from 0): an oracle party is an
orc_create_range handle, ids in no party's range are never started, and a
record addressed to one fails the run.  One party alone is the one-party
driver: nothing may leave it, so its outbound list is empty every round.

Every party gets every event call.  A round: every party emits; the records
are dealt by destination; every party's import is shuffled by a seeded
permutation; every party absorbs; the stats are summed, `round` from one.

Records here are in the wire codec's word order (dst, src, type word, seq,
a0..a3, ex[8]); the oracle packs seq before the type word, swapped at its
door."""
import ctypes as C

import numpy as np

from _oracle import Oracle
from partisan_amd import _abi
from partisan_amd.sim import SimError, _Driver


def _swap23(recs):
    out = np.ascontiguousarray(recs, np.uint32).reshape(-1, 16).copy()
    out[:, [2, 3]] = out[:, [3, 2]]
    return out


def canonical(recs):
    """(src, seq) order"""
    return recs[np.lexsort((recs[:, 3], recs[:, 1]))]


def _first_diff(a, b):
    if a.shape != b.shape:
        return f"{len(a)} records against {len(b)}"
    k = int(np.nonzero((a != b).any(1))[0][0])
    return f"record {k}: {a[k].tolist()} against {b[k].tolist()}"


class _Rounds:
    """a round in its two halves (orc_round_emit / orc_get_outbox /
    orc_round_absorb)"""
    _st = None

    def emit(self):
        self._st = np.zeros(1, _abi.STATS_DTYPE)
        assert self._lib.orc_round_emit(self._h, self._st.ctypes.data) == 0

    def outbound(self):
        """every record the party emitted, its own range's included"""
        n = C.c_size_t()
        self._lib.orc_get_outbox(self._h, None, 0, C.byref(n))
        box = np.zeros((n.value, 16), np.uint32)
        self._lib.orc_get_outbox(self._h, box.ctypes.data, n.value, C.byref(n))
        return _swap23(box)

    def absorb(self, recs):
        r = _swap23(recs)
        assert self._lib.orc_round_absorb(self._h, r.ctypes.data, r.shape[0]) == 0
        return self._st


class OracleShard(_Rounds, Oracle):
    """One rank of the oracle's sharded protocol: orc_create's equal cut."""

    def __init__(self, cfg, world, rank):
        c = type(cfg).from_buffer_copy(cfg)
        c.comm_id = None
        c.shard_world, c.shard_rank = world, rank
        super().__init__(c)
        per = (cfg.n_nodes + world - 1) // world
        self.lo, self.hi = min(cfg.n_nodes, rank * per), min(cfg.n_nodes, (rank + 1) * per)


class OracleRange(_Rounds, Oracle):
    """An oracle that owns the ids [lo, hi) of cfg.n_nodes (orc_create_range)."""

    def __init__(self, cfg, lo, hi):
        c = type(cfg).from_buffer_copy(cfg)
        c.comm_id = None
        c.shard_world, c.shard_rank = 1, 0
        super().__init__(c, lo, hi)


ENGINE, ORACLE = "engine", "oracle"


class Hybrid:
    """Hybrid(cfg, world, ranks): the equal cut of the module's head.
    Hybrid(cfg, parties=[(lo, hi, ENGINE | ORACLE), ...]): explicit ranges in
    id order, at most one of them the engine's (engine=False: an OracleRange
    plays it, and the trace is still that range's).  Ids in no party's range
    are never started: a record addressed to one fails the run."""

    def __init__(self, cfg, world=None, ranks=None, engine=True, seed=2024, expect=None, resume_at=None, probes=None,
                 on_outbound=None, parties=None, on_records=None):
        from partisan_amd.sim import HostSim

        n = cfg.n_nodes
        self.cfg, self.n, self.world = cfg, n, world
        self._seed = seed
        self.engine = None
        self.parties = []                    # in id order: each has .lo and .hi
        if parties is None:
            self.per = (n + world - 1) // world
            r0, r1 = ranks
            self.lo, self.hi = r0 * self.per, min(n, r1 * self.per)
            self.first, self.end = 0, n
            for r in range(world):
                if r0 <= r < r1 and engine:
                    if r == r0:
                        self.engine = HostSim(type(cfg).from_buffer_copy(cfg), self.lo, self.hi)
                        self.parties.append(self.engine)
                else:
                    self.parties.append(OracleShard(cfg, world, r))
        else:
            assert all(a[0] < a[1] <= b[0] for a, b in zip(parties, parties[1:])) and parties[-1][0] < parties[-1][1] <= n
            mine = [p for p in parties if p[2] == ENGINE]
            assert len(mine) <= 1
            # (no engine range: the first party's is the one the trace follows)
            self.lo, self.hi = (mine or parties)[0][:2]
            self.first, self.end = parties[0][0], parties[-1][1]
            for lo, hi, kind in parties:
                if kind == ENGINE and engine:
                    self.engine = HostSim(type(cfg).from_buffer_copy(cfg), lo, hi)
                    self.parties.append(self.engine)
                else:
                    self.parties.append(OracleRange(cfg, lo, hi))
        # the exchange of every round, as this run saw it: the records that
        # left [lo, hi) -- those for ids below first, then those for ids at or
        # above, each side in (src, seq) order -- and the ones that entered it
        self.trace = []
        self.expect = expect                 # another run's trace: compared round by round
        self.resume_at, self.probes, self.on_outbound = resume_at, probes or {}, on_outbound
        self.n_out = self.n_in = 0
        self.resumed = False
        self.tables = []
        self.on_records = on_records         # on_records(round, every record of the round)

    # ---- events: every party makes the same call
    def _all(self, name, *a):
        """a call one party refuses every party refuses, with the same code:
        raised once every party has been asked"""
        errs = []
        for p in self.parties:
            try:
                getattr(p, name)(*a)
            except SimError as e:
                errs.append(e)
        if errs:
            assert len(errs) == len(self.parties) and len({e.rc for e in errs}) == 1, \
                f"{name}: the parties disagree: {[str(e) for e in errs]}"
            raise errs[0]

    def join(self, nodes, contacts): self._all("join", nodes, contacts)
    def crash(self, nodes): self._all("crash", nodes)
    def revive(self, nodes): self._all("revive", nodes)
    def leave(self, nodes): self._all("leave", nodes)
    def set_partition(self, group): self._all("set_partition", group)
    def clear_partition(self): self._all("clear_partition")
    def broadcast(self, root, msg_id): self._all("broadcast", root, msg_id)
    def begin_omission(self, nodes): self._all("begin_omission", nodes)
    def end_omission(self, nodes): self._all("end_omission", nodes)
    def begin_send_omission(self, src, dst): self._all("begin_send_omission", src, dst)
    def end_send_omission(self, src, dst): self._all("end_send_omission", src, dst)
    def begin_receive_omission(self, src, dst): self._all("begin_receive_omission", src, dst)
    def end_receive_omission(self, src, dst): self._all("end_receive_omission", src, dst)
    def resolve_all_faults(self): self._all("resolve_all_faults")

    # (the view-order tables are kept: a handle that takes over the engine's
    # state needs them before its restore)
    def set_bucket_table(self, buckets):
        self._all("set_bucket_table", buckets)
        self.tables.append(("set_bucket_table", buckets))

    def set_phash_table(self, phash):
        self._all("set_phash_table", phash)
        self.tables.append(("set_phash_table", phash))

    # ---- inspection: each party answers for the ids it owns
    def _owned(self, name, first, count):
        first = self.first if first is None else first
        count = self.end - first if count is None else count
        parts = []
        for p in self.parties:
            lo, hi = max(first, p.lo), min(first + count, p.hi)
            if lo < hi:
                parts.append(getattr(p, name)(lo, hi - lo))
        return parts

    def nodes(self, first=None, count=None):
        return np.concatenate(self._owned("nodes", first, count))

    def strategy_nodes(self, first=None, count=None):
        return np.concatenate(self._owned("strategy_nodes", first, count))

    def delivery(self, first=None, count=None):
        p = self._owned("delivery", first, count)
        return tuple(np.concatenate([x[i] for x in p]) for i in range(3))

    def msg_slots(self):
        """host state, the same at every party"""
        out = [p.msg_slots() for p in self.parties]
        for o in out[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(o, out[0])), "the parties disagree on the message slots"
        return out[0]

    @property
    def round(self):
        return self.parties[0].round

    run_schedule = _Driver.run_schedule

    def _inside(self, ids):
        return (ids >= self.lo) & (ids < self.hi)

    def _round(self):
        r = self.round
        for p in self.parties:
            p.emit()
        boxes = []
        for p in self.parties:
            box = p.outbound()
            if p is self.engine:
                assert not self._inside(box[:, 0]).any(), "an owned destination in the outbound list"
                assert self._inside(box[:, 1]).all()
                if self.on_outbound is not None:
                    self.on_outbound(r, box)
            boxes.append(box)
        # what crossed the engine range's boundary, from the senders' side
        every = np.concatenate(boxes)
        held = np.zeros(len(every), bool)
        for p in self.parties:
            held |= (every[:, 0] >= p.lo) & (every[:, 0] < p.hi)
        assert held.all(), f"round {r}: a record for an id no party owns: {every[~held][0].tolist()}"
        if self.on_records is not None:
            self.on_records(r, every)
        src_in, dst_in = self._inside(every[:, 1]), self._inside(every[:, 0])
        out = every[src_in & ~dst_in]
        out = np.concatenate([canonical(out[out[:, 0] < self.lo]), canonical(out[out[:, 0] >= self.hi])])
        inn = canonical(every[~src_in & dst_in])
        if self.engine is not None:
            # (the engine's own list, in the order it gave it)
            mine = boxes[self.parties.index(self.engine)]
            assert np.array_equal(mine, out), f"round {r}: the outbound list is not in its promised order"
        self.trace.append((out, inn))
        self.n_out += len(out)
        self.n_in += len(inn)
        if self.expect is not None:
            eo, ei = self.expect[r]
            assert np.array_equal(out, eo), f"round {r}: outbound records differ from the all-oracle exchange: " + \
                _first_diff(out, eo)
            assert np.array_equal(inn, ei), f"round {r}: records for the engine differ from the all-oracle " + \
                "exchange: " + _first_diff(inn, ei)
        total = None
        for k, p in enumerate(self.parties):
            mine = every[(every[:, 0] >= p.lo) & (every[:, 0] < p.hi)]
            if p is self.engine:
                mine = mine[~self._inside(mine[:, 1])]     # (its own records never left it)
            rng = np.random.Generator(np.random.PCG64([self._seed, r, k]))
            mine = np.ascontiguousarray(mine[rng.permutation(len(mine))])
            if p is self.engine and r in self.probes:
                self.probes[r](p, mine)
            st = p.absorb(mine)
            flat = st.view(np.uint64).copy()
            total = flat if total is None else total + flat
        total[0] = r                                        # (the round number is not summed)
        if self.engine is not None and self.resume_at is not None and self.round == self.resume_at:
            self._resume()
        return total.view(_abi.STATS_DTYPE)

    def _resume(self):
        """the engine's state moves to a fresh handle of the same range"""
        from partisan_amd.sim import HostSim

        snap = self.engine.snapshot()
        other = HostSim(type(self.cfg).from_buffer_copy(self.cfg), self.lo, self.hi)
        other.restore(snap)
        k = self.parties.index(self.engine)
        self.engine.close()
        self.engine = self.parties[k] = other
        self.resumed = True

    def step(self, n_rounds=1):
        return np.concatenate([self._round() for _ in range(n_rounds)])

    def close(self):
        for p in self.parties:
            p.close()
