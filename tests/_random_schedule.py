"""Seeded random event schedules: a generator, an executor and a comparer, kept
apart, plus a replay and shrink tool run by hand (python -m
tests._random_schedule, below).

generate(kind, seed) is a pure function: it touches no driver and draws from
np.random.Generator(np.random.PCG64([seed, TAG])).  A Schedule is plain data --
a config dict and a list of steps, arrays as lists -- so it dumps to JSON and
loads back unchanged.  A step is one of

    ("call", name, args)            an event call of the ABI; refusals are wanted
    ("step", k)                     k rounds in one psim_step
    ("probe", what, first, count)   a getter over the window [first, first + count)
    ("snapshot_restore",)           move the run to a second handle (the executor
                                    decides how; the oracle ignores it)

The generator keeps a rough picture of which nodes are up (exact for the
refusals it provokes on purpose: a second start of a node in one round, a
second broadcast of a root or a message slot, a second leave/1 of an actor, a
restart on a full-membership handle), so that crashes leave at least a quarter
of the started nodes up and about half of the crashed ones come back.

execute(make, schedule, opts) applies the steps to any _Driver-like object and
returns a Trace: every round's stats, every event call's return code, every
probe's result, the final state.  compare(a, b) names the seed, the first
differing round, call or probe, and the field.

What the paths cannot do is decided here, in Opts, never silently:
  * full-membership handles run on one shard only (psim_create refuses more);
  * rank handles (loopback, RCCL) have no windowed getter across ranks other
    than what tests/_loopback.py assembles; the one-rank RCCL handle answers
    every getter itself;
  * host-exchange schedules are generated with host=True: no leave_node and no
    histogram probe (both need a collective across the parties), every
    ("step", k) becomes k emit/absorb rounds, and every getter is assembled
    from the parties that own the ids of its window (tests/_hybrid.py)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _scenarios as S  # noqa: E402
from partisan_amd import _abi  # noqa: E402
from partisan_amd.sim import SimError, default_config  # noqa: E402
from partisan_amd.workloads import NONE  # noqa: E402

TAG = 0x52A7D
KINDS = ("hv", "xbot", "scamp_v1", "scamp_v2", "full")
ROUNDS = 90
STEP_SIZES = (1, 1, 1, 2, 3, 5, 8)
SIZES = (65, 257, 509, 1021)
FULL_FLOOD_N = 17           # the one size at which full-membership handles run with fanout 0
MANAGER = {"hv": (0, 0), "xbot": (2, 0), "full": (1, 0), "scamp_v1": (1, 1), "scamp_v2": (1, 2)}
OMISSION_CALLS = ("begin_omission", "end_omission", "begin_send_omission", "end_send_omission",
                  "begin_receive_omission", "end_receive_omission")
TABLE_CALLS = ("set_bucket_table", "set_phash_table")
# the event calls a kind's corpus must make, and have accepted, at least once
COMMON_CALLS = ("join", "crash", "revive", "set_partition", "clear_partition")
CALLS = {
    "hv": COMMON_CALLS + ("broadcast",),
    "xbot": COMMON_CALLS + ("broadcast",),
    "scamp_v1": COMMON_CALLS + ("leave", "leave_node", "resolve_all_faults") + OMISSION_CALLS,
    "scamp_v2": COMMON_CALLS + ("leave", "leave_node", "resolve_all_faults") + OMISSION_CALLS,
    # (leave_node: SCAMP schedules only, as the corpus is specified)
    "full": COMMON_CALLS + ("leave", "resolve_all_faults") + OMISSION_CALLS,
}
PROBES = {
    "hv": ("nodes", "delivery", "msg_slots", "histograms", "round"),
    "xbot": ("nodes", "delivery", "msg_slots", "histograms", "round"),
    "scamp_v1": ("strategy_nodes", "round"),
    "scamp_v2": ("strategy_nodes", "round"),
    "full": ("strategy_nodes", "member_bits", "round"),
}
# the corpus: about ten seeds a kind, chosen so that the conditions of
# tests/test_random_schedule.py hold on the oracle
CORPUS_SEEDS = {
    "hv": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10),
    # (seeds 3 and 8 count overflows too: at most two schedules a kind may)
    "xbot": (1, 2, 4, 5, 6, 7, 9, 10, 11, 12),
    "scamp_v1": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10),
    "scamp_v2": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10),
    "full": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10),
}
CORPUS = [(k, s) for k in KINDS for s in CORPUS_SEEDS[k]]


def is_pl(kind):
    return kind in ("scamp_v1", "scamp_v2", "full")


# ---------------------------------------------------------------- the data
class Schedule:
    def __init__(self, kind, seed, config, steps, host=False):
        self.kind, self.seed, self.config, self.host = kind, int(seed), dict(config), bool(host)
        self.steps = [_as_step(s) for s in steps]

    @property
    def n(self):
        return self.config["n_nodes"]

    def to_dict(self):
        return {"kind": self.kind, "seed": self.seed, "host": self.host, "config": self.config,
                "steps": [list(s) for s in self.steps]}

    def to_json(self):
        """canonical: what the pinned hash is taken of"""
        return json.dumps(self.to_dict(), sort_keys=True, separators=(",", ":"))

    @classmethod
    def from_json(cls, text):
        d = json.loads(text) if isinstance(text, str) else text
        return cls(d["kind"], d["seed"], d["config"], d["steps"], d.get("host", False))

    def sha256(self):
        return hashlib.sha256(self.to_json().encode()).hexdigest()

    def __eq__(self, other):
        return isinstance(other, Schedule) and self.to_json() == other.to_json()

    def rounds(self):
        return sum(s[1] for s in self.steps if s[0] == "step")

    def calls(self):
        return [s for s in self.steps if s[0] == "call" and s[1] not in TABLE_CALLS]


def _plain(x):
    if isinstance(x, np.ndarray):
        return [int(v) for v in x.tolist()]
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return int(x)


def _as_step(s):
    s = list(s)
    if s[0] == "call":
        return ("call", str(s[1]), _plain(s[2]))
    if s[0] == "step":
        return ("step", int(s[1]))
    if s[0] == "probe":
        return ("probe", str(s[1]), int(s[2]), int(s[3]))
    assert s[0] == "snapshot_restore", s
    return ("snapshot_restore",)


# ---------------------------------------------------------------- the generator
def _draw_config(rng, kind, n, seed):
    man, strat = MANAGER[kind]
    cfg = {"n_nodes": int(n), "seed": int(seed) * 7919 + 11, "manager": man, "strategy": strat}
    if not is_pl(kind):
        cfg["shuffle_period"] = int(rng.choice([1, 2, 3, 5, 10]))
        cfg["promotion_period"] = int(rng.choice([1, 2, 3, 5]))
        cfg["lazy_tick_period"] = int(rng.integers(1, 4))
        cfg["random_promotion"] = int(rng.random() < 0.8)
        u = rng.random()
        if u < 0.2:
            cfg.update(S.VARIANT)                  # arwl = prwl
        elif u < 0.45:
            a = int(rng.choice([3, 4, 5]))
            cfg.update(max_active_size=a, min_active_size=int(rng.integers(1, a)),
                       max_passive_size=int(rng.choice([6, 12, 17])))
        if kind == "xbot":
            # (a period of 1 to 3 rounds overruns the disconnect-id maps and the
            # connection table throughout: tests/_config_cases.py xbot_p1)
            cfg["xbot_period"] = int(rng.choice([4, 5, 10, 20]))
    else:
        cfg["periodic_interval"] = int(rng.choice([1, 2, 3, 5, 10]))
        cfg["scamp_c"] = int(rng.choice([1, 3, 5, 64]))
        if kind == "full":
            # fanout 0, the reference's gossip to every member, multiplies the
            # message count by |members| a round while states disagree (DESIGN.md
            # section 6): 1.6e7 messages in round 10 of a doubling ramp at 65
            # nodes.  It stays in the domain at FULL_FLOOD_N nodes only.
            cfg["fanout"] = 0 if n <= FULL_FLOOD_N and rng.random() < 0.7 else int(rng.choice([1, 2, 3, 5]))
        else:
            cfg["fanout"] = int(rng.choice([0, 3]))
    return cfg


def _bootstrap(rng, n, m):
    """the join batches that start ids [0, m), one batch before each step"""
    how = str(rng.choice(["doubling", "doubling", "sequential", "star"]))
    out = [(np.array([0]), np.array([NONE]))]
    if how == "doubling":
        lo = 1
        while lo < m:
            hi = min(2 * lo, m)
            out.append((np.arange(lo, hi), rng.integers(0, lo, hi - lo)))
            lo = hi
    elif how == "sequential":
        per = max(1, -(-m // int(rng.integers(12, 31))))
        for lo in range(1, m, per):
            ids = np.arange(lo, min(m, lo + per))
            out.append((ids, ids - 1 if rng.random() < 0.5 else rng.integers(0, lo, ids.size)))
    else:
        # a star on one contact, a few joiners a round (more would overrun the
        # contact's disconnect-id maps: 64 entries)
        c, per = 0, int(rng.integers(8, 25))
        for lo in range(1, m, per):
            ids = np.arange(lo, min(m, lo + per))
            out.append((ids, np.full(ids.size, c)))
    return out


class _Gen:
    """the generator's picture of the run between two steps"""

    def __init__(self, rng, kind, n, host):
        self.rng, self.kind, self.n, self.host = rng, kind, n, host
        self.started = np.zeros(n, bool)
        self.up = np.zeros(n, bool)
        self.steps = []
        self.faults = False          # an omission fault may be installed
        self.partition = False
        self.msg = 0
        self.roots = None
        self.send_pairs, self.recv_pairs, self.general = [], [], []
        self.boot_end = n
        self._new_slot()

    def _new_slot(self):
        self.pend_join, self.pend_root, self.pend_slot, self.pend_actor = set(), set(), set(), set()

    # ---- bookkeeping of one call
    def call(self, name, *args):
        self.steps.append(("call", name, [_plain(a) for a in args]))

    def _ids(self, pool, k):
        pool = np.asarray(pool)
        if pool.size == 0:
            return np.zeros(0, np.int64)
        return np.sort(self.rng.choice(pool, size=min(k, pool.size), replace=False))

    def _some(self, prefer, k, stray=0.15):
        """k ids, mostly from `prefer`; sometimes any id at all (down, never started)"""
        ids = self._ids(np.nonzero(prefer)[0], k)
        if ids.size == 0 or self.rng.random() < stray:
            ids = np.union1d(ids, self._ids(np.arange(self.n), max(1, k // 3)))
        return ids

    def join(self, ids, contacts):
        ids, contacts = np.asarray(ids, np.int64), np.asarray(contacts, np.int64)
        self.call("join", ids, contacts)
        self._joined(ids)

    def _joined(self, ids):
        lst = [int(x) for x in ids]
        if len(set(lst)) != len(lst) or self.pend_join & set(lst):
            return                                    # refused: a second start in one round
        if self.kind == "full" and self.started[ids].any():
            return                                    # refused: no restart on a full handle
        self.pend_join |= set(lst)
        self.started[ids] = True
        self.up[ids] = True

    # ---- the event calls
    def ev_crash(self):
        up_n, st_n = int(self.up.sum()), int(self.started.sum())
        room = up_n - max(2, (st_n + 1) // 3 + 1)      # (a third: slack for stops the picture misses)
        if self.kind == "full":
            room = up_n - (self.n * 2 // 5 + 1)         # (no restart on a full handle: what goes down stays down)
            if room <= 0:
                return self.ev_partition()
        if room <= 0:
            return self.ev_revive()
        k = int(self.rng.integers(1, max(2, min(room, self.n // 16) + 1)))
        ids = self._some(self.up, min(k, room))
        name = "leave" if is_pl(self.kind) and self.rng.random() < 0.35 else "crash"
        self.call(name, ids)
        self.up[ids] = False

    def ev_revive(self):
        down = self.started & ~self.up
        ids = self._some(down, int(self.rng.integers(1, max(2, int(down.sum()) // 2 + 1))), stray=0.1)
        self.call("revive", ids)
        self._joined(ids)

    def ev_join(self):
        r = self.rng
        down = ~self.up if r.random() < 0.4 else self.started & ~self.up
        if self.kind == "full":
            # (the ids the bootstrap left out; a stray started one has the call refused)
            down = ~self.started & (np.arange(self.n) >= self.boot_end)
        ids = self._some(down, int(r.integers(1, max(2, min(int(down.sum()), self.n // 16) + 1))), stray=0.1)
        if self.pend_join and r.random() < 0.12:
            ids = np.union1d(ids, [int(r.choice(sorted(self.pend_join)))])    # a second start this round
        ups = np.nonzero(self.up)[0]
        contacts = r.choice(ups, size=ids.size) if ups.size else np.zeros(ids.size, np.int64)
        odd = r.random(ids.size) < 0.15                 # contacts drawn freely: down, self, never started
        free = r.integers(0, self.n, ids.size)
        free = np.where(r.random(ids.size) < 0.3, ids, free)
        self.join(ids, np.where(odd, free, contacts))

    def ev_partition(self):
        r = self.rng
        if self.partition and r.random() < 0.45:
            self.call("clear_partition")
            self.partition = False
            return
        g = int(r.integers(2, 5))
        how = r.random()
        ids = np.arange(self.n)
        if how < 0.4:
            grp = ids * g // self.n
        elif how < 0.7:
            grp = ids % g
        else:
            grp = r.integers(0, g, self.n)
        if r.random() < 0.35:
            grp = np.where(r.random(self.n) < 0.1, 254, grp)
        self.call("set_partition", grp)
        self.partition = True

    def _bcast(self, root, msg):
        self.call("broadcast", root, msg)
        if root in self.pend_root or msg % _abi.MSG_SLOTS in self.pend_slot:
            return
        self.pend_root.add(root)
        self.pend_slot.add(msg % _abi.MSG_SLOTS)

    def ev_broadcast(self):
        r = self.rng
        if self.roots is None:
            started = np.nonzero(self.started)[0]
            self.roots = [int(x) for x in self._ids(started, 6)] or [0]
        if r.random() < 0.2:
            # a heartbeat-like burst: several roots in one round, ids counting up
            for root in self._ids(np.array(self.roots), int(r.integers(2, _abi.PT_ROOTS + 1))):
                self.msg += 1
                self._bcast(int(root), self.msg % 0x10000)
            return
        root = int(r.choice(self.roots))
        u = r.random()
        if u < 0.08 and self.pend_slot:
            msg = int(r.choice(sorted(self.pend_slot))) + _abi.MSG_SLOTS * int(r.integers(1, 4))   # a slot taken
        else:
            self.msg += int(r.integers(1, 4))
            msg = self.msg % 0x10000
        self._bcast(root, msg)

    def ev_leave_node(self):
        r = self.rng
        k = int(r.integers(1, 4))
        actors = self._ids(np.nonzero(self.up)[0], k)
        if actors.size == 0:
            return
        if self.pend_actor and r.random() < 0.15:
            actors = np.union1d(actors, [int(r.choice(sorted(self.pend_actor)))])
        targets = r.integers(0, self.n, actors.size)
        targets = np.where(r.random(actors.size) < 0.1, actors, targets)      # (actor == target: leave/0)
        self.call("leave_node", actors, targets)
        if not (self.pend_actor & set(int(a) for a in actors)):
            self.pend_actor |= set(int(a) for a in actors)
            self.up[targets[targets == actors]] = False

    def ev_fault(self):
        r = self.rng
        u = r.random()

        def pairs():
            k = int(r.integers(1, max(2, self.n // 32)))
            s = self._some(self.up, k, stray=0.1)
            return s, (s + 1 + r.integers(0, self.n - 1, s.size)) % self.n

        if self.faults and u < 0.2:
            self.call("resolve_all_faults")
            self.send_pairs, self.recv_pairs, self.general = [], [], []
            self.faults = False
            return
        self.faults = True
        if u < 0.4:
            ids = self._some(self.up, int(r.integers(1, max(2, self.n // 32))), stray=0.1)
            self.call("begin_omission", ids)
            self.general.append(ids)
        elif u < 0.55:
            s, d = pairs()
            self.call("begin_send_omission", s, d)
            self.send_pairs.append((s, d))
        elif u < 0.7:
            s, d = pairs()
            self.call("begin_receive_omission", s, d)
            self.recv_pairs.append((s, d))
        elif u < 0.8 and self.general:
            ids = self.general.pop(int(r.integers(0, len(self.general))))
            self.call("end_omission", ids[: max(1, ids.size // 2 + 1)])
        elif u < 0.9 and self.send_pairs:
            s, d = self.send_pairs.pop(int(r.integers(0, len(self.send_pairs))))
            self.call("end_send_omission", s, d)
        elif self.recv_pairs:
            s, d = self.recv_pairs.pop(int(r.integers(0, len(self.recv_pairs))))
            self.call("end_receive_omission", s, d)
        else:
            ids = self._some(self.up, 2, stray=0.3)
            self.call("end_omission", ids)               # (ends a fault nobody began)

    def event(self):
        r = self.rng
        down = int((self.started & ~self.up).sum())
        table = [(self.ev_crash, 3.0), (self.ev_partition, 1.2)]
        if self.kind == "full":
            # (no restart on a full handle: a few tries stay, to be refused alike)
            table += [(self.ev_join, 1.5 if (~self.started).any() else 0.1), (self.ev_revive, 0.1)]
        else:
            table += [(self.ev_join, 1.5 + 0.1 * min(down, 20)), (self.ev_revive, 0.6 + 0.05 * min(down, 20))]
        if is_pl(self.kind):
            table += [(self.ev_fault, 2.2)]
            if self.kind != "full" and not self.host:
                table += [(self.ev_leave_node, 0.8)]
        else:
            table += [(self.ev_broadcast, 4.0)]
        w = np.array([x[1] for x in table])
        table[int(r.choice(len(table), p=w / w.sum()))][0]()

    # ---- probes
    def probe(self):
        r, n = self.rng, self.n
        what = str(r.choice(PROBES[self.kind]))
        if self.host and what == "histograms":
            what = "nodes"
        if what in ("msg_slots", "histograms", "round"):
            return self.steps.append(("probe", what, 0, 0))
        if what == "member_bits":
            return self.steps.append(("probe", what, int(r.integers(0, n)), 1))
        u = r.random()
        if u < 0.15:
            first, count = 0, n
        elif u < 0.6:
            # a window across a shard or rank boundary (3, 4 and 7 parts)
            parts = int(r.choice([3, 4, 7]))
            per = -(-n // parts)
            edge = per * int(r.integers(1, parts))
            edge = min(edge, n - 1)
            first = max(0, edge - int(r.integers(1, 40)))
            count = min(n - first, edge - first + int(r.integers(1, 40)))
        else:
            first = int(r.integers(0, n))
            count = int(r.integers(1, n - first + 1))
        self.steps.append(("probe", what, first, count))


def generate(kind, seed, host=False, rounds=ROUNDS):
    """The schedule of (kind, seed).  host=True: a schedule a host-exchange
    handle can run (no leave_node, no histogram probe)."""
    assert kind in KINDS, kind
    rng = np.random.Generator(np.random.PCG64([int(seed), TAG]))
    sizes = (FULL_FLOOD_N, 65, 257) if kind == "full" else SIZES
    n = int(rng.choice(sizes))
    cfg = _draw_config(rng, kind, n, seed)
    g = _Gen(rng, kind, n, host)
    # sometimes a view-order table
    u = rng.random()
    if u < 0.3:
        g.call("set_bucket_table", S.random_buckets(n, int(seed)))
    elif u < 0.6 and kind == "scamp_v1":
        g.call("set_phash_table", S.random_phash(n, int(seed)))
    # the bootstrap leaves some ids for later joins
    m = n if rng.random() < 0.4 and kind != "full" else max(2, int(n * rng.uniform(0.7, 0.95)))
    g.boot_end = m
    boot = _bootstrap(rng, n, m)
    ev_from = int(rng.integers(2, 13))
    snaps = sorted(int(x) for x in rng.integers(15, rounds - 8, int(rng.integers(1, 3))))
    done = 0
    while done < rounds:
        if boot:
            ids, contacts = boot.pop(0)
            if kind == "full":                      # (an id a stray join started cannot start again)
                keep = ~g.started[ids]
                ids, contacts = ids[keep], contacts[keep]
            if ids.size:
                g.join(ids, contacts)
        if done >= ev_from:
            for _ in range(int(rng.integers(0, 5))):
                g.event()
            if snaps and done >= snaps[0] and g.faults:
                # a restore point is due and faults are installed (host state no
                # snapshot holds): they are resolved first, the restore follows
                # the round that applies it
                g.call("resolve_all_faults")
                g.send_pairs, g.recv_pairs, g.general, g.faults = [], [], [], False
        k = min(int(rng.choice(STEP_SIZES)), rounds - done)
        g.steps.append(("step", k))
        done += k
        g._new_slot()
        if rng.random() < 0.4:
            for _ in range(int(rng.integers(1, 3))):
                g.probe()
        if snaps and done >= snaps[0] and not g.faults and done < rounds:
            g.steps.append(("snapshot_restore",))
            snaps.pop(0)
    return Schedule(kind, seed, cfg, g.steps, host=host)


# ---------------------------------------------------------------- the executor
_U32, _U8 = np.uint32, np.uint8
ARG_TYPES = {
    "join": (_U32, _U32), "crash": (_U32,), "revive": (_U32,), "leave": (_U32,), "leave_node": (_U32, _U32),
    "set_partition": (_U8,), "clear_partition": (), "broadcast": (int, int), "resolve_all_faults": (),
    "begin_omission": (_U32,), "end_omission": (_U32,),
    "begin_send_omission": (_U32, _U32), "end_send_omission": (_U32, _U32),
    "begin_receive_omission": (_U32, _U32), "end_receive_omission": (_U32, _U32),
    "set_bucket_table": (_U8,), "set_phash_table": (_U32,),
}


def _args(name, args):
    types = ARG_TYPES[name]
    assert len(types) == len(args), (name, args)
    return [int(a) if t is int else np.array(a, dtype=t) for t, a in zip(types, args)]


class Opts:
    """How a path honours what it cannot do as written.
    drop: probe kinds left out on this path; restore(sim, fresh) -> sim: how
    ("snapshot_restore",) is honoured, None: ignored (the oracle);
    single_rounds: ("step", k) as k calls of one round."""

    def __init__(self, drop=(), restore=None, single_rounds=False):
        self.drop, self.restore, self.single_rounds = frozenset(drop), restore, single_rounds


def resume_into_second_handle(sim, fresh):
    """snapshot, a second handle with the same config and tables, restore into
    it, close the first, go on with the second"""
    snap = sim.snapshot()
    other = fresh()
    other.restore(snap)
    sim.close()
    return other


class Trace:
    def __init__(self, schedule):
        self.schedule = schedule
        self.stats = None
        self.rcs = []            # (index of the step, name, return code)
        self.probes = []         # (index of the step, what, first, count, round, result)
        self.final = {}
        self.restored = 0
        self.seconds = 0.0

    def copy(self):
        import copy
        t = Trace(self.schedule)
        t.stats = self.stats.copy()
        t.rcs = list(self.rcs)
        t.probes = copy.deepcopy(self.probes)
        t.final = copy.deepcopy(self.final)
        return t

    def digest(self):
        return int(self.stats["digest"].sum(dtype=np.uint64))


def _probe(sim, what, first, count, n):
    if what == "round":
        return int(sim.round)
    if what == "msg_slots":
        return tuple(np.asarray(x).copy() for x in sim.msg_slots())
    if what == "histograms":
        return {k: np.asarray(v).copy() for k, v in sim.histograms().items()}
    if what == "member_bits":
        return sim.member_bits(first).copy()
    if what == "delivery":
        return tuple(np.asarray(x).copy() for x in sim.delivery(first, count))
    assert what in ("nodes", "strategy_nodes"), what
    return getattr(sim, what)(first, count).copy()


def full_bits_nodes(n):
    return sorted({0, n // 2, n - 1})


def execute(make, schedule, opts=None):
    """Apply the schedule to make(cfg).  Returns the Trace; the handle is closed."""
    opts = opts or Opts()
    tr = Trace(schedule)
    tables = []

    def fresh():
        sim = make(default_config(**schedule.config))
        for name, args in tables:
            getattr(sim, name)(*_args(name, args))
        return sim

    t0 = time.perf_counter()
    sim = make(default_config(**schedule.config))
    stats = []
    try:
        for i, s in enumerate(schedule.steps):
            if s[0] == "call":
                name, args = s[1], s[2]
                try:
                    getattr(sim, name)(*_args(name, args))
                    rc = 0
                except SimError as e:
                    rc = e.rc
                if name in TABLE_CALLS:
                    assert rc == 0, (name, rc)
                    tables.append((name, args))
                else:
                    tr.rcs.append((i, name, rc))
            elif s[0] == "step":
                if opts.single_rounds:
                    for _ in range(s[1]):
                        stats.append(sim.step(1))
                else:
                    stats.append(sim.step(s[1]))
            elif s[0] == "probe":
                what, first, count = s[1], s[2], s[3]
                if what in opts.drop:
                    continue
                tr.probes.append((i, what, first, count, int(sim.round), _probe(sim, what, first, count, schedule.n)))
            elif opts.restore is not None:
                sim = opts.restore(sim, fresh)
                tr.restored += 1
        tr.stats = np.concatenate(stats) if stats else np.zeros(0, _abi.STATS_DTYPE)
        first, count = 0, schedule.n
        if is_pl(schedule.kind):
            tr.final["strategy_nodes"] = sim.strategy_nodes(first, count).copy()
            if schedule.kind == "full":
                for node in full_bits_nodes(schedule.n):
                    tr.final[f"member_bits[{node}]"] = sim.member_bits(node).copy()
        else:
            tr.final["nodes"] = sim.nodes(first, count).copy()
            tr.final["delivery"] = tuple(np.asarray(x).copy() for x in sim.delivery(first, count))
            if "histograms" not in opts.drop:
                tr.final["histograms"] = {k: np.asarray(v).copy() for k, v in sim.histograms().items()}
    finally:
        sim.close()
    tr.seconds = time.perf_counter() - t0
    return tr


# ---------------------------------------------------------------- the comparer
def _same(what, a, b):
    """AssertionError naming the field that differs"""
    if isinstance(a, np.ndarray) and a.dtype.names:
        assert a.shape == b.shape, f"{what}: {a.shape} rows against {b.shape}"
        S.compare_nodes(a, b)           # (also S.compare_strategy's row check, on views already read)
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), f"{what}: keys differ"
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{what} field {k}: {a[k]} against {b[k]}"
    elif isinstance(a, tuple):
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            if not np.array_equal(x, y):
                bad = np.nonzero(np.asarray(x) != np.asarray(y))[0][:8].tolist() if np.shape(x) == np.shape(y) else "shape"
                raise AssertionError(f"{what} array {k} differs at {bad}")
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), f"{what} differs at words {np.nonzero(a != b)[0][:8].tolist()}"
    else:
        assert a == b, f"{what}: {a} against {b}"


def compare(a, b):
    """Trace a (the side under test) against trace b (the reference).  Raises
    an AssertionError that names the seed, the first differing round, call or
    probe, and the field.  Probes are matched by step index: a probe one side
    dropped (Opts.drop) is not compared."""
    sch = a.schedule
    tag = f"schedule {sch.kind} seed {sch.seed}"
    try:
        S.compare_stats(a.stats, b.stats)
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from None
    assert len(a.rcs) == len(b.rcs), f"{tag}: {len(a.rcs)} event calls against {len(b.rcs)}"
    for (i, name, ra), (_, _, rb) in zip(a.rcs, b.rcs):
        assert ra == rb, f"{tag}: step {i}, call {name}: return code {ra} against {rb}"
    theirs = {p[0]: p for p in b.probes}
    for i, what, first, count, rnd, res in a.probes:
        if i not in theirs:
            continue
        _, _, bf, bc, brnd, bres = theirs[i]
        where = f"{tag}: probe {what} [{first}, {first + count}) at step {i}, after round {rnd - 1}"
        assert rnd == brnd, f"{where}: taken at round {rnd} against {brnd}"
        assert (bf, bc) == (first, count), where
        try:
            _same(f"probe {what}", res, bres)
        except AssertionError as e:
            raise AssertionError(f"{where}: {e}") from None
    for k in a.final:
        if k not in b.final:
            continue
        try:
            _same(f"final {k}", a.final[k], b.final[k])
        except AssertionError as e:
            raise AssertionError(f"{tag}: final state, {k}: {e}") from None


# ---------------------------------------------------------------- the paths
def oracle_make(cfg):
    from _oracle import Oracle
    return Oracle(cfg)


def gpu_make(n_shards=1):
    def make(cfg):
        from partisan_amd import Simulator
        cfg.device, cfg.n_shards = 0, n_shards
        return Simulator(cfg)
    return make


def loopback_make(world):
    def make(cfg):
        from _loopback import LoopbackRanks
        return LoopbackRanks(cfg, world)
    return make


def rccl1_make(cfg):
    """the rank path on a one-rank RCCL communicator (tests/_knob_run.py)"""
    from partisan_amd import Simulator
    from partisan_amd.sim import comm_id
    c = type(cfg).from_buffer_copy(cfg)
    c.shard_world, c.shard_rank, c.n_shards = 1, 0, 1
    return Simulator(c, comm=comm_id())


HYBRID = (4, (1, 3))      # the engine plays ranks 1 and 2 of 4


def hybrid_make(engine=True, expect=None, holder=None):
    def make(cfg):
        from _hybrid import Hybrid
        hy = Hybrid(cfg, HYBRID[0], HYBRID[1], engine=engine, expect=expect)
        if holder is not None:
            holder.append(hy)
        return hy
    return make


def hybrid_restore(hy, fresh):
    """the engine's state moves to a fresh handle of the same range (the
    oracle shards play on); the view-order tables go to it first"""
    from partisan_amd.sim import HostSim
    snap = hy.engine.snapshot()
    other = HostSim(type(hy.cfg).from_buffer_copy(hy.cfg), hy.lo, hy.hi)
    for name, table in hy.tables:
        getattr(other, name)(table)
    other.restore(snap)
    k = hy.parties.index(hy.engine)
    hy.engine.close()
    hy.engine = hy.parties[k] = other
    hy.resumed = True
    return hy


# path -> (make, Opts); `full` handles run on one shard and one rank only
def path(name, kind="hv"):
    if name == "oracle":
        return oracle_make, Opts()
    if name == "local":
        return gpu_make(1), Opts(restore=resume_into_second_handle)
    if name.startswith("shards"):
        return gpu_make(int(name[6:])), Opts(restore=resume_into_second_handle)
    if name.startswith("loopback"):
        # member_bits is a full handle's, which has no ranks; every other probe
        # is assembled from the owning ranks (tests/_loopback.py)
        return loopback_make(int(name[8:])), Opts(restore=resume_into_second_handle)
    if name == "rccl1":
        # (one communicator a process: the restore step is ignored, as on the oracle)
        return rccl1_make, Opts()
    if name == "oracle-sharded":
        return hybrid_make(engine=False), Opts(drop=("histograms",), single_rounds=True)
    if name == "host-exchange":
        return hybrid_make(engine=True), Opts(drop=("histograms",), single_rounds=True, restore=hybrid_restore)
    raise KeyError(name)


PATHS = ("oracle", "local", "shards3", "shards7", "loopback3", "rccl1", "oracle-sharded", "host-exchange")


def paths_of(kind):
    """the engine paths a kind's handles can be created on"""
    return ("rccl1",) if kind == "full" else ("shards3", "shards7", "loopback3", "rccl1")


# ---------------------------------------------------------------- replay and shrink
def differ(schedule, backends, compare_fn=compare):
    """None if the two backends agree on the schedule, else the message.  Any
    error other than a mismatch (a SimError from a step, a crash) propagates:
    the tool ends at once and never runs a faulting schedule again."""
    (ma, oa), (mb, ob) = (path(x, schedule.kind) for x in backends)
    a, b = execute(ma, schedule, oa), execute(mb, schedule, ob)
    try:
        compare_fn(a, b)
    except AssertionError as e:
        return str(e)
    return None


def _candidates(sch):
    """smaller schedules, the most promising first"""
    steps = sch.steps

    def mk(new_steps, config=None):
        return Schedule(sch.kind, sch.seed, config or sch.config, new_steps, sch.host)
    total = sch.rounds()
    # fewer rounds: cut the tail
    for keep in (total // 2, total * 3 // 4, total - 1):
        if 0 < keep < total:
            out, done = [], 0
            for s in steps:
                if s[0] == "step":
                    if done >= keep:
                        break
                    s = ("step", min(s[1], keep - done))
                    done += s[1]
                out.append(s)
            yield mk(out)
    # drop runs of calls and probes, then single ones
    idx = [i for i, s in enumerate(steps) if s[0] in ("probe", "snapshot_restore") or
           (s[0] == "call" and s[1] not in TABLE_CALLS)]
    size = len(idx) // 2
    while size >= 1:
        for at in range(0, len(idx), size):
            gone = set(idx[at:at + size])
            yield mk([s for i, s in enumerate(steps) if i not in gone])
        size //= 2
    for i, s in enumerate(steps):
        if s[0] == "call" and s[1] in TABLE_CALLS:
            yield mk(steps[:i] + steps[i + 1:])
    # merge neighbouring steps
    for i in range(len(steps) - 1):
        if steps[i][0] == "step" and steps[i + 1][0] == "step":
            yield mk(steps[:i] + [("step", steps[i][1] + steps[i + 1][1])] + steps[i + 2:])
    # half the overlay, where every id of the schedule still fits
    n = sch.n
    if n >= 16:                     # (four oracle shards, seven engine shards: each needs a node)
        h = (n + 1) // 2
        ok, out = True, []
        for s in steps:
            if s[0] == "call":
                args = s[2]
                if s[1] in ("set_partition",) + TABLE_CALLS:
                    args = [args[0][:h]]
                elif s[1] != "broadcast" and any(x >= h and x != NONE for a in args for x in a):
                    ok = False
                    break
                elif s[1] == "broadcast" and args[0] >= h:
                    ok = False
                    break
                s = ("call", s[1], args)
            elif s[0] == "probe" and s[1] not in ("round", "msg_slots", "histograms"):
                if s[2] >= h:
                    continue
                s = ("probe", s[1], s[2], min(s[3], h - s[2]))
            out.append(s)
        if ok:
            yield mk(out, dict(sch.config, n_nodes=h))


def shrink(schedule, fails, max_steps=400):
    """Greedy reducer: keep a candidate while `fails(candidate)` still answers
    a message.  Bounded by max_steps evaluations.  Returns (schedule, evaluations)."""
    assert fails(schedule), "the schedule does not differ"
    used, progress = 1, True
    while progress and used < max_steps:
        progress = False
        for cand in _candidates(schedule):
            if used >= max_steps:
                break
            used += 1
            if fails(cand):
                schedule, progress = cand, True
                break
    return schedule, used


def main(argv=None):
    ap = argparse.ArgumentParser(description="replay or shrink one random schedule")
    ap.add_argument("--kind", choices=KINDS, default="hv")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--path", default="local", help="the engine path: " + ", ".join(PATHS))
    ap.add_argument("--backends", default=None, help="two paths, comma separated (default: PATH,oracle)")
    ap.add_argument("--dump", help="write the schedule as JSON and stop")
    ap.add_argument("--replay", help="run the schedule of this JSON file")
    ap.add_argument("--shrink", action="store_true")
    ap.add_argument("--out", default="shrunk.json")
    ap.add_argument("--max-steps", type=int, default=400)
    a = ap.parse_args(argv)
    backends = tuple(a.backends.split(",")) if a.backends else (a.path, "oracle")
    assert len(backends) == 2
    hosted = any(b in ("oracle-sharded", "host-exchange") for b in backends)
    if a.replay:
        with open(a.replay) as f:
            sch = Schedule.from_json(f.read())
    else:
        sch = generate(a.kind, a.seed, host=hosted)
    if a.dump:
        with open(a.dump, "w") as f:
            f.write(sch.to_json())
        return 0
    msg = differ(sch, backends)
    print(f"{sch.kind} seed {sch.seed}: n {sch.n}, {sch.rounds()} rounds, {len(sch.calls())} event calls:",
          msg or "identical")
    if msg and a.shrink:
        small, used = shrink(sch, lambda s: differ(s, backends), a.max_steps)
        with open(a.out, "w") as f:
            f.write(small.to_json())
        print(f"shrunk in {used} runs to n {small.n}, {small.rounds()} rounds, {len(small.calls())} event calls: {a.out}")
        print(differ(small, backends))
    return 1 if msg else 0


if __name__ == "__main__":
    sys.exit(main())
