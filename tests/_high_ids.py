"""Scenarios at ids far from 0 (tests/test_high_ids.py, tests/test_gpu_high_ids.py).

Every bit-exact comparison of the engine with the oracle used ids below 2^20;
ids share 32-bit words with other bits in the route keys, the lite kernel's
tags, the connection entries, the Plumtree identities and the records, and a
mask one bit short or a 24-bit multiply only shows above 2^24.  A backend
that allocates rows for an id window only (a host-exchange handle of the
engine, an orc_create_range handle of the oracle) can run a scenario of n
nodes at [base, base + n) of an id space of up to 2^27 - 1 ids.

at_ids(make_range, base, id_space) is a `make` in the idiom of
S.with_buckets: the scenario's cfg, of n nodes, becomes one of id_space ids,
make_range(cfg, base, base + n) creates the backend, and the proxy returned
adds `base` to every id of every call.  What comes back (rows, records) is in
global numbering: nothing is subtracted."""
import numpy as np

import _scenarios as S
from _hybrid import ENGINE, ORACLE, Hybrid
from _oracle import Oracle
from partisan_amd.sim import _Driver

NONE = 0xFFFFFFFF
TOP = (1 << 27) - 1                 # psim_create accepts n_nodes < PSIM_MAP_BIT


def windows(n):
    """name -> (id_space, base) for a scenario of n nodes: the largest ids a
    handle can hold (the last id has bits 0..26 all set), and the two powers
    of two at which narrower arithmetic ends, each in the window's middle"""
    return {"top": (TOP, TOP - n),
            "2^26": ((1 << 26) + 4096, (1 << 26) - n // 2),
            "2^24": ((1 << 24) + 4096, (1 << 24) - n // 2)}


class Shifted:
    def __init__(self, inner, base, n, id_space):
        self.inner, self.base, self.n, self.id_space = inner, base, n, id_space
        self.roots, self.partitions = set(), []        # what the scenario asked for, in its own numbering

    def _ids(self, x):
        return (np.atleast_1d(np.asarray(x)).astype(np.uint64) + self.base).astype(np.uint32)

    def _placed(self, arr, dtype):
        a = np.asarray(arr, dtype)
        assert a.size == self.n
        out = np.zeros(self.id_space, dtype)           # group 0 / bucket 0 outside the window
        out[self.base:self.base + self.n] = a
        return out

    # ---- events
    def join(self, nodes, contacts):
        c = np.asarray(contacts, np.uint32)
        self.inner.join(self._ids(nodes), np.where(c == NONE, c, self._ids(c)).astype(np.uint32))

    def crash(self, nodes): self.inner.crash(self._ids(nodes))
    def revive(self, nodes): self.inner.revive(self._ids(nodes))
    def leave(self, nodes): self.inner.leave(self._ids(nodes))
    def leave_node(self, actors, targets): self.inner.leave_node(self._ids(actors), self._ids(targets))
    def broadcast(self, root, msg_id):
        self.inner.broadcast(int(root) + self.base, msg_id)
        self.roots.add(int(root))

    def begin_omission(self, nodes): self.inner.begin_omission(self._ids(nodes))
    def end_omission(self, nodes): self.inner.end_omission(self._ids(nodes))
    def begin_send_omission(self, s, d): self.inner.begin_send_omission(self._ids(s), self._ids(d))
    def end_send_omission(self, s, d): self.inner.end_send_omission(self._ids(s), self._ids(d))
    def begin_receive_omission(self, s, d): self.inner.begin_receive_omission(self._ids(s), self._ids(d))
    def end_receive_omission(self, s, d): self.inner.end_receive_omission(self._ids(s), self._ids(d))
    def resolve_all_faults(self): self.inner.resolve_all_faults()
    def clear_partition(self): self.inner.clear_partition()

    def set_partition(self, group):
        self.inner.set_partition(self._placed(group, np.uint8))
        self.partitions.append(np.asarray(group, np.uint8).copy())

    def set_bucket_table(self, buckets):
        self.inner.set_bucket_table(None if buckets is None else self._placed(buckets, np.uint8))

    def set_phash_table(self, phash):
        self.inner.set_phash_table(None if phash is None else self._placed(phash, np.uint32))

    # ---- rounds and getters
    def step(self, n_rounds=1): return self.inner.step(n_rounds)
    def msg_slots(self): return self.inner.msg_slots()
    def histograms(self): return self.inner.histograms()
    def close(self): self.inner.close()

    @property
    def round(self):
        return self.inner.round

    run_schedule = _Driver.run_schedule

    def _get(self, name, first, count):
        return getattr(self.inner, name)(first + self.base, self.n - first if count is None else count)

    def nodes(self, first=0, count=None): return self._get("nodes", first, count)
    def strategy_nodes(self, first=0, count=None): return self._get("strategy_nodes", first, count)
    def delivery(self, first=0, count=None): return self._get("delivery", first, count)

    def __getattr__(self, name):             # (a Hybrid's engine, trace, n_out, ...)
        return getattr(self.inner, name)


def at_ids(make_range, base, id_space):
    def make(cfg):
        n = cfg.n_nodes
        assert base + n <= id_space
        c = type(cfg).from_buffer_copy(cfg)
        c.n_nodes = id_space
        return Shifted(make_range(c, base, base + n), base, n, id_space)
    return make


# ---- make_range's
def whole_oracle(cfg, lo, hi):
    """the unchanged unsharded oracle over the whole space (small spaces only)"""
    return Oracle(cfg)


def one_party(kind=ORACLE, **kw):
    """one handle owns the window; every round's outbound list is empty"""
    return lambda cfg, lo, hi: Hybrid(cfg, parties=[(lo, hi, kind)], **kw)


def split(kinds, engine=True, cut=None, **kw):
    """two adjacent parties: [lo, cut) and [cut, hi), cut the middle by default"""
    def make(cfg, lo, hi):
        c = (lo + hi) // 2 if cut is None else lo + cut
        return Hybrid(cfg, parties=[(lo, c, kinds[0]), (c, hi, kinds[1])], engine=engine, **kw)
    return make


# ---- the scenarios the host-exchange handles run (tests/test_gpu_host_exchange.py)
SCENARIOS = {
    "churn_partition": ("churn_partition", dict(n=1024, rounds=110)),
    "xbot_churn": ("xbot_churn", dict(n=1024, rounds=110)),
    "multi_root": ("multi_root", dict(n=1024, rounds=100, churn=True)),
    "scamp_v1": ("pl_doubling", dict(n=512, seed=3, rounds=60, strategy=1, crash_at=30, part_at=45)),
    "scamp_v2": ("pl_doubling", dict(n=512, seed=3, rounds=60, strategy=2, crash_at=30, part_at=45)),
    "event_edges": ("event_edges", dict(n=1021)),
    "config_a": ("config_a", dict()),
}
# The message types each scenario sends whatever the ids (psim_msg_type /
# PSIM_PL_*): HyParView's join, forward join, neighbor, disconnect, neighbor
# request and accept, shuffle and its reply; Plumtree's five once broadcasts
# repeat (config A has one broadcast: the push and its prunes); X-BOT's six;
# SCAMP's hello, state, forward_subscription and ping, v2's keep.
# NEIGHBOR_REJECTED (6) is left out: it needs a request to meet a stale
# disconnect id, a race no schedule here forces (0 to 12 a run).
_HV, _PT, _XB = (0, 1, 2, 3, 4, 5, 7, 8), (9, 10, 11, 12, 13), (16, 17, 18, 19, 20, 21)
SENDS = {
    "churn_partition": _HV + _PT, "xbot_churn": _HV + _PT + _XB, "multi_root": _HV + _PT,
    "event_edges": _HV + _PT, "config_a": _HV + (9, 10), "scamp_v1": (0, 1, 3, 4), "scamp_v2": (0, 1, 3, 4, 5),
}
BOUNDARY = ("churn_partition", "xbot_churn", "multi_root", "scamp_v2")


def size_of(name):
    return SCENARIOS[name][1].get("n", 32)


def pluggable(name):
    return SCENARIOS[name][0] == "pl_doubling"


# A host-exchange handle's round costs the engine time in proportion to the
# id space (about 25 ms a quiet round and 90 ms one with events at 2^27 - 1
# ids, a tenth of that at 2^24), so the GPU file runs fewer rounds at the top
# window, never a smaller id space: through the bootstrap, three broadcasts
# and half the churn (churn_partition, xbot_churn); the churn whole
# (multi_root); the partitions, the crash of all but node 0 and the rejoin
# (event_edges); the joins and the broadcast (config A).  The 2^26 and 2^24
# windows and the CPU file run every scenario whole.
GPU_TOP = {
    "churn_partition": dict(rounds=60), "xbot_churn": dict(rounds=60), "multi_root": dict(rounds=80),
    "event_edges": dict(rounds=70), "config_a": dict(rounds=60, tail=20),
}
RANDOM_TOP_ROUNDS = 45


def gpu_kw(name, window):
    return GPU_TOP.get(name, {}) if window == "top" else {}


def run(name, make, **over):
    """(sim, stats, extra...) of a scenario on make(cfg)"""
    fn, kw = SCENARIOS[name]
    return getattr(S, fn)(make, **dict(kw, **over))


def final(name, sim):
    """the rows a run ends with: node or strategy views, delivery, slots"""
    if pluggable(name):
        return {"strategy_nodes": sim.strategy_nodes()}
    return {"nodes": sim.nodes(), "delivery": sim.delivery(), "msg_slots": sim.msg_slots()}


def compare_final(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], tuple):
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                assert np.array_equal(x, y), f"{k}[{i}] differs at {np.nonzero(x != y)[0][:8].tolist()}"
        else:
            S.compare_nodes(a[k], b[k])


def compare_runs(name, a, b):
    """a and b: what run() returned, on two backends"""
    S.compare_stats(a[1], b[1])
    assert a[2:] == b[2:]
    compare_final(final(name, a[0]), final(name, b[0]))
