"""Host-side driver over the C ABI (include/partisan_gpu_sim.h).

`Simulator` is the product entry point: it loads only the HIP library
(libpartisan_gpu_sim.so) and raises if it is missing.  `_Driver` holds the
backend-independent logic so the tests can drive the CPU oracle through the
same code (tests/_oracle.py).
"""
import ctypes as C

import numpy as np

from . import _abi
from .workloads import NONE


class SimError(RuntimeError):
    """`rc`: the PSIM_* code of the failed call (None: not from the ABI)"""
    rc = None


def default_config(**kw):
    cfg = _abi.PsimConfig()
    cfg.abi_version = _abi.PSIM_ABI_VERSION
    cfg.n_nodes = 32
    cfg.seed = 1
    # partisan_config.erl:102-145 defaults
    cfg.max_active_size, cfg.min_active_size, cfg.max_passive_size = 6, 3, 30
    cfg.arwl, cfg.prwl, cfg.k_active, cfg.k_passive = 5, 30, 3, 4
    cfg.shuffle_period, cfg.promotion_period, cfg.random_promotion = 10, 5, 1
    cfg.persist_epoch, cfg.plumtree, cfg.lazy_tick_period = 0, 1, 1
    cfg.device, cfg.n_shards, cfg.shard_rank, cfg.shard_world = -1, 1, 0, 1
    cfg.comm_id = None
    cfg.max_msgs_per_round = 0
    # pluggable manager (partisan_config.erl:129-130, partisan.hrl:31)
    cfg.manager, cfg.strategy = _abi.MANAGER_HYPARVIEW, _abi.STRATEGY_FULL
    cfg.periodic_interval, cfg.scamp_c, cfg.fanout = 10, 5, 0
    # X-BOT: xbot_interval, 5000 + uniform(60000) ms (partisan_config.erl:100) -> its mean
    cfg.xbot_period = 35
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise KeyError(k)
        setattr(cfg, k, v)
    return cfg


class _Driver:
    """Backend-independent host logic: event batching, stats decoding."""

    def __init__(self, api, cfg, errname=None):
        self._api = api
        self._errname = errname
        self.cfg = cfg
        self.n = cfg.n_nodes
        h = C.c_void_p()
        self._check(api["create"](C.byref(cfg), C.byref(h)), "create")
        self._h = h

    def _check(self, rc, what):
        if rc != 0:
            msg = _abi.ERRORS.get(rc, str(rc))
            if self._errname is not None:
                msg = self._errname(rc).decode()
            err = SimError(f"{what}: {msg}")
            err.rc = rc
            raise err

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._api["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- events (applied at the start of the next round)
    def join(self, nodes, contacts):
        nodes = np.ascontiguousarray(nodes, np.uint32)
        contacts = np.ascontiguousarray(contacts, np.uint32)
        assert nodes.shape == contacts.shape
        self._check(self._api["join"](self._h, _abi.u32p(nodes), _abi.u32p(contacts), nodes.size),
                    "join")

    def crash(self, nodes):
        nodes = np.ascontiguousarray(nodes, np.uint32)
        self._check(self._api["crash"](self._h, _abi.u32p(nodes), nodes.size), "crash")

    def revive(self, nodes):
        """Restart nodes without a join (init/1 state, reached by others)."""
        nodes = np.ascontiguousarray(nodes, np.uint32)
        self._check(self._api["revive"](self._h, _abi.u32p(nodes), nodes.size), "revive")

    def leave(self, nodes):
        """leave/0 at each node (pluggable manager; raises on HyParView, whose
        leave answers `error`): the manager stops before its leave messages
        go out, so the node goes down as in crash()."""
        nodes = np.ascontiguousarray(nodes, np.uint32)
        self._check(self._api["leave"](self._h, _abi.u32p(nodes), nodes.size), "leave")

    def leave_node(self, actors, targets):
        """leave/1: actors[i] removes targets[i] (SCAMP v1 / v2 handles)."""
        a = np.ascontiguousarray(actors, np.uint32)
        t = np.ascontiguousarray(targets, np.uint32)
        if a.size != t.size:
            raise ValueError("actors and targets differ in length")
        self._check(self._api["leave_node"](self._h, _abi.u32p(a), _abi.u32p(t), a.size), "leave_node")

    def set_partition(self, group):
        g = np.ascontiguousarray(group, np.uint8)
        self._check(self._api["set_partition"](
            self._h, g.ctypes.data_as(C.POINTER(C.c_uint8)), g.size), "set_partition")

    def clear_partition(self):
        self._check(self._api["clear_partition"](self._h), "clear_partition")

    def set_bucket_table(self, buckets):
        """The sets v1 bucket (erlang:phash(NodeSpec, 16) - 1, 0..15) of every
        node: the view order of SURVEY App. A Q1.  Before the first round;
        None restores the built-in stand-in."""
        if buckets is None:
            self._check(self._api["set_bucket_table"](self._h, None, 0), "set_bucket_table")
            return
        b = np.ascontiguousarray(buckets, np.uint8)
        self._check(self._api["set_bucket_table"](
            self._h, b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size), "set_bucket_table")

    def set_phash_table(self, phash):
        """erlang:phash(NodeSpec, 2^32) - 1 of every node (uint32): the sets
        v1 slots of every set the handle keeps -- 16 buckets for HyParView
        views, the linear hash's wider tables for SCAMP v1 memberships past
        80 ids.  Before the first round; None restores
        the built-in stand-in."""
        if phash is None:
            self._check(self._api["set_phash_table"](self._h, None, 0), "set_phash_table")
            return
        p = np.ascontiguousarray(phash, np.uint32)
        self._check(self._api["set_phash_table"](self._h, _abi.u32p(p), p.size), "set_phash_table")

    # ---- omission faults of the pluggable manager's interposition layer
    # (add_interposition_fun/2, pluggable:297-326; the crash-fault model's
    # begin/end_send_omission, begin/end_receive_omission, begin/end_omission,
    # resolve_all_faults_with_heal: prop_partisan_crash_fault_model:93-229)
    def _omission(self, kind, src, dst, on):
        s = np.ascontiguousarray(np.atleast_1d(src), np.uint32)
        d = np.ascontiguousarray(np.atleast_1d(dst), np.uint32)
        if s.size != d.size:
            raise ValueError("src and dst differ in length")
        self._check(self._api["set_omission"](self._h, kind, _abi.u32p(s), _abi.u32p(d), s.size, int(on)),
                    "set_omission")

    def begin_send_omission(self, src, dst):
        """Messages src forwards to dst are dropped at src (never sent)."""
        self._omission(_abi.OMIT_SEND, src, dst, True)

    def end_send_omission(self, src, dst):
        self._omission(_abi.OMIT_SEND, src, dst, False)

    def begin_receive_omission(self, src, dst):
        """Messages dst receives from src are dropped at dst (never handled)."""
        self._omission(_abi.OMIT_RECEIVE, src, dst, True)

    def end_receive_omission(self, src, dst):
        self._omission(_abi.OMIT_RECEIVE, src, dst, False)

    def begin_omission(self, nodes):
        """General omission: every strategy message the nodes send or receive."""
        n = np.ascontiguousarray(np.atleast_1d(nodes), np.uint32)
        self._check(self._api["set_faulted"](self._h, _abi.u32p(n), n.size, 1), "set_faulted")

    def end_omission(self, nodes):
        n = np.ascontiguousarray(np.atleast_1d(nodes), np.uint32)
        self._check(self._api["set_faulted"](self._h, _abi.u32p(n), n.size, 0), "set_faulted")

    def resolve_all_faults(self):
        self._check(self._api["clear_faults"](self._h), "clear_faults")

    def broadcast(self, root, msg_id):
        self._check(self._api["broadcast"](self._h, root, msg_id), "broadcast")

    # ---- execution
    def step(self, n_rounds=1):
        st = np.zeros(n_rounds, _abi.STATS_DTYPE)
        self._check(self._api["step"](self._h, n_rounds,
                                      st.ctypes.data_as(C.POINTER(_abi.PsimRoundStats))), "step")
        return st

    @property
    def round(self):
        r = C.c_uint64()
        self._check(self._api["get_round"](self._h, C.byref(r)), "get_round")
        return r.value

    def nodes(self, first=0, count=None):
        if count is None:
            count = self.n - first
        out = np.zeros(count, _abi.NODE_VIEW_DTYPE)
        self._check(self._api["get_nodes"](self._h, first, count,
                                           out.ctypes.data_as(C.POINTER(_abi.PsimNodeView))),
                    "get_nodes")
        return out

    def delivery(self, first=0, count=None):
        """Tracked broadcast per node: (have, first-delivery round, hop)."""
        if count is None:
            count = self.n - first
        have = np.zeros(count, np.uint8)
        rnd = np.zeros(count, np.uint32)
        hop = np.zeros(count, np.uint32)
        self._check(self._api["get_delivery"](self._h, first, count,
                                              have.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              _abi.u32p(rnd), _abi.u32p(hop)), "get_delivery")
        return have, rnd, hop

    def msg_slots(self):
        """The live Plumtree message slots (psim_get_msg_slots): per slot k the
        message id owning it (NONE = free) and its root identity."""
        ids = np.zeros(_abi.MSG_SLOTS, np.uint32)
        roots = np.zeros(_abi.MSG_SLOTS, np.uint32)
        self._check(self._api["get_msg_slots"](self._h, _abi.u32p(ids), _abi.u32p(roots), ids.size),
                    "get_msg_slots")
        return ids, roots

    def histograms(self):
        """Overlay statistics (psim_histograms) as a dict of ints / arrays."""
        h = _abi.PsimHistograms()
        self._check(self._api["get_histograms"](self._h, C.byref(h)), "get_histograms")
        out = {}
        for name, _ in _abi.PsimHistograms._fields_:
            if name == "reserved":
                continue
            v = getattr(h, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    def run_schedule(self, schedule, until_round, extra=None):
        """Apply [(round, ids, contacts)] join events and step until `until_round`.
        `extra(round)` may inject further events before each round."""
        ev = {}
        for r, ids, contacts in schedule:
            ev.setdefault(r, []).append((ids, contacts))
        stats = []
        while self.round < until_round:
            r = self.round
            for ids, contacts in ev.get(r, []):
                self.join(ids, contacts)
            if extra is not None:
                extra(r)
            stats.append(self.step(1))
        return np.concatenate(stats) if stats else np.zeros(0, _abi.STATS_DTYPE)

    # ---- pluggable manager state (get_local_state/0, members/0)
    def strategy_nodes(self, first=0, count=None):
        if count is None:
            count = self.n - first
        out = np.zeros(count, _abi.STRATEGY_VIEW_DTYPE)
        self._check(self._api["get_strategy_nodes"](
            self._h, first, count, out.ctypes.data_as(C.POINTER(_abi.PsimStrategyView))),
            "get_strategy_nodes")
        return out

    def member_bits(self, node):
        w = np.zeros((self.n + 31) // 32, np.uint32)
        self._check(self._api["get_member_bits"](self._h, node, _abi.u32p(w), w.size),
                    "get_member_bits")
        return w

    def members(self, node):
        """membership_list/1 of a node: full -> ids of query(ORSet) in id order;
        scamp -> the view in its list order"""
        if self.cfg.strategy == _abi.STRATEGY_FULL:
            w = self.member_bits(node)
            return [int(i) for i in np.nonzero(np.unpackbits(w.view(np.uint8), bitorder="little"))[0]]
        v = self.strategy_nodes(node, 1)[0]
        return [int(x) for x in v["view"][: v["view_n"]]]

    # ---- reference-style debug getters (hyparview:261-281)
    def active(self, node):
        v = self.nodes(node, 1)[0]
        return [int(x) for x in v["act"][: v["act_n"]]]

    def passive(self, node):
        v = self.nodes(node, 1)[0]
        return [int(x) for x in v["pas"][: v["pas_n"]]]


def comm_id():
    """A fresh RCCL unique id (rank 0 creates it and shares the bytes)."""
    from . import _lib

    lib = _lib.load()
    extra = _abi.bind(lib, "psim_", _abi.GPU_ONLY)
    n = extra["comm_id_size"]()
    buf = C.create_string_buffer(n)
    rc = extra["get_comm_id"](buf, n)
    if rc != 0:
        raise SimError(f"get_comm_id: {extra['strerror'](rc).decode()}")
    return buf.raw


def loopback_comm_id():
    """TEST VEHICLE: the id of a new loopback world (psim_loopback_comm_id):
    ranks as threads of this process on one device, in place of RCCL."""
    from . import _lib

    lib = _lib.load()
    extra = _abi.bind(lib, "psim_", _abi.GPU_ONLY)
    n = extra["comm_id_size"]()
    buf = C.create_string_buffer(n)
    rc = extra["loopback_comm_id"](buf, n)
    if rc != 0:
        raise SimError(f"loopback_comm_id: {extra['strerror'](rc).decode()}")
    return buf.raw


def host_comm_id(lo, hi):
    """The id of a host-exchange handle that owns the ids [lo, hi)
    (psim_host_comm_id); HostSim passes it as cfg.comm_id."""
    from . import _lib

    lib = _lib.load()
    extra = _abi.bind(lib, "psim_", _abi.GPU_ONLY)
    n = extra["comm_id_size"]()
    buf = C.create_string_buffer(n)
    rc = _abi.bind(lib, "psim_", _abi.HOST_BOUNDARY)["host_comm_id"](buf, n, lo, hi)
    if rc != 0:
        raise SimError(f"host_comm_id: {extra['strerror'](rc).decode()}")
    return buf.raw


class Simulator(_Driver):
    """MI355X simulator handle (HIP library; fails loudly without it).

    Multi-GPU: one process per GPU, all with the same global n_nodes and
    `shard_world`, each with its `shard_rank` and the same `comm` bytes from
    comm_id() on rank 0; every rank then issues the same event calls."""

    def __init__(self, cfg=None, comm=None, **kw):
        from . import _lib

        lib = _lib.load()
        api = _abi.bind(lib, "psim_", _abi.SIGNATURES)
        extra = _abi.bind(lib, "psim_", _abi.GPU_ONLY)
        self._extra = extra
        if cfg is None:
            cfg = default_config(**kw)
        if comm is not None:
            self._comm_buf = C.create_string_buffer(bytes(comm), len(comm))
            cfg.comm_id = C.cast(self._comm_buf, C.c_void_p)
        super().__init__(api, cfg, errname=extra["strerror"])

    def snapshot(self):
        """The whole simulation state as bytes (psim_snapshot)."""
        need = C.c_size_t()
        self._check(self._extra["snapshot"](self._h, None, 0, C.byref(need)), "snapshot")
        buf = C.create_string_buffer(need.value)
        self._check(self._extra["snapshot"](self._h, buf, need.value, C.byref(need)), "snapshot")
        return buf.raw[:need.value]

    def restore(self, data):
        """Load a snapshot into this handle (same config)."""
        buf = C.create_string_buffer(bytes(data), len(data))
        self._check(self._extra["restore"](self._h, buf, len(data)), "restore")

    def exchange_stats(self):
        """(records, wire bytes) this process's shards sent to other shards
        since creation (psim_get_exchange_stats)."""
        r, b = C.c_uint64(), C.c_uint64()
        self._check(self._extra["get_exchange_stats"](self._h, C.byref(r), C.byref(b)), "get_exchange_stats")
        return r.value, b.value

    def strategy_histograms(self):
        """Overlay statistics of a pluggable handle (psim_strategy_histograms)
        as a dict of ints / arrays; a collective on rank handles."""
        h = _abi.PsimStrategyHistograms()
        self._check(self._extra["get_strategy_histograms"](self._h, C.byref(h)), "get_strategy_histograms")
        out = {}
        for name, _ in _abi.PsimStrategyHistograms._fields_:
            if name == "reserved":
                continue
            v = getattr(h, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    def graph_metrics(self, sources=None, k=64, seed=0, max_levels=0):
        """Path lengths from up to 64 sources and the clustering of the whole
        overlay (psim_graph_metrics) as a dict of ints / arrays; a collective
        on rank handles.  sources=None draws k distinct ids from
        np.random.Generator(PCG64([seed, 0x6d])); an empty list fills the
        clustering half only."""
        if sources is None:
            rng = np.random.Generator(np.random.PCG64([seed, 0x6d]))
            sources = rng.choice(self.n, size=min(k, self.n), replace=False)
        src = np.ascontiguousarray(sources, np.uint32).reshape(-1)
        m = _abi.PsimGraphMetrics()
        self._check(self._extra["get_graph_metrics"](self._h, _abi.u32p(src) if src.size else None, src.size,
                                                     max_levels, C.byref(m)), "get_graph_metrics")
        out = {}
        for name, _ in _abi.PsimGraphMetrics._fields_:
            if name == "reserved":
                continue
            v = getattr(m, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    # the fields of graph_metrics() that add up over disjoint source batches
    _PATH_SUMS = ("sources_live", "dist", "dist_sum", "pairs_reached", "pairs_unreached")

    def graph_metrics_all(self, max_levels=0):
        """graph_metrics() over every id as a source, in batches of 64: exact
        all-pairs path numbers of a small overlay.  The path sums add up over
        the batches; ecc_max, levels and truncated are the largest; `reach`
        and `ecc` come back per node (n entries, zero for a dead node)."""
        out = None
        reach, ecc = np.zeros(self.n, np.uint64), np.zeros(self.n, np.uint64)
        for lo in range(0, self.n, _abi.GRAPH_SOURCES):
            ids = np.arange(lo, min(self.n, lo + _abi.GRAPH_SOURCES), dtype=np.uint32)
            m = self.graph_metrics(ids, max_levels=max_levels)
            reach[ids], ecc[ids] = m["reach"][: ids.size], m["ecc"][: ids.size]
            if out is None:
                out = m
                continue
            for f in self._PATH_SUMS:
                out[f] = out[f] + m[f]
            for f in ("ecc_max", "levels", "truncated"):
                out[f] = max(out[f], m[f])
        if out is None:
            out = self.graph_metrics([])
        out["reach"], out["ecc"] = reach, ecc
        return out

    def tree_metrics(self, root, max_levels=0):
        """The broadcast tree of Plumtree root `root` (psim_tree_metrics) as a
        dict of ints / arrays; a collective on rank handles."""
        m = _abi.PsimTreeMetrics()
        self._check(self._extra["get_tree_metrics"](self._h, int(root), max_levels, C.byref(m)), "get_tree_metrics")
        out = {}
        for name, _ in _abi.PsimTreeMetrics._fields_:
            if name == "reserved":
                continue
            v = getattr(m, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    def latency_metrics(self, sources=None, k=64, seed=0, tree_root=None, max_sweeps=0):
        """Link costs and the cheapest paths by latency from up to 64 sources
        (psim_latency_metrics) as a dict of ints / arrays; a collective on
        rank handles.  The sources are picked as graph_metrics() picks them
        (the same k and seed give the same ids); an empty list with no
        tree_root fills the link census only.  tree_root adds the tree half of
        that Plumtree root."""
        if sources is None:
            rng = np.random.Generator(np.random.PCG64([seed, 0x6d]))
            sources = rng.choice(self.n, size=min(k, self.n), replace=False)
        src = np.ascontiguousarray(sources, np.uint32).reshape(-1)
        root = NONE if tree_root is None else int(tree_root)
        m = _abi.PsimLatencyMetrics()
        self._check(self._extra["get_latency_metrics"](self._h, _abi.u32p(src) if src.size else None, src.size,
                                                       root, max_sweeps, C.byref(m)), "get_latency_metrics")
        out = {}
        for name, _ in _abi.PsimLatencyMetrics._fields_:
            if name == "reserved":
                continue
            v = getattr(m, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    def resilience(self, sources, thresholds, salts=None, fail_seed=0, max_levels=0):
        """Reach of a flood under up to 64 failure cases (psim_resilience) as
        a dict of ints / arrays; a collective on rank handles.  Case j floods
        from sources[j] after every other node v with u(v, salts[j]) <
        thresholds[j] has failed: the failed share is thresholds[j] / 2^32.
        salts=None means all 0 (nested failure sets)."""
        src = np.ascontiguousarray(sources, np.uint32).reshape(-1)
        thr = np.ascontiguousarray(thresholds, np.uint32).reshape(-1)
        slt = np.zeros(src.size, np.uint32) if salts is None else np.ascontiguousarray(salts, np.uint32).reshape(-1)
        if not src.size == thr.size == slt.size:
            raise ValueError("sources, thresholds and salts differ in length")
        cases = (_abi.PsimFailureCase * max(src.size, 1))()
        for j in range(src.size):
            cases[j].source, cases[j].threshold, cases[j].salt = int(src[j]), int(thr[j]), int(slt[j])
        m = _abi.PsimResilience()
        self._check(self._extra["get_resilience"](self._h, cases if src.size else None, src.size, int(fail_seed),
                                                  max_levels, C.byref(m)), "get_resilience")
        out = {}
        for name, _ in _abi.PsimResilience._fields_:
            if name == "reserved":
                continue
            v = getattr(m, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    def gossip_reach(self, sources, fanouts, thresholds=None, salts=None, fail_seed=0, max_levels=0):
        """Reach and cost of a gossip with a fanout under up to 64 cases
        (psim_gossip_reach) as a dict of ints / arrays; a collective on rank
        handles.  Case j starts at sources[j] after the failures of
        resilience()'s case (sources[j], thresholds[j], salts[j]); every node
        reached pushes once, to at most fanouts[j] of its links (0: to all of
        them).  thresholds=None and salts=None mean all 0."""
        src = np.ascontiguousarray(sources, np.uint32).reshape(-1)
        cols = [src, np.ascontiguousarray(fanouts, np.uint32).reshape(-1)]
        for v in (thresholds, salts):
            cols.append(np.zeros(src.size, np.uint32) if v is None else np.ascontiguousarray(v, np.uint32).reshape(-1))
        if any(c.size != src.size for c in cols):
            raise ValueError("sources, fanouts, thresholds and salts differ in length")
        cases = (_abi.PsimGossipCase * max(src.size, 1))()
        for j in range(src.size):
            cases[j].source, cases[j].fanout, cases[j].threshold, cases[j].salt = (int(c[j]) for c in cols)
        m = _abi.PsimGossipReach()
        self._check(self._extra["get_gossip_reach"](self._h, cases if src.size else None, src.size, int(fail_seed),
                                                    max_levels, C.byref(m)), "get_gossip_reach")
        out = {}
        for name, _ in _abi.PsimGossipReach._fields_:
            if name == "reserved":
                continue
            v = getattr(m, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    def relay_reach(self, sources, targets, ttls, max_levels=0):
        """Up to 64 transitive unicasts over the frozen overlay
        (psim_relay_reach) as a dict of ints / arrays; a collective on rank
        handles.  Case j sends from sources[j] to targets[j] with
        {broadcast, true} and {transitive, true}: directly where the source
        holds a connection, else as the relay_message flood with ttl ttls[j]
        (a scalar: the same for every case).  max_levels caps the levels run
        (0: 16)."""
        src = np.ascontiguousarray(sources, np.uint32).reshape(-1)
        dst = np.ascontiguousarray(targets, np.uint32).reshape(-1)
        ttl = np.full(src.size, ttls, np.uint32) if np.ndim(ttls) == 0 else np.ascontiguousarray(ttls, np.uint32).reshape(-1)
        if not src.size == dst.size == ttl.size:
            raise ValueError("sources, targets and ttls differ in length")
        cases = (_abi.PsimRelayCase * max(src.size, 1))()
        for j in range(src.size):
            cases[j].source, cases[j].target, cases[j].ttl = int(src[j]), int(dst[j]), int(ttl[j])
        m = _abi.PsimRelayReach()
        self._check(self._extra["get_relay_reach"](self._h, cases if src.size else None, src.size, max_levels,
                                                   C.byref(m)), "get_relay_reach")
        out = {}
        for name, _ in _abi.PsimRelayReach._fields_:
            if name == "reserved":
                continue
            v = getattr(m, name)
            out[name] = np.array(v[:], np.uint64) if hasattr(v, "__len__") else int(v)
        return out

    # ---- the message trace (psim_trace_watch / psim_trace_read / psim_trace_clear)
    def trace_watch(self, nodes=None, to=True, frm=True, types=None, capacity=1 << 20):
        """Arm a watch: from the next round on, the records sent to (`to`) or
        by (`frm`) the ids in `nodes` (None: every node) are kept, up to
        `capacity` between two reads.  `types`: an iterable of message type
        numbers (None: all).  Replaces an earlier watch and drops its records."""
        mask = (1 << _abi.NTYPES) - 1
        if types is not None:
            mask = 0
            for t in types:
                mask |= 1 << int(t)
        d = (_abi.PSIM_TRACE_TO if to else 0) | (_abi.PSIM_TRACE_FROM if frm else 0)
        if nodes is None:
            ptr, n = None, 0
        else:
            ids = np.ascontiguousarray(nodes, np.uint32).reshape(-1)
            ptr, n = _abi.u32p(ids), ids.size
        self._check(self._extra["trace_watch"](self._h, ptr, n, d, mask & 0xFFFFFFFF, capacity), "trace_watch")

    def trace_read(self):
        """(recs[n, 16] uint32, rounds[n] uint32, lost): the records kept since
        the last read, in (round, dst, src, seq) order, each in the wire
        codec's layout, and the number of matches past the capacity.  Empties
        the buffer."""
        n, lost = C.c_size_t(), C.c_uint64()
        self._check(self._extra["trace_read"](self._h, None, None, 0, C.byref(n), C.byref(lost)), "trace_read")
        recs = np.zeros((n.value, 16), np.uint32)
        rounds = np.zeros(n.value, np.uint32)
        self._check(self._extra["trace_read"](self._h, _abi.u32p(recs), _abi.u32p(rounds), n.value, C.byref(n),
                                              C.byref(lost)), "trace_read")
        return recs, rounds, lost.value

    def trace_clear(self):
        """Disarm the watch and free its buffers (a no-op without one)."""
        self._check(self._extra["trace_clear"](self._h), "trace_clear")

    # (k_node_prep: the quiet lazy ticks it counts without running the node)
    KERNELS = ("k_relay", "k_shuf", "k_lite_half", "k_consume", "k_ptl", "k_pt", "k_node_prep")

    def kernel_counts(self):
        """{kernel: (nodes processed, delivered, emitted)} of the last round,
        per node-round kernel (psim_debug_kernel_counts); {} under the
        pluggable manager."""
        out = (C.c_uint64 * 28)()
        k = self._extra["debug_kernel_counts"](self._h, out, 28)
        self._check(min(k, 0), "debug_kernel_counts")
        return {self.KERNELS[i]: (out[4 * i], out[4 * i + 1], out[4 * i + 2]) for i in range(k)}

    def kernel_times(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        launches = (C.c_uint64 * cap)()
        k = self._extra["kernel_times"](self._h, names, ms, launches, cap)
        return {names[i].decode(): (ms[i], launches[i]) for i in range(k)}


class HostSim(Simulator):
    """A host-exchange handle: the engine simulates the ids [lo, hi) of
    cfg.n_nodes and the host speaks for every other id (real partisan nodes,
    or another simulator).  Every event call is made here too, for outside
    nodes as well.  A round is emit() -> outbound() -> absorb(records);
    step() raises SimError."""

    def __init__(self, cfg, lo, hi):
        from . import _lib

        self.lo, self.hi = lo, hi
        self._host = _abi.bind(_lib.load(), "psim_", _abi.HOST_BOUNDARY)
        super().__init__(cfg, comm=host_comm_id(lo, hi))

    def emit(self):
        """Apply the pending events and run the owned nodes' round."""
        self._check(self._host["round_emit"](self._h), "round_emit")

    def outbound(self):
        """The open round's records for outside nodes, an (n, 16) uint32
        array in the wire codec's layout: ids below lo first, then ids at or
        above hi, each side in (src, seq) order."""
        n = C.c_size_t()
        self._check(self._host["get_outbound"](self._h, None, 0, C.byref(n)), "get_outbound")
        out = np.zeros((n.value, 16), np.uint32)
        self._check(self._host["get_outbound"](self._h, _abi.u32p(out), n.value, C.byref(n)), "get_outbound")
        return out

    def absorb(self, recs):
        """Close the round with the records outside nodes sent to owned
        nodes, in any order; returns this handle's stats row of the round."""
        r = np.ascontiguousarray(recs, np.uint32).reshape(-1, 16)
        st = np.zeros(1, _abi.STATS_DTYPE)
        self._check(self._host["round_absorb"](self._h, _abi.u32p(r), r.shape[0],
                                                st.ctypes.data_as(C.POINTER(_abi.PsimRoundStats))), "round_absorb")
        return st

    def nodes(self, first=None, count=None):
        """Views of owned nodes (default: the whole owned range)."""
        first = self.lo if first is None else first
        return super().nodes(first, self.hi - first if count is None else count)

    def strategy_nodes(self, first=None, count=None):
        first = self.lo if first is None else first
        return super().strategy_nodes(first, self.hi - first if count is None else count)


__all__ = ["Simulator", "HostSim", "SimError", "default_config", "comm_id", "host_comm_id", "NONE"]
