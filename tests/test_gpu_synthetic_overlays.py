"""The overlay getters on hand-built graphs, put into a handle through a
restored snapshot (tests/_overlay_inject.py): every field of every struct
exact against its plain reference applied to the *requested* rows.  Overlays
a protocol run never makes: distance 63 and more, the level and sweep caps at
their natural 4096, in-degree n - 1 on one word, HyParView rows of 8 links,
thousands of components, a label that has to cross 12 500 hops, 8^16 relay
copies -- on one shard, 3 virtual shards and 2 loopback ranks.

Which rows are dirty.  Repeated ids, a node's own id and dead targets reach
only the getters whose header text defines them: the link set L of
psim_graph_metrics (shared by resilience, gossip and latency) and
psim_strategy_histograms' self_entries / duplicate_entries / dangling_links.
psim_histograms gets dead targets only ("links count live -> live only"; it
says nothing of a repeated id).  The tree and the relay getter get clean rows:
their headers define dead and self entries too, but the scenario tests of
those getters already reach them; here they see the shapes, not the dirt.

No test passes a row outside the engine's own domain: inject() refuses those
on the host (tests/test_graph_families.py covers the refusals)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _gossip as P
import _graph_families as F
import _graph_metrics as G
import _latency as Q
import _overlay_inject as I
import _relay as Y
import _resilience as R
import _scenarios as S
import _strategy_stats as SS
import _tree_metrics as T
from partisan_amd import _abi
from partisan_amd.sim import default_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAP = G.MAX_LEVELS
NONE = 0xFFFFFFFF


# ---- handles
def _gpu(cfg):
    from partisan_amd import Simulator
    return Simulator(cfg)


def _vshards(k):
    def mk(cfg):
        from partisan_amd import Simulator
        c = type(cfg).from_buffer_copy(cfg)
        c.n_shards = k
        return Simulator(c)
    return mk


def _loop(world):
    def mk(cfg):
        from _loopback import LoopbackRanks
        return LoopbackRanks(cfg, world)
    return mk


MAKES = [_gpu, _vshards(3), _loop(2)]
MAKE_IDS = ["gpu", "3-shards", "loopback-2"]


def _boot(make, n, kind="hv", seed=1):
    """a handle of the wanted manager whose every id has joined (id i at
    i - 1: one JOIN a node) and that has stepped a round: flags, started and
    every table are the engine's own"""
    kw = dict(manager=_abi.MANAGER_PLUGGABLE, strategy=_abi.STRATEGY_SCAMP_V2) if kind == "scamp" else {}
    sim = make(default_config(n_nodes=n, seed=seed, **kw))
    ids = np.arange(n, dtype=np.uint32)
    contacts = np.concatenate([np.array([NONE], np.uint32), ids[:-1]])
    sim.join(ids, contacts)
    sim.step(1)
    return sim


def _call(sim, name, *a):
    """a getter of a handle; of loopback ranks: one thread per rank (a
    collective), every rank the same answer"""
    if hasattr(sim, "ranks"):
        ms = sim._threads(name, *a)
        for m in ms[1:]:
            assert all(np.array_equal(m[k], ms[0][k]) for k in m), f"ranks disagree on {name}"
        return ms[0]
    return getattr(sim, name)(*a)


def _uniq(ids):
    return list(dict.fromkeys(int(x) for x in ids))


def _seed_of(sim):
    return int(sim.cfg.seed)


# ---- the link getters on one injected graph
def _fails(srcs):
    """64 failure cases: the report's grid over up to 8 sources (share q / 10
    failed, salt k); q = 0 rows flood the whole graph"""
    return R.grid(list(srcs)[:8])


def _gossips(srcs):
    s = list(srcs)[:8]
    return [(int(x), (q << 32) // 10, k, f) for q, f in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 3), (3, 2), (0, 8), (5, 0))
            for k, x in enumerate(s)]


_REF = {}


def _ref(key, name, fn):
    """a reference computed once per (graph key, getter), shared by the handle kinds, left unchanged"""
    if key is None:
        return fn()
    if (key, name) not in _REF:
        _REF[key, name] = fn()
    return _REF[key, name]


def _links(sim, g, sources, max_levels=0, max_sweeps=None, lat_sources=None, key=None):
    """graph metrics, resilience, gossip and latency of `g`, already injected"""
    rows = g.rows()
    G.compare(_call(sim, "graph_metrics", list(sources), 64, 0, max_levels),
              _ref(key, "graph", lambda: G.reference_rows(rows, sources, max_levels)))
    fc = _fails(sources)
    src, thr, salt = ([c[k] for c in fc] for k in range(3))
    R.compare(_call(sim, "resilience", src, thr, salt, 7, max_levels),
              _ref(key, "resilience", lambda: R.reference_rows(rows, fc, 7, max_levels)))
    gc = _gossips(sources)
    src, thr, salt, fan = ([c[k] for c in gc] for k in range(4))
    P.compare(_call(sim, "gossip_reach", src, fan, thr, salt, 7, max_levels),
              _ref(key, "gossip", lambda: P.reference_rows(rows, gc, 7, max_levels)))
    ls = list(sources if lat_sources is None else lat_sources)
    sweeps = max_levels if max_sweeps is None else max_sweeps
    Q.compare(_call(sim, "latency_metrics", ls, 64, 0, None, sweeps),
              _ref(key, "latency", lambda: Q.reference_links(Q.links_rows(rows), _seed_of(sim), ls, sweeps)))


def _hist(sim, g):
    """psim_histograms' link fields; the rest is what the injection leaves: an
    empty passive view, no tracked broadcast"""
    want = F.histograms_reference(g.rows())
    h = _call(sim, "histograms")
    bad = [k for k in want if not np.array_equal(np.asarray(h[k], np.uint64), np.asarray(want[k], np.uint64))]
    assert not bad, {k: (h[k], want[k]) for k in bad}
    assert int(h["passive_fill"][0]) == want["n_up"] and int(h["passive_in"][0]) == want["n_up"]
    return h


def _views(rows):
    """strategy_nodes() as the strategy reference reads it, from injected rows"""
    v = np.zeros(len(rows), _abi.STRATEGY_VIEW_DTYPE)
    for i, r in enumerate(rows):
        v["up"][i] = 1 if r.get("up", True) else 0
        for col, cnt, key in (("view", "view_n", "view"), ("in_view", "in_n", "in_view")):
            ids = r.get(key, [])
            v[cnt][i] = len(ids)
            v[col][i][: len(ids)] = ids
    return v


def _shist(sim, rows):
    SS.compare(_call(sim, "strategy_histograms"), SS.reference(_views(rows), _abi.STRATEGY_SCAMP_V2))


# ---- the layout mirror against real scenarios
def _sum_check(sim, snap, cfg):
    lay = I.layout(cfg, snap)                   # (raises unless the sizes add up to exactly len(snap))
    assert lay.tobytes() == snap
    return lay


def test_layout_mirror_config_a():
    """config A after 40 rounds of its tail: hdr, act, pt_*, conn as nodes() reports them"""
    sim = S.config_a(_gpu)[0]
    try:
        snap = sim.snapshot()
        lay = _sum_check(sim, snap, sim.cfg)
        s = lay.shards[0]
        v = sim.nodes()
        assert np.array_equal(s.flags & 1, v["up"])
        for a, b in (("act_n", "act_n"), ("pas_n", "pas_n"), ("all_n", "pt_all_n"), ("com_n", "pt_common_n"),
                     ("conn_n", "conn_n"), ("out_n", "pt_out_n"), ("epoch", "epoch"), ("start_round", "start_round"),
                     ("rng", "rng_ctr"), ("trk_round", "trk_round"), ("trk_hop", "trk_hop"), ("sent_n", "sent_n"),
                     ("recv_head", "recv_head")):
            assert np.array_equal(s.hdr[a], v[b]), a
        assert np.array_equal(s.hdr["have"].astype(np.uint64) | (s.hdr["aux"].astype(np.uint64) << 32), v["have"])
        for a, b in (("act", "act"), ("pas", "pas"), ("pt_all", "pt_all"), ("pt_com", "pt_common"),
                     ("pt_eag", "pt_eager"), ("pt_laz", "pt_lazy")):
            assert np.array_equal(s[a], v[b]), a
        assert np.array_equal(s.pt_rt[:, :4], v["pt_root"])
        for q in range(4):
            assert np.array_equal((s.pt_rt[:, 4] >> (8 * q)) & 0xFF, v["pt_eager_n"][:, q])
            assert np.array_equal((s.pt_rt[:, 5] >> (8 * q)) & 0xFF, v["pt_lazy_n"][:, q])
        for i in range(sim.n):
            assert np.array_equal(s.conn[i, : v["conn_n"][i]], v["conn"][i, : v["conn_n"][i]])
        assert v["act_n"].max() >= 3 and v["pt_eager_n"].any() and int(lay.head["round"]) == sim.round
        # parse, serialise, restore: nodes() and the next 10 rounds unchanged
        other = S.config_a(_gpu, rounds=200, tail=40)[0]
        want = other.step(10)
        sim.restore(lay.tobytes())
        assert sim.nodes().tobytes() == v.tobytes()
        S.compare_stats(sim.step(10), want)
        S.compare_nodes(sim.nodes(), other.nodes())
        other.close()
    finally:
        sim.close()


@pytest.mark.parametrize("make,shards", list(zip(MAKES, [1, 3, 1])), ids=MAKE_IDS)
def test_layout_mirror_scamp_v2(make, shards):
    """a SCAMP v2 run, three rounds after a tenth of the nodes crashed: sview /
    sinv, one ShardHead a virtual shard, one snapshot a rank"""
    run = lambda mk: S.pl_doubling(mk, 1024, 11, 43, strategy=2, crash_at=40)[0]
    sim, other = run(make), run(make)
    try:
        ranked = hasattr(sim, "ranks")
        snaps = sim.snapshot() if ranked else [sim.snapshot()]
        cfgs = [r.cfg for r in sim.ranks] if ranked else [sim.cfg]
        lays = [_sum_check(sim, b, c) for b, c in zip(snaps, cfgs)]
        v = sim.strategy_nodes()
        seen = 0
        for lay in lays:
            assert len(lay.shards) == shards
            for s in lay.shards:
                lo, n = int(s.head["lo"]), int(s.head["n"])
                seen += n
                assert np.array_equal(s.flags & 1, v["up"])                  # (replicated: all N in every shard)
                assert np.array_equal(s.hdr["act_n"], v["view_n"][lo: lo + n])
                assert np.array_equal(s.hdr["pas_n"], v["in_n"][lo: lo + n])
                assert np.array_equal(s.sview, v["view"][lo: lo + n]) and np.array_equal(s.sinv, v["in_view"][lo: lo + n])
                assert np.array_equal(s.hdr["rng"], v["rng_ctr"][lo: lo + n])
        assert seen == 1024 and v["view_n"].max() > 8 and not v["up"].all()
        want = other.step(10)
        data = [lay.tobytes() for lay in lays]
        sim.restore(data if ranked else data[0])
        assert sim.strategy_nodes().tobytes() == v.tobytes()
        S.compare_stats(sim.step(10), want)
        S.compare_strategy(sim, other)
    finally:
        sim.close()
        other.close()


# ---- graph metrics; resilience, gossip and latency share the runs
@pytest.mark.parametrize("make", MAKES, ids=MAKE_IDS)
def test_path_4200_hits_every_cap(make):
    """a source at an end, max_levels = 0: level 4096 still finds a node
    (truncated = 1, 103 pairs unreached), dist[63] holds 4034 pairs; the
    latency sweeps end at their cap with D_R about 2 * 10^6"""
    g = F.path(4200, "random", seed=3)
    end = g.closed["end"]
    sim = _boot(make, g.n)
    try:
        I.inject(sim, g.hv())
        m = _call(sim, "graph_metrics", [end], 64, 0, 0)
        assert (m["levels"], m["truncated"], int(m["dist"][63]), m["pairs_unreached"]) == (CAP, 1, CAP - 62, 4199 - CAP)
        _links(sim, g, [end, g.perm[2100], g.perm[4199]], 0, max_sweeps=CAP, lat_sources=[end, g.perm[2100]], key="path4200")
        lat = _call(sim, "latency_metrics", [end], 64, 0, None, CAP)
        assert lat["truncated_mask"] == 1 and int(lat["last_sweep"][0]) == CAP and int(lat["lat"][63]) > 3000
        assert 1_000_000 < lat["lat_max"] < 4_300_000
        _hist(sim, g)
    finally:
        sim.close()


@pytest.mark.parametrize("n,trunc", [(CAP + 1, 1), (CAP + 2, 1), (CAP, 0)])
def test_path_at_the_two_sides_of_the_cap(n, trunc):
    g = F.path(n, "zigzag")
    sim = _boot(_gpu, n)
    try:
        I.inject(sim, g.hv())
        m = _call(sim, "graph_metrics", [g.closed["end"]], 64, 0, 0)
        assert (m["levels"], m["truncated"], m["pairs_reached"]) == (CAP, trunc, min(n - 1, CAP))
        _links(sim, g, [g.closed["end"]], 0, max_sweeps=CAP)
    finally:
        sim.close()


def test_path_200_all_pairs():
    g = F.path(200, "random", seed=8)
    sim = _boot(_gpu, 200)
    try:
        I.inject(sim, g.hv())
        m = sim.graph_metrics_all()
        G.compare(m, G.reference_all(_hv_views(g), "hv"))
        assert m["dist_sum"] == 200 * 199 * 201 // 3 and m["ecc_max"] == 199 and int(m["dist"][63]) == 137 * 138
    finally:
        sim.close()


def _hv_views(g):
    v = np.zeros(g.n, _abi.NODE_VIEW_DTYPE)
    for i in range(g.n):
        v["up"][i], v["act_n"][i] = g.up[i], len(g.adj[i])
        v["act"][i][: len(g.adj[i])] = g.adj[i]
    return v


def test_ring_257():
    g = F.ring(257, "random", seed=2)
    sim = _boot(_gpu, 257)
    try:
        I.inject(sim, g.hv())
        m = sim.graph_metrics([0])
        assert (m["cl_closed"], m["cl_nodes"], m["cl_sum_q32"], m["ecc_max"]) == (0, 257, 0, 128)
        _links(sim, g, [0, 100, 256])
        _hist(sim, g)
    finally:
        sim.close()


@pytest.mark.parametrize("make", MAKES, ids=MAKE_IDS)
def test_nine_cliques_261(make):
    """29 9-cliques: all 8 lanes of k_gm_cluster_hv's groups, 1 << 32 a node"""
    g = F.cliques(9, 29, "random", seed=4)
    sim = _boot(make, 261)
    try:
        I.inject(sim, g.hv())
        m = _call(sim, "graph_metrics", [0, 260], 64, 0, 0)
        assert (m["cl_sum_q32"], m["links"], m["cl_closed"]) == (261 << 32, 261 * 8, 261 * 56)
        _links(sim, g, [0, 5, 64, 130, 191, 192, 255, 260], key="cliques261")
        h = _hist(sim, g)
        assert (h["components"], h["largest_component"], int(h["active_in"][8])) == (29, 9, 261)
        # every clique size below: 6, 7 and 8 links a row among them
        for k in range(2, 9):
            gk = F.cliques(k, 261 // k, "random", seed=k)
            gk = F.Graph(gk.adj + [[] for _ in range(261 - gk.n)])
            I.inject(sim, gk.hv())
            G.compare(_call(sim, "graph_metrics", [0, 260], 64, 0, 0), G.reference_rows(gk.rows(), [0, 260]))
            _hist(sim, gk)
    finally:
        sim.close()


def _owned_ranges(sim):
    """(lo, n) of every shard of every rank, from the ShardHeads of the handle's snapshot(s)"""
    ranked = hasattr(sim, "ranks")
    snaps = sim.snapshot() if ranked else [sim.snapshot()]
    cfgs = [r.cfg for r in sim.ranks] if ranked else [sim.cfg]
    return sorted((int(s.head["lo"]), int(s.head["n"])) for c, b in zip(cfgs, snaps) for s in I.layout(c, b).shards)


@pytest.mark.parametrize("make,hub,parts", list(zip(MAKES, [4097, 1366, 2049], [1, 3, 2])), ids=MAKE_IDS)
def test_in_star_4099(make, hub, parts):
    """in-degree 4098 on one word of indeg / next (every atomic on one address);
    the hub in the last, partial wave (ids 4096-4098), or the last id of the
    first shard / rank"""
    g = F.in_star(4099, hub)
    sim = _boot(make, 4099)
    try:
        I.inject(sim, g.hv())
        own = _owned_ranges(sim)
        assert len(own) == parts and (parts == 1 or own[0][0] + own[0][1] - 1 == hub), own
        assert hub // 64 == 4098 // 64 or parts > 1
        _links(sim, g, [0, hub, 4098, 64])
        h = _hist(sim, g)
        assert int(h["active_in"][63]) == 1 and h["components"] == 1 and h["largest_component"] == 4099
        d = F.dead_tenth(g, seed=1, keep=(hub,))
        I.inject(sim, d.hv(), allow=("dead",))
        _links(sim, d, [0, hub, 4098, 64])
        _hist(sim, d)
        d = F.dead_tenth(g, seed=1, keep=(1,))
        d.up[hub] = False                                                      # (every link dangling)
        I.inject(sim, d.hv(), allow=("dead",))
        _links(sim, d, [1, hub])
        assert _hist(sim, d)["active_links"] == 0
    finally:
        sim.close()


def test_directed_path_1000():
    g = F.path(1000, "random", directed=True, seed=2)
    sim = _boot(_gpu, 1000)
    try:
        I.inject(sim, g.hv())
        src = [g.perm[0], g.perm[999], g.perm[500], g.perm[937]]
        m = sim.graph_metrics(src)
        assert m["pairs_unreached"] == 4 * 999 - 999 - 499 - 62 and int(m["dist"][63]) == 937 + 437
        _links(sim, g, src)
        r = sim.resilience([g.perm[0]], [0])
        assert (int(r["no_in"][0]), int(r["no_out"][0]), int(r["reached"][0])) == (1, 1, 999)
        h = _hist(sim, g)
        assert (h["symmetric_links"], h["components"]) == (0, 1)
    finally:
        sim.close()


def test_matching_and_isolated_1001():
    g = F.matching(1001, 300, "random", seed=4)
    sim = _boot(_gpu, 1001)
    try:
        I.inject(sim, g.hv())
        _links(sim, g, [g.perm[0], g.perm[1], g.perm[1000], 1000])
        h = _hist(sim, g)
        assert (h["components"], h["largest_component"]) == (701, 2)
        e = F.Graph([[] for _ in range(1001)])                                 # no link at all
        I.inject(sim, e.hv())
        _links(sim, e, [0, 1000])
        assert _hist(sim, e)["components"] == 1001
    finally:
        sim.close()


@pytest.mark.parametrize("kind", ["hv", "scamp"])
@pytest.mark.parametrize("k", [3, 6])
def test_dirty_rows_261(k, kind):
    """261 nodes of 3-cliques, and of 6-cliques with 3 isolated nodes (a
    9-clique's row is full: it has no room for dirt; a 6-clique's 5 links
    leave room for an own id and a repeat, rows of 6 and 7 entries), with a
    dead tenth: L is what the clean rows give; the SCAMP statistics count
    the dirt"""
    c = F.cliques(k, 261 // k, "random", seed=5)
    c = F.Graph(c.adj + [[] for _ in range(261 - c.n)])
    base = F.dead_tenth(c, seed=2, keep=(0,))
    g = F.dirty(base, 8 if kind == "hv" else 128, seed=3)
    assert max(len(a) for a in g.adj) == k + 1 and any(len(set(a)) < len(a) for a in g.adj)
    assert G.links_of(g.rows()) == G.links_of(base.rows()) and g.adj != base.adj
    sim = _boot(_gpu, 261, kind)
    try:
        I.inject(sim, g.hv() if kind == "hv" else g.scamp(), allow=("self", "dup", "dead"))
        _links(sim, g, [0, 1, 130, 260])
        G.compare(sim.graph_metrics([0, 1, 130, 260]), G.reference_rows(base.rows(), [0, 1, 130, 260]))
        if kind == "scamp":
            _shist(sim, g.scamp())
            s = sim.strategy_histograms()
            assert s["self_entries"] and s["duplicate_entries"] and s["dangling_links"]
    finally:
        sim.close()


def test_grid_40x40_latency_and_dead_source():
    g = F.grid(40, 40, "random", seed=6)
    corner = g.closed["corner"]
    sim = _boot(_gpu, 1600)
    try:
        I.inject(sim, g.hv())
        m = sim.graph_metrics([corner])
        assert (m["ecc_max"], m["dist_sum"], int(m["dist"][63])) == (78, g.closed["corner_dist_sum"], 136)
        _links(sim, g, [corner, 0, 799, 1599])
        _hist(sim, g)
        d = F.dead_tenth(g, seed=4, keep=(corner,))
        dead = d.up.index(False)
        I.inject(sim, d.hv(), allow=("dead",))
        _links(sim, d, [corner, dead, 1599 if d.up[1599] else corner ^ 1])
        lat = sim.latency_metrics([dead, corner])
        assert lat["live_mask"] == 2 and int(lat["reach"][0]) == 0
    finally:
        sim.close()


FAMILIES = {
    "path": lambda: F.path(300, "random", seed=1),
    "dipath": lambda: F.path(300, "zigzag", directed=True),
    "ring": lambda: F.ring(257, "random", seed=2),
    "cliques9": lambda: F.cliques(9, 29, "random", seed=4),
    "matching": lambda: F.matching(301, 120, "random", seed=4),
    "grid": lambda: F.grid(17, 13, "random", seed=6),
    "bridge": lambda: F.two_cliques_one_bridge(8, "random", seed=9),
    "in_star": lambda: F.in_star(321, 319),
    "tree": lambda: F.binary_tree(255, "random", seed=6),
    "out_star8": lambda: F.out_star(300, 299, fan=8, seed=2),
}


@pytest.mark.parametrize("kind", ["hv", "scamp"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_with_a_dead_tenth(name, kind):
    """every family clean and again with a tenth of its nodes down (their
    neighbours' rows still name them), on HyParView and on SCAMP rows, whose
    CSR builder and clustering kernel are other code: the four link getters
    and the handle kind's histogram getter"""
    g = FAMILIES[name]()
    d = F.dead_tenth(g, seed=3, keep=(g.perm[0],))
    src = _uniq([g.perm[0], g.perm[g.n // 2], g.perm[g.n - 1], d.up.index(False)])
    sim = _boot(_gpu, g.n, kind)
    try:
        for x, allow in ((g, ()), (d, ("dead",))):
            I.inject(sim, x.hv() if kind == "hv" else x.scamp(), allow=allow)
            _links(sim, x, src)
            if kind == "hv":
                _hist(sim, x)
            else:
                _shist(sim, x.scamp())
    finally:
        sim.close()


# ---- components: a label that has to cross the whole path
@pytest.mark.parametrize("kind", ["hv", "scamp"])
@pytest.mark.parametrize("order", ["min_then_desc", "random"])
def test_path_12500_is_one_component(order, kind):
    """ids 0, n-1, n-2, ..., 1 along a path: plain min-label propagation
    moves the label 0 one hop an iteration, 12 499 hops in all"""
    g = F.path(12500, order, seed=1)
    sim = _boot(_gpu, g.n, kind)
    try:
        I.inject(sim, g.hv() if kind == "hv" else g.scamp())
        ms = []
        for _ in range(5):                              # (the whole getter's wall time, call by call)
            t0 = time.perf_counter()
            h = sim.histograms() if kind == "hv" else sim.strategy_histograms()
            ms.append(round((time.perf_counter() - t0) * 1e3, 1))
        print(f"cc path {order} {kind}: components {h['components']} largest {h['largest_component']} in {ms} ms")
        assert (h["components"], h["largest_component"]) == (1, 12500)
        if kind == "hv":
            _hist(sim, g)
        else:
            _shist(sim, g.scamp())
    finally:
        sim.close()


# ---- SCAMP rows
@pytest.mark.parametrize("make", [_gpu, _vshards(3)], ids=MAKE_IDS[:2])
def test_scamp_out_star_128(make):
    """a 128-id row at the hub, the last id of a shard; then the same hub
    with repeats and its own id, and an in-star over SCAMP rows"""
    hub = 666 if make is not _gpu else 1999
    g = F.out_star(2000, hub, fan=128, seed=1)
    sim = _boot(make, 2000, "scamp")
    try:
        I.inject(sim, g.scamp())
        _shist(sim, g.scamp())
        _links(sim, g, _uniq([hub, 0, g.adj[hub][0], 1998]))
        m = _call(sim, "graph_metrics", [hub], 64, 0, 0)
        assert (m["cl_pairs"], m["cl_closed"], int(m["reach"][0])) == (128 * 127, 0, 128)
        d = F.Graph(g.adj)
        d.adj[hub] = d.adj[hub][:100] + [hub] + d.adj[hub][:27]
        rows = d.scamp()
        for i in g.adj[hub][:40]:
            rows[i]["in_view"] = [hub, hub, i]
        I.inject(sim, rows, allow=("self", "dup"))
        _shist(sim, rows)
        s = _call(sim, "strategy_histograms")
        assert (s["self_entries"], s["duplicate_entries"], s["links"], s["in_view_confirmed"]) == (1, 27, 100, 40)
        star = F.in_star(2000, hub)
        I.inject(sim, star.scamp())
        _shist(sim, star.scamp())
        _links(sim, star, [0, hub])
    finally:
        sim.close()


# ---- the broadcast tree
def _tree(sim, rows, root, max_levels=0):
    T.compare(_call(sim, "tree_metrics", root, max_levels), T.reference_rows(rows, root, max_levels))


def test_tree_binary_4095():
    g = F.binary_tree(4095, "random", seed=6)
    root = g.closed["root"]
    rows = F.tree_rows(g.n, g.adj, root)
    sim = _boot(_gpu, g.n)
    try:
        I.inject(sim, rows)
        m = sim.tree_metrics(root)
        assert (m["depth_max"], m["depth_sum"], m["reached"]) == (11, g.closed["depth_sum"], 4094)
        _tree(sim, rows, root)
        _tree(sim, rows, g.perm[1])                     # (no slot of this root anywhere: the common sets, empty)
    finally:
        sim.close()


@pytest.mark.parametrize("make", [_gpu, _loop(2)], ids=["gpu", "loopback-2"])
def test_tree_chain_4200_hits_the_cap(make):
    g = F.path(4200, "random", directed=True, seed=7)
    root = g.closed["end"]
    rows = F.tree_rows(g.n, g.adj, root)
    sim = _boot(make, g.n)
    try:
        I.inject(sim, rows)
        m = _call(sim, "tree_metrics", root, 0)
        assert (m["levels"], m["truncated"], m["reached"], m["depth_max"]) == (CAP, 1, CAP, CAP)
        _tree(sim, rows, root)
    finally:
        sim.close()


def test_tree_full_pool_and_mixed_slots():
    """a root with 64 eager entries (the pool full), and nodes that hold four
    roots' slots in mixed order with both identity forms and lazy runs"""
    n, root = 300, 17
    rng = np.random.Generator(np.random.PCG64([5, 0x74]))
    others = [i for i in range(n) if i != root]
    rows = []
    for i in range(n):
        if i == root:
            e = [int(x) for x in rng.permutation(others)[:64]]
            rows.append(dict(up=True, act=e[:8], common=[], slots=[(root | I.MAP_BIT, e, [])]))
            continue
        pick = [int(x) for x in rng.permutation([x for x in others if x != i])[:24]]
        roots = [int(r) for r in rng.permutation([root, 1, 2, 3])]
        slots = []
        for q, r in enumerate(roots):
            e = pick[6 * q: 6 * q + 3 + q]
            z = pick[6 * q + 3 + q: 6 * q + 6]
            slots.append((r | I.MAP_BIT, [x | (I.MAP_BIT if (x + q) % 3 == 0 else 0) for x in e], z))
        rows.append(dict(up=True, act=pick[:6], common=pick[20:24], slots=slots))
    sim = _boot(_gpu, n)
    try:
        I.inject(sim, rows)
        for r in (root, 1, 2, 3, 9):
            _tree(sim, rows, r)
        assert sim.tree_metrics(root)["eager_entries"] > 64 + 3 * 299 - 1
    finally:
        sim.close()


# ---- the relay flood
def _relay(sim, rows, cases, max_levels=0):
    src, dst, ttl = ([c[k] for c in cases] for k in range(3))
    m = _call(sim, "relay_reach", src, dst, ttl, max_levels)
    Y.compare(m, Y.reference_rows(rows, cases, max_levels))
    return m


@pytest.mark.parametrize("make", MAKES, ids=MAKE_IDS)
def test_relay_nine_clique_powers_of_eight(make):
    """ttl 1, 5 and 16 on a 9-clique towards a node nobody holds: 8^l copies
    on level l, merged into 9 entries; 8^16 = 2^48 of them expire"""
    g = F.clique_and_outsider(9)
    g = F.Graph(g.adj + [[] for _ in range(70 - g.n)], closed=g.closed)      # (more than one wave of nodes)
    rows = F.relay_rows(g)
    sim = _boot(make, g.n)
    try:
        I.inject(sim, F.relay_inject_rows(rows))
        cases = [(j % 9, 9, t) for j, t in enumerate([1, 5, 16] * 7)] + [(3, 4, 16), (9, 0, 16), (0, 69, 2)]
        m = _relay(sim, rows, cases)
        for j, t in enumerate([1, 5, 16] * 7):
            relays, expired, levels = F.clique_flood(9, t)
            assert (int(m["relays"][j]), int(m["expired"][j]), int(m["levels"][j])) == (relays, expired, levels)
        assert int(m["expired"][2]) == 1 << 48 and (m["direct_mask"] >> 21) & 1
        _relay(sim, rows, cases, 7)
    finally:
        sim.close()


def test_relay_path_target_beyond_the_ttl():
    g = F.path(40, "random", seed=3)
    rows = F.relay_rows(g)
    sim = _boot(_gpu, g.n)
    try:
        I.inject(sim, F.relay_inject_rows(rows))
        cases = [(g.perm[0], g.perm[k], t) for k, t in ((20, 16), (17, 16), (18, 16), (5, 3), (5, 4), (39, 16), (2, 1))]
        m = _relay(sim, rows, cases)
        assert int(m["delivered"][0]) == 0 and int(m["delivered"][4]) > 0
    finally:
        sim.close()


@pytest.mark.parametrize("make", MAKES, ids=MAKE_IDS)
def test_relay_bridge_64_cases(make):
    rows = F.bridge_relay_rows()
    cases = F.bridge_relay_cases(rows)
    sim = _boot(make, len(rows))
    try:
        I.inject(sim, F.relay_inject_rows(rows))
        m = _relay(sim, rows, cases)
        assert m["restarts"].any() and m["delivered"].any() and m["members_down"] == 3
        _relay(sim, rows, cases, 5)
    finally:
        sim.close()


@pytest.mark.parametrize("lanes,slots", [("8", "16"), ("1", "16"), ("8", "")], ids=["group-16slots", "lane-16slots", "group"])
def test_relay_bridge_small_table_and_lane_layouts(lanes, slots):
    """a fresh process a setting (the library reads both at the call): the
    bridge graph's 64 cases and the clique's 8^16 under a 16-slot table and
    the 8-lane-group layout"""
    env = dict(os.environ, PSIM_RELAY_LANES=lanes)
    env.pop("PSIM_RELAY_SLOTS", None)
    if slots:
        env["PSIM_RELAY_SLOTS"] = slots
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_synthetic_relay_run.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    rows = F.bridge_relay_rows()
    Y.compare(got["bridge"], Y.reference_rows(rows, F.bridge_relay_cases(rows)))
    g = F.clique_and_outsider(9)
    Y.compare(got["clique"], Y.reference_rows(F.relay_rows(g), [(0, 9, 16), (1, 9, 5)]))
