"""The graph families (tests/_graph_families.py) against their closed forms,
through the same plain references the GPU tests compare the kernels with: at
these shapes -- distance 63 and more, the level cap itself, in-degree n - 1,
thousands of components, 8^16 copies -- the references have not been seen
either, so here each is held against arithmetic that needs no search.  Then
the injection's host side: the refusals of inject()'s validators and the
byte layout mirror's dtypes.  No GPU."""
import numpy as np
import pytest

import _gossip as P
import _graph_families as F
import _graph_metrics as G
import _latency as Q
import _overlay_inject as I
import _relay as Y
import _resilience as R
import _tree_metrics as T
from partisan_amd import _abi
from partisan_amd.sim import default_config

CAP = G.MAX_LEVELS


# ---- placement
@pytest.mark.parametrize("order", F.ORDERS)
@pytest.mark.parametrize("n", [1, 2, 7, 64, 65])
def test_place_is_a_permutation(order, n):
    assert sorted(F.place(n, order, 3)) == list(range(n))


def test_min_then_desc_reads_as_the_issue_says():
    assert F.place(6, "min_then_desc") == [0, 5, 4, 3, 2, 1]
    assert F.place(6, "zigzag") == [0, 5, 1, 4, 2, 3]


# ---- graph metrics
@pytest.mark.parametrize("order", F.ORDERS)
@pytest.mark.parametrize("n", [2, 63, 64, 65, 200])
def test_path_from_an_end(n, order):
    g = F.path(n, order, seed=5)
    c = g.closed
    m = G.reference_rows(g.rows(), [c["end"]])
    assert m["links"] == c["links"] == 2 * (n - 1)
    assert (m["dist_sum"], m["ecc_max"], int(m["ecc"][0])) == (n * (n - 1) // 2, n - 1, n - 1)
    assert int(m["dist"][63]) == max(n - 63, 0) == c["end_far"]
    assert all(int(m["dist"][d]) == (1 if d < n else 0) for d in range(1, 63))
    assert (m["pairs_reached"], m["pairs_unreached"], m["truncated"]) == (n - 1, 0, 0)
    assert (m["cl_closed"], m["cl_sum_q32"]) == (0, 0) and m["cl_nodes"] == max(n - 2, 0)


@pytest.mark.parametrize("n,levels,trunc,reached", [(CAP, CAP, 0, CAP - 1), (CAP + 1, CAP, 1, CAP),
                                                    (CAP + 2, CAP, 1, CAP), (4200, CAP, 1, CAP)])
def test_path_at_the_level_cap(n, levels, trunc, reached):
    """deepest = min(n - 1, cap); truncated exactly when level `cap` found a node"""
    g = F.path(n, "ident")
    m = G.reference_rows(g.rows(), [0])
    assert (m["levels"], m["truncated"], m["pairs_reached"]) == (levels, trunc, reached)
    assert m["pairs_unreached"] == n - 1 - reached
    assert m["dist_sum"] == reached * (reached + 1) // 2 and int(m["dist"][63]) == reached - 62
    r = R.reference_rows(g.rows(), [(0, 0, 0)])
    assert (r["levels"], r["truncated"], int(r["reached"][0]), int(r["ecc"][0])) == (levels, trunc, reached, min(n - 1, CAP))
    p = P.reference_rows(g.rows(), [(0, 0, 0, 0)])
    assert (p["levels"], p["truncated"], int(p["reached"][0])) == (levels, trunc, reached)


def test_directed_path():
    n = 1000
    g = F.path(n, "random", directed=True, seed=2)
    m = G.reference_rows(g.rows(), [g.perm[0], g.perm[n - 1], g.perm[500]])
    assert [int(x) for x in m["reach"][:3]] == [n - 1, 0, n - 1 - 500]
    assert m["pairs_unreached"] == 3 * (n - 1) - (n - 1) - (n - 1 - 500)
    assert (m["links"], m["cl_nodes"]) == (n - 1, 0)
    r = R.reference_rows(g.rows(), [(g.perm[0], 0, 0)])
    assert (int(r["no_in"][0]), int(r["no_out"][0])) == (1, 1)


@pytest.mark.parametrize("n", [4, 5, 64, 257])
def test_ring(n):
    g = F.ring(n, "random", seed=n)
    m = G.reference_rows(g.rows(), [g.perm[0]])
    c = g.closed
    for k in ("links", "cl_nodes", "cl_closed", "cl_pairs", "cl_sum_q32"):
        assert m[k] == c[k], k
    assert m["cl_closed"] == 0 and m["cl_nodes"] == n
    assert (m["ecc_max"], m["dist_sum"]) == (n // 2, c["dist_sum_one"])


@pytest.mark.parametrize("k", range(2, 10))
def test_cliques(k):
    copies = 3
    g = F.cliques(k, copies, "random", seed=k)
    m = G.reference_rows(g.rows(), [0])
    c = g.closed
    assert m["links"] == copies * k * (k - 1) == c["links"]
    if k >= 3:
        assert m["cl_sum_q32"] == (copies * k) << 32 == c["cl_sum_q32"]       # exactly 1 << 32 a node
        assert m["cl_closed"] == m["cl_pairs"] == c["cl_pairs"]
    else:
        assert (m["cl_nodes"], m["cl_sum_q32"]) == (0, 0)
    assert (int(m["reach"][0]), m["ecc_max"]) == (k - 1, 1)
    h = F.histograms_reference(g.rows())
    assert (h["components"], h["largest_component"], h["symmetric_links"]) == (copies, k, c["links"])
    assert int(h["active_in"][k - 1]) == copies * k == int(h["active_out"][k - 1])


def test_in_star_saturates_the_in_degree_bin():
    n = 4099
    g = F.in_star(n, hub=4095)
    h = F.histograms_reference(g.rows())
    assert int(h["active_in"][63]) == 1 and int(h["active_in"][0]) == n - 1
    assert int(h["active_out"][1]) == n - 1 and int(h["active_out"][0]) == 1
    assert (h["active_links"], h["symmetric_links"], h["components"], h["largest_component"]) == (n - 1, 0, 1, n)
    m = G.reference_rows(g.rows(), [0, 4095])
    assert [int(x) for x in m["reach"][:2]] == [1, 0] and m["cl_nodes"] == 0


def test_out_star():
    g = F.out_star(2000, hub=1999, fan=128, seed=1)
    assert g.max_out() == 128 and len(set(g.adj[1999])) == 128
    m = G.reference_rows(g.rows(), [1999])
    assert (m["links"], m["cl_nodes"], m["cl_pairs"], m["cl_closed"]) == (128, 1, 128 * 127, 0)
    assert int(m["reach"][0]) == 128


@pytest.mark.parametrize("n,pairs", [(1001, 300), (10, 0), (10, 5)])
def test_matching_components(n, pairs):
    g = F.matching(n, pairs, "random", seed=4)
    h = F.histograms_reference(g.rows())
    assert (h["components"], h["largest_component"]) == (n - pairs, 2 if pairs else 1)
    assert (h["active_links"], h["symmetric_links"]) == (2 * pairs, 2 * pairs)
    assert int(h["active_out"][0]) == n - 2 * pairs == g.closed["isolated"]


@pytest.mark.parametrize("order", F.ORDERS)
def test_path_components_any_order(order):
    g = F.path(12500, order, seed=1)
    h = F.histograms_reference(g.rows())
    assert (h["components"], h["largest_component"], h["active_links"]) == (1, 12500, 2 * 12499)


def _cc_model(rows):
    """k_cc_hook / k_cc_jump as the library runs them, one thread after the
    other in id order: (labels, passes).  Roots are hooked, the larger under
    the smaller; a pass that hooks nothing ends the loop."""
    n = len(rows)
    L = [i if rows[i][0] else None for i in range(n)]
    passes = 0
    while True:
        passes += 1
        changed = False
        for i in range(n):
            if L[i] is None:
                continue
            for p in rows[i][1]:
                if p == i or L[p] is None:
                    continue
                a, b = L[i], L[p]
                while L[a] != a:
                    a = L[a]
                while L[b] != b:
                    b = L[b]
                if a != b:
                    L[max(a, b)] = min(L[max(a, b)], min(a, b))
                    changed = True
        for i in range(n):
            if L[i] is not None:
                r = L[i]
                while L[r] != r:
                    r = L[r]
                L[i] = r
        if not changed:
            return L, passes


@pytest.mark.parametrize("order", F.ORDERS)
def test_root_hooking_model_on_paths(order):
    """the order that costs plain min-label propagation one pass a hop costs
    root hooking a handful"""
    g = F.path(4200, order, seed=1)
    L, passes = _cc_model(g.rows())
    assert set(L) == {0} and passes <= 16


def test_root_hooking_model_counts_components():
    for g in (F.matching(1001, 300, "random", seed=4), F.cliques(9, 29, "random", seed=4),
              F.dead_tenth(F.grid(20, 20, "random", seed=3), seed=1), F.in_star(500, 499),
              F.path(300, "zigzag", directed=True)):
        L, passes = _cc_model(g.rows())
        sizes = {}
        for x in L:
            if x is not None:
                sizes[x] = sizes.get(x, 0) + 1
        h = F.histograms_reference(g.rows())
        assert (len(sizes), max(sizes.values())) == (h["components"], h["largest_component"]) and passes <= 16


def test_grid_from_a_corner():
    g = F.grid(7, 5, "random", seed=1)
    m = G.reference_rows(g.rows(), [g.closed["corner"]])
    assert (m["links"], m["ecc_max"], m["dist_sum"]) == (g.closed["links"], 10, g.closed["corner_dist_sum"])
    assert m["cl_closed"] == 0


def test_two_cliques_one_bridge():
    g = F.two_cliques_one_bridge(8, "zigzag")
    m = G.reference_rows(g.rows(), list(range(16)))
    assert m["ecc_max"] == 3 and m["links"] == g.closed["links"] and g.max_out() == 8
    a, b = g.closed["bridge"]
    assert sorted(int(x) for x in m["ecc"][:16]).count(2) == 2 and int(m["ecc"][a]) == int(m["ecc"][b]) == 2


def test_dead_tenth_and_dirty_keep_the_link_set():
    g = F.cliques(9, 29, "random", seed=3)
    d = F.dirty(g, 8)                                   # (9-clique rows are full: nothing fits)
    assert d.adj == g.adj
    g = F.cliques(6, 40, "random", seed=3)
    d = F.dirty(g, 8, seed=1)
    assert d.adj != g.adj and G.links_of(d.rows()) == G.links_of(g.rows())
    assert any(i in a for i, a in enumerate(d.adj)) and any(len(set(a)) < len(a) for a in d.adj)
    x = F.dead_tenth(g, seed=2, keep=(0,))
    assert x.up[0] and 0.03 < x.up.count(False) / x.n < 0.25
    assert G.reference_rows(x.rows())["n_up"] == x.up.count(True)


# ---- relay: copies on a clique as a sum of powers
@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("ttl", [1, 5, 16])
def test_relay_clique_sum_of_powers(k, ttl):
    g = F.clique_and_outsider(k)
    m = Y.reference_rows(F.relay_rows(g), [(0, k, ttl), (k - 1, k, ttl)])
    relays, expired, levels = F.clique_flood(k, ttl)
    for j in range(2):
        assert (int(m["relays"][j]), int(m["expired"][j]), int(m["levels"][j])) == (relays, expired, levels)
        assert (int(m["delivered"][j]), int(m["refused"][j]), int(m["in_flight"][j])) == (0, 0, 0)
    assert m["truncated_mask"] == 0 and m["direct_mask"] == 0
    if (k, ttl) == (9, 16):
        assert expired == 1 << 48 and relays > 1 << 48          # 64-bit sums


# ---- tree
def test_binary_tree_depths():
    n = 4095
    g = F.binary_tree(n, "random", seed=6)
    root = g.closed["root"]
    m = T.reference_rows(F.tree_rows(n, g.adj, root), root)
    assert (m["depth_max"], m["depth_sum"], m["reached"], m["unreached"]) == (11, g.closed["depth_sum"], n - 1, 0)
    assert m["eager_links"] == n - 1 and m["slot_nodes"] == n


# ---- latency against Floyd-Warshall
@pytest.mark.parametrize("make", [lambda: F.grid(12, 11, "random", seed=2), lambda: F.ring(150, "zigzag"),
                                  lambda: F.dead_tenth(F.two_cliques_one_bridge(8), seed=1, keep=(0,)),
                                  lambda: F.path(200, "random", directed=True, seed=9)],
                         ids=["grid", "ring", "bridge_dead", "dipath"])
def test_latency_against_floyd_warshall(make):
    g = make()
    assert g.n <= 200
    nb = Q.links_rows(g.rows())
    seed = 11
    fw = Q.floyd_warshall(nb, lambda i, p: Q.latency(seed, i, p))
    src = sorted(nb)[:: max(1, len(nb) // 8)][:8]
    m = Q.reference_links(nb, seed, src)
    for j, s in enumerate(src):
        ds = [d for (a, v), d in fw.items() if a == s and v != s]
        assert (int(m["reach"][j]), int(m["lat_sum"][j]), int(m["lat_ecc"][j])) == (len(ds), sum(ds), max(ds, default=0))


# ---- the injection's host side
def _cfg(n=16, **kw):
    return default_config(n_nodes=n, **kw)


def _scamp(n=16):
    return _cfg(n, manager=_abi.MANAGER_PLUGGABLE, strategy=_abi.STRATEGY_SCAMP_V2)


@pytest.mark.parametrize("rows,why", [
    ([dict(act=[16])] + [dict()] * 15, "names no node"),
    ([dict(act=[0xFFFFFFFF])] + [dict()] * 15, "names no node"),
    ([dict(act=list(range(1, 10)))] + [dict()] * 15, "the cap is 8"),
    ([dict(common=list(range(1, 10)))] + [dict()] * 15, "the cap is 8"),
    ([dict(common=[16 | I.MAP_BIT])] + [dict()] * 15, "names no node"),
    ([dict(conn=list(range(1, 10)))] + [dict()] * 15, "the cap is 8"),
    ([dict(conn=[3 | I.CONN_CLOSING])] + [dict()] * 15, "names no node"),
    ([dict(slots=[(1 | I.MAP_BIT, [], [])] * 5)] + [dict()] * 15, "root slots"),
    ([dict(slots=[(1 | I.MAP_BIT, [], []), (1 | I.MAP_BIT, [], [])])] + [dict()] * 15, "two slots of one root"),
    ([dict(slots=[(1, [], [])])] + [dict()] * 15, "MAP_BIT"),
    ([dict(slots=[(1 | I.MAP_BIT, [2] * 40, []), (2 | I.MAP_BIT, [3] * 25, [])])] + [dict()] * 15, "eager pool"),
    ([dict(slots=[(1 | I.MAP_BIT, [], [2] * 65)])] + [dict()] * 15, "the cap is 64"),
    ([dict(slots=[(1 | I.MAP_BIT, [99], [])])] + [dict()] * 15, "names no node"),
    ([dict(view=[1])] + [dict()] * 15, "unknown field"),
    ([dict(passive=[1])] + [dict()] * 15, "unknown field"),
    ([dict()] * 15, "15 rows for 16"),
    ([dict(act=[0])] + [dict()] * 15, "holds the node itself"),
    ([dict(act=[1, 1])] + [dict()] * 15, "repeats an id"),
    ([dict(act=[1]), dict(up=False)] + [dict()] * 14, "names a dead node"),
])
def test_inject_refuses_out_of_domain_hv_rows(rows, why):
    with pytest.raises(I.DomainError, match=why):
        I.validate(_cfg(), rows)


@pytest.mark.parametrize("rows,why", [
    ([dict(view=list(range(129)))] + [dict()] * 199, "the cap is 128"),
    ([dict(view=[200])] + [dict()] * 199, "names no node"),
    ([dict(in_view=[200])] + [dict()] * 199, "names no node"),
    ([dict(act=[1])] + [dict()] * 199, "unknown field"),
    ([dict(view=[0])] + [dict()] * 199, "holds the node itself"),
])
def test_inject_refuses_out_of_domain_scamp_rows(rows, why):
    with pytest.raises(I.DomainError, match=why):
        I.validate(_scamp(200), rows)


def test_inject_dirt_only_where_allowed_and_known_kinds_only():
    rows = [dict(act=[0, 1, 1, 2]), dict(), dict(up=False)] + [dict()] * 13
    out = I.validate(_cfg(), rows, allow=("self", "dup", "dead"))
    assert out[0]["act"] == [0, 1, 1, 2] and out[2]["up"] is False and out[1]["slots"] == []
    with pytest.raises(I.DomainError, match="unknown kind of dirt"):
        I.validate(_cfg(), rows, allow=("wild",))
    for strategy in (_abi.STRATEGY_FULL, _abi.STRATEGY_SCAMP_V1):
        with pytest.raises(I.DomainError, match="SCAMP v2 handles only"):
            I.validate(_cfg(manager=_abi.MANAGER_PLUGGABLE, strategy=strategy), [dict()] * 16)


def test_inject_validates_before_any_device_call():
    class NoDevice:
        cfg = _cfg()

        def __getattr__(self, name):
            raise AssertionError(f"inject touched the handle ({name}) before refusing")
    with pytest.raises(I.DomainError):
        I.inject(NoDevice(), [dict(act=[16])] + [dict()] * 15)


# ---- the dtype mirror
HDR_OFFSETS = {  # Hdr of psim_device.h, written out: field -> (offset, bytes)
    "rng": (0, 8), "start_round": (8, 4), "join_contact": (12, 4), "epoch": (16, 4), "aux": (20, 4), "have": (24, 4),
    "trk_round": (28, 4), "trk_hop": (32, 4), "act_n": (36, 1), "pas_n": (37, 1), "sent_n": (38, 1),
    "sent_head": (39, 1), "recv_n": (40, 1), "recv_head": (41, 1), "all_n": (42, 1), "com_n": (43, 1),
    "conn_n": (44, 1), "conn_dn": (45, 1), "out_n": (46, 1), "conn_cl": (47, 1), "pad1": (48, 16),
}


def test_hdr_dtype_mirror():
    assert I.HDR.itemsize == 64
    assert {k: (I.HDR.fields[k][1], I.HDR.fields[k][0].itemsize) for k in I.HDR.names} == HDR_OFFSETS
    # header word 11 holds the connection table's counts (HW_CONN), words 13-15 the extension rows
    assert I.HDR.fields["conn_n"][1] == 4 * 11 and I.HDR.fields["pad1"][1] == 4 * 12


def test_head_dtype_mirrors():
    assert I.SNAP_HEAD.itemsize == 8 * 4 + 8 + 4 * 4 + 2 * _abi.MSG_SLOTS * 4 == 568
    assert I.SNAP_HEAD.fields["round"][1] == 32 and I.SNAP_HEAD.fields["slot_tab"][1] == 56
    assert I.SHARD_HEAD.itemsize == 48 and I.SHARD_HEAD.fields["out_rows"][1] == 32
    assert I.SHARD_HEAD.fields["pad"][1] == 24 and I.SHARD_HEAD.fields["pad2"][1] == 36


def test_layout_fails_loudly_on_a_wrong_snapshot():
    cfg = _cfg()
    with pytest.raises(I.LayoutError, match="shorter"):
        I.layout(cfg, b"\0" * 10)
    head = np.zeros(1, I.SNAP_HEAD)
    head["magic"], head["abi"], head["n_nodes"], head["world"] = I.SNAP_MAGIC, _abi.PSIM_ABI_VERSION, 16, 1
    head["n_local_shards"] = 1
    with pytest.raises(I.LayoutError, match="ShardHead passes"):
        I.layout(cfg, head.tobytes())
    sh = np.zeros(1, I.SHARD_HEAD)
    sh["n"] = 16
    body = sum(int(np.prod(shape)) * np.dtype(dt).itemsize for _, dt, shape in I._sections(head[0], sh[0]))
    ok = head.tobytes() + sh.tobytes() + b"\0" * body
    lay = I.layout(cfg, ok)
    assert lay.shards[0].hdr.shape == (16,) and lay.shards[0].conn.shape == (16, 8) and lay.tobytes() == ok
    with pytest.raises(I.LayoutError, match="add up"):
        I.layout(cfg, ok + b"\0")
    with pytest.raises(I.LayoutError, match="passes the end"):
        I.layout(cfg, ok[:-1])
    bad = head.copy()
    bad["abi"] += 1
    with pytest.raises(I.LayoutError, match="abi"):
        I.layout(cfg, bad.tobytes() + ok[568:])
