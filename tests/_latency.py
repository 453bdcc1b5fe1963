"""Reference for psim_latency_metrics (test infrastructure): every field of the
struct from node rows, in plain Python -- the latency oracle restated, a set
per row, Dijkstra with heapq for uncapped calls, a synchronous hop-bounded
Bellman-Ford for capped ones, Python-int arithmetic.  It calls nothing of the
engine, so a test can apply it to the CPU oracle's rows and compare the engine
against it.

Definitions (include/partisan_gpu_sim.h, psim_latency_metrics): w(i, p) =
psim_xbot_latency(seed, i, p).  L: ordered pairs (i, p), i live, p in i's row,
p != i, p live, a repeated id counted once.  D_r(s, v): the least total weight
of a path s -> v over L with at most r links.  Sweep r turns D_(r-1) into D_r;
the sweeps end after the first one that lowers no distance of any slot, or
after sweep `cap`.  A slot's last_sweep is the last sweep that lowered one of
its distances: the largest, over the nodes it reaches, of the fewest links a
cheapest path takes."""
import heapq

import numpy as np

import _graph_metrics as G
import _tree_metrics as T

HIST_BINS = 64
SOURCES = 64
MAX_SWEEPS = 4096
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15

CENSUS = ("n_up", "links", "link_cost_sum", "link_nodes", "worst_sum", "best_sum")
PATHS = ("sources_live", "live_mask", "lat_sum_all", "lat_max", "pairs_reached", "pairs_unreached", "sweeps",
         "truncated_mask")
TREE = ("tree_root_live", "tree_links", "tree_link_cost_sum", "tree_reached", "tree_lat_sum", "tree_lat_max",
        "tree_sweeps", "overlay_reached", "both_reached", "tree_lat_sum_both", "overlay_lat_sum_both", "slower",
        "faster", "tree_truncated")
SCALARS = CENSUS + PATHS + TREE
SLOTS = ("reach", "lat_sum", "lat_ecc", "last_sweep")
HISTS = ("link_cost", "lat")
ARRAYS = SLOTS + HISTS


# ---- the latency oracle (psim_device.h xbot_latency, restated)
def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def cell(seed, a):
    """a node's place on the 1024 x 1024 torus: 20 bits"""
    return mix64(seed ^ ((a * GOLDEN) & M64)) & 0xFFFFF


def _axis(a, b):
    d = abs(a - b)
    return min(d, 1024 - d)


def latency(seed, a, b):
    if a == b:
        return 0
    p, q = cell(seed, a), cell(seed, b)
    return _axis(p & 1023, q & 1023) + _axis(p >> 10, q >> 10)


# ---- link sets
def links_hv(views):
    """L of a HyParView / X-BOT handle's nodes(): {live i: N(i)}"""
    return G.links_of(G.rows_of(views, "hv"))


def links_scamp(views):
    """L of a SCAMP handle's strategy_nodes()"""
    return G.links_of(G.rows_of(views, "scamp"))


def links_rows(rows):
    """L of hand-built rows [(up, [ids])]"""
    return G.links_of(rows)


def tree_links(views, root):
    """T of `root` from nodes(), by the tree reference's row builder: {live i: E_i}"""
    rows = T.rows_of(views)
    live = {i for i, r in enumerate(rows) if r["up"]}
    out = {}
    for i in sorted(live):
        eag = T.sets_of(rows[i], root)[0]
        out[i] = {e & ~T.MAP_BIT for e in eag if e & ~T.MAP_BIT != i and e & ~T.MAP_BIT in live}
    return out


# ---- cheapest paths
def cap_of(max_sweeps):
    return MAX_SWEEPS if not max_sweeps or max_sweeps > MAX_SWEEPS else int(max_sweeps)


def dijkstra(nb, w, s):
    """({v: D(s, v)}, {v: the fewest links of a cheapest path}): Dijkstra over
    the pairs (weight, links), compared weight first"""
    best = {s: (0, 0)}
    heap, done = [(0, 0, s)], set()
    while heap:
        d, k, x = heapq.heappop(heap)
        if x in done:
            continue
        done.add(x)
        for p in nb[x]:
            c = (d + w(x, p), k + 1)
            if p not in best or c < best[p]:
                best[p] = c
                heapq.heappush(heap, (c[0], c[1], p))
    return {v: c[0] for v, c in best.items()}, {v: c[1] for v, c in best.items()}


def bellman_ford(nb, w, s, cap):
    """({v: D_R(s, v)}, the last sweep that lowered a distance): sweep r
    relaxes the links of the nodes that fell in sweep r - 1 from their
    distances as of the end of that sweep"""
    dist, front, last = {s: 0}, {s}, 0
    for r in range(1, cap + 1):
        new, fell = dict(dist), set()
        for x in front:
            for p in nb[x]:
                c = dist[x] + w(x, p)
                if p not in new or c < new[p]:
                    new[p] = c
                    fell.add(p)
        if not fell:
            break
        dist, front, last = new, fell, r
    return dist, last


def floyd_warshall(nb, w):
    """{(s, v): D(s, v)} over the live nodes: the third opinion of the CPU test"""
    ids = sorted(nb)
    ix = {v: k for k, v in enumerate(ids)}
    inf = 1 << 40
    d = np.full((len(ids), len(ids)), inf, np.int64)
    for i in ids:
        d[ix[i], ix[i]] = 0
        for p in nb[i]:
            d[ix[i], ix[p]] = min(d[ix[i], ix[p]], w(i, p))
    for k in range(len(ids)):
        d = np.minimum(d, d[:, k:k + 1] + d[k:k + 1, :])
    return {(s, v): int(d[ix[s], ix[v]]) for s in ids for v in ids if d[ix[s], ix[v]] < inf}


def sssp(nb, w, s, max_sweeps=0):
    """({v: D_R}, last sweep): Dijkstra for an uncapped call, else Bellman-Ford"""
    if not max_sweeps:
        dist, hops = dijkstra(nb, w, s)
        return dist, max(hops.values())
    return bellman_ford(nb, w, s, cap_of(max_sweeps))


def _zero():
    out = {k: 0 for k in SCALARS}
    for k in SLOTS:
        out[k] = np.zeros(SOURCES, np.uint64)
    for k in HISTS:
        out[k] = np.zeros(HIST_BINS, np.uint64)
    return out


def reference_links(nb, seed, sources=(), max_sweeps=0, tree=None, tree_root=None):
    """nb: L as {live i: N(i)}; tree: T as {live i: E_i} with tree_root, or
    None for a call without a root"""
    def w(i, p):
        return latency(seed, i, p)
    out = _zero()
    out["n_up"] = len(nb)
    for i, ni in nb.items():
        ws = [w(i, p) for p in ni]
        out["links"] += len(ws)
        out["link_cost_sum"] += sum(ws)
        for x in ws:
            out["link_cost"][min(x >> 4, HIST_BINS - 1)] += 1
        if ws:
            out["link_nodes"] += 1
            out["worst_sum"] += max(ws)
            out["best_sum"] += min(ws)
    sources = [int(s) for s in sources]
    assert len(sources) <= SOURCES and len(set(sources)) == len(sources)
    cap = cap_of(max_sweeps)
    live = [(j, s) for j, s in enumerate(sources) if s in nb]
    out["sources_live"] = len(live)
    lasts = []
    for j, s in live:
        out["live_mask"] |= 1 << j
        dist, last = sssp(nb, w, s, max_sweeps)
        lasts.append(last)
        out["last_sweep"][j] = last
        if last == cap:
            out["truncated_mask"] |= 1 << j
        for v, d in dist.items():
            if v == s:
                continue
            out["reach"][j] += 1
            out["lat_sum"][j] += d
            out["lat_ecc"][j] = max(int(out["lat_ecc"][j]), d)
            out["lat"][min(d >> 8, HIST_BINS - 1)] += 1
    if live:
        out["lat_sum_all"] = int(sum(int(x) for x in out["lat_sum"]))
        out["lat_max"] = int(out["lat_ecc"].max())
        out["pairs_reached"] = int(sum(int(x) for x in out["reach"]))
        out["pairs_unreached"] = len(live) * (out["n_up"] - 1) - out["pairs_reached"]
        out["sweeps"] = min(max(lasts) + 1, cap)
    if tree is None or tree_root not in nb:
        return out
    out["tree_root_live"] = 1
    for i, ei in tree.items():
        out["tree_links"] += len(ei)
        out["tree_link_cost_sum"] += sum(w(i, p) for p in ei)
    dt, last_t = sssp(tree, w, tree_root, max_sweeps)
    dl, last_l = sssp(nb, w, tree_root, max_sweeps)
    out["tree_sweeps"] = min(last_t + 1, cap)
    out["tree_truncated"] = 1 if cap in (last_t, last_l) else 0
    out["overlay_reached"] = len(dl) - 1
    for v, d in dt.items():
        if v == tree_root:
            continue
        out["tree_reached"] += 1
        out["tree_lat_sum"] += d
        out["tree_lat_max"] = max(out["tree_lat_max"], d)
        if v in dl:
            out["both_reached"] += 1
            out["tree_lat_sum_both"] += d
            out["overlay_lat_sum_both"] += dl[v]
            out["slower"] += 1 if d > dl[v] else 0
            out["faster"] += 1 if d < dl[v] else 0
    return out


def reference(views, seed, sources=(), max_sweeps=0, tree_root=None, kind="hv"):
    """views: nodes() (kind "hv") or strategy_nodes() (kind "scamp") of every node"""
    nb = G.links_of(G.rows_of(views, kind))
    tree = tree_links(views, tree_root) if tree_root is not None else None
    return reference_links(nb, seed, sources, max_sweeps, tree, tree_root)


def compare(got, want):
    """field for field, the first differing entry named; `got` may carry more
    keys than the reference"""
    bad = []
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append(f"{k}: {int(got[k])} != {int(want[k])}")
    for k in ARRAYS:
        g, w = np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)
        if not np.array_equal(g, w):
            j = int(np.flatnonzero(g != w)[0]) if g.shape == w.shape else -1
            bad.append(f"{k}[{j}]: {int(g[j])} != {int(w[j])}" if j >= 0 else f"{k}: shape {g.shape} != {w.shape}")
    assert not bad, bad
