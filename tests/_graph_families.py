"""Hand-built overlays for the getters (test infrastructure): pure functions
of (n, seed) that return a Graph -- per node id its out-links and whether it
is up -- and, where one exists, the closed form of what a getter must say.
The shape is laid out over positions 0..n-1 and `order` places position k at
id perm[k], so the same shape lands on different lanes, words and shards.

Nothing here calls the engine or a reference: test_graph_families.py checks
the references against the closed forms, test_gpu_synthetic_overlays.py the
kernels against the references."""
import numpy as np

MAP_BIT = 0x80000000
CONN_DOWN = 0x80000000
ORDERS = ("ident", "reversed", "random", "zigzag", "min_then_desc")


def place(n, order="ident", seed=0):
    """perm: position -> id"""
    if order == "ident":
        return list(range(n))
    if order == "reversed":
        return list(range(n - 1, -1, -1))
    if order == "random":
        return [int(x) for x in np.random.Generator(np.random.PCG64([seed, 0x67])).permutation(n)]
    if order == "zigzag":                       # 0, n-1, 1, n-2, ...
        return [k // 2 if k % 2 == 0 else n - 1 - k // 2 for k in range(n)]
    if order == "min_then_desc":                # 0, n-1, n-2, ..., 1
        return [0] + list(range(n - 1, 0, -1))
    raise KeyError(order)


class Graph:
    """adj[i]: the raw out-row of node i (ids, in row order); up[i]; perm:
    position -> id; closed: {field: value} known without any search"""

    def __init__(self, adj, perm=None, up=None, closed=None):
        self.adj = [list(a) for a in adj]
        self.n = len(adj)
        self.perm = list(range(self.n)) if perm is None else list(perm)
        self.up = [True] * self.n if up is None else list(up)
        self.closed = dict(closed or {})

    def rows(self):
        """[(up, [ids])]: what the graph, resilience and gossip references take"""
        return [(self.up[i], list(self.adj[i])) for i in range(self.n)]

    def hv(self):
        """inject() rows of a HyParView handle"""
        return [dict(up=self.up[i], act=list(self.adj[i])) for i in range(self.n)]

    def scamp(self):
        """inject() rows of a SCAMP v2 handle"""
        return [dict(up=self.up[i], view=list(self.adj[i])) for i in range(self.n)]

    def max_out(self):
        return max((len(a) for a in self.adj), default=0)


def _placed(n, links, perm, closed=None):
    adj = [[] for _ in range(n)]
    for a, b in links:                          # (positions)
        adj[perm[a]].append(perm[b])
    return Graph(adj, perm, closed=closed)


def path(n, order="ident", directed=False, seed=0):
    """positions 0 - 1 - ... - n-1; directed: k -> k + 1 only.  From the end
    perm[0]: every node reached, v at position k at distance k."""
    perm = place(n, order, seed)
    links = [(k, k + 1) for k in range(n - 1)]
    if not directed:
        links += [(k + 1, k) for k in range(n - 1)]
    links.sort()
    closed = dict(links=len(links), components=1 if n else 0, largest_component=n,
                  end=perm[0], end_dist_sum=n * (n - 1) // 2, end_ecc=n - 1, end_far=max(n - 63, 0),
                  cl_closed=0, symmetric_links=0 if directed else len(links))
    return _placed(n, links, perm, closed)


def ring(n, order="ident", seed=0):
    """a symmetric cycle, n >= 4: no triangle, every node two links"""
    assert n >= 4
    perm = place(n, order, seed)
    links = sorted([(k, (k + 1) % n) for k in range(n)] + [((k + 1) % n, k) for k in range(n)])
    return _placed(n, links, perm, dict(links=2 * n, cl_nodes=n, cl_closed=0, cl_pairs=2 * n, cl_sum_q32=0,
                                        components=1, largest_component=n, symmetric_links=2 * n,
                                        ecc=n // 2, dist_sum_one=(n // 2) * ((n + 1) // 2)))


def cliques(k, copies=1, order="ident", seed=0):
    """`copies` disjoint k-cliques, 2 <= k <= 9 (a HyParView row holds 8)"""
    assert 2 <= k <= 9
    n = k * copies
    perm = place(n, order, seed)
    links = [(c * k + a, c * k + b) for c in range(copies) for a in range(k) for b in range(k) if a != b]
    closed = dict(links=n * (k - 1), components=copies, largest_component=k, symmetric_links=n * (k - 1),
                  cl_nodes=n if k >= 3 else 0, cl_pairs=n * (k - 1) * (k - 2) if k >= 3 else 0,
                  cl_closed=n * (k - 1) * (k - 2) if k >= 3 else 0, cl_sum_q32=(n << 32) if k >= 3 else 0,
                  reach=k - 1, ecc=1)
    return _placed(n, links, perm, closed)


def in_star(n, hub=0):
    """every other node -> hub: in-degree n - 1 on one word"""
    adj = [[hub] if i != hub else [] for i in range(n)]
    return Graph(adj, closed=dict(links=n - 1, hub=hub, hub_in=n - 1, components=1, largest_component=n,
                                  symmetric_links=0, cl_nodes=0))


def out_star(n, hub=0, fan=None, seed=0):
    """hub -> `fan` other nodes (default: all others); fan above 8 needs SCAMP rows"""
    others = [i for i in range(n) if i != hub]
    if fan is not None:
        pick = np.random.Generator(np.random.PCG64([seed, 0x6f])).permutation(len(others))[:fan]
        others = [others[int(j)] for j in pick]
    adj = [list(others) if i == hub else [] for i in range(n)]
    m = len(others)
    return Graph(adj, closed=dict(links=m, hub=hub, components=n - m, largest_component=m + 1, isolated=n - m - 1,
                                  cl_nodes=1 if m >= 2 else 0, cl_closed=0, cl_pairs=m * (m - 1)))


def matching(n, pairs, order="ident", seed=0):
    """positions 2j <-> 2j + 1 for j < pairs; the other n - 2 pairs nodes isolated"""
    assert 2 * pairs <= n
    perm = place(n, order, seed)
    links = sorted([(2 * j, 2 * j + 1) for j in range(pairs)] + [(2 * j + 1, 2 * j) for j in range(pairs)])
    return _placed(n, links, perm, dict(links=2 * pairs, components=n - pairs, largest_component=2 if pairs else 1,
                                        isolated=n - 2 * pairs, symmetric_links=2 * pairs, cl_nodes=0))


def grid(w, h, order="ident", seed=0):
    """w x h lattice, 4-neighbour, symmetric; position y * w + x"""
    n = w * h
    perm = place(n, order, seed)
    links = []
    for y in range(h):
        for x in range(w):
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= x + dx < w and 0 <= y + dy < h:
                    links.append((y * w + x, (y + dy) * w + x + dx))
    m = 2 * ((w - 1) * h + (h - 1) * w)
    return _placed(n, links, perm, dict(links=m, components=1, largest_component=n, symmetric_links=m, cl_closed=0,
                                        corner=perm[0], corner_ecc=w + h - 2,
                                        corner_dist_sum=w * h * (w + h - 2) // 2))


def binary_tree(n, order="ident", seed=0):
    """position k -> 2k + 1, 2k + 2 (children only): depth of k = floor(log2(k + 1))"""
    perm = place(n, order, seed)
    links = [(k, c) for k in range(n) for c in (2 * k + 1, 2 * k + 2) if c < n]
    depth = [(k + 1).bit_length() - 1 for k in range(n)]
    return _placed(n, links, perm, dict(links=n - 1 if n else 0, root=perm[0] if n else None, depth_sum=sum(depth),
                                        depth_max=max(depth, default=0)))


def two_cliques_one_bridge(k, order="ident", seed=0):
    """two k-cliques, 2 <= k <= 8, position k - 1 <-> position k the bridge"""
    assert 2 <= k <= 8
    n = 2 * k
    perm = place(n, order, seed)
    links = [(c * k + a, c * k + b) for c in range(2) for a in range(k) for b in range(k) if a != b]
    links += [(k - 1, k), (k, k - 1)]
    return _placed(n, links, perm, dict(links=2 * k * (k - 1) + 2, components=1, largest_component=n, ecc=3,
                                        bridge=(perm[k - 1], perm[k])))


# ---- variants of any family
def _mix(z):
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & (1 << 64) - 1
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & (1 << 64) - 1
    return z ^ (z >> 31)


def dead_tenth(g, seed=0, keep=()):
    """the same rows with about a tenth of the nodes down (never one of `keep`);
    the rows of live nodes still name them: dead targets"""
    up = [i in keep or _mix(seed * 0x9E3779B9 + i + 1) % 10 != 0 for i in range(g.n)]
    return Graph(g.adj, g.perm, up)


def dirty(g, cap, seed=0):
    """the same link set L from dirty rows: where a row has room (cap: its
    capacity), a node's own id and a repeat of its first entry are added at
    seeded places -- the set of distinct live targets other than self stays"""
    rng = np.random.Generator(np.random.PCG64([seed, 0x64]))
    adj = []
    for i, a in enumerate(g.adj):
        a = list(a)
        if len(a) < cap and rng.integers(2):
            a.insert(int(rng.integers(len(a) + 1)), i)
        if a and len(a) < cap and rng.integers(2):
            a.insert(int(rng.integers(len(a) + 1)), next(x for x in a if x != i) if any(x != i for x in a) else i)
        adj.append(a)
    return Graph(adj, g.perm, g.up, {k: v for k, v in g.closed.items() if k in ("links", "components", "largest_component")})


# ---- the reference of psim_histograms' link fields (no other file has one)
HIST_BINS = 64


def histograms_reference(rows):
    """rows [(up, [ids])] of clean or dead-target rows (no repeat, no self):
    n_up, active_out (row length), active_in, active_links, symmetric_links,
    components and largest_component as include/partisan_gpu_sim.h defines them"""
    n = len(rows)
    up = [u for u, _ in rows]
    out = dict(n_up=sum(up), active_links=0, symmetric_links=0,
               active_in=np.zeros(HIST_BINS, np.uint64), active_out=np.zeros(HIST_BINS, np.uint64))
    indeg = [0] * n
    sets = [set(r) for _, r in rows]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, (u, r) in enumerate(rows):
        if not u:
            continue
        assert len(set(r)) == len(r) and i not in r, "histograms_reference takes clean rows"
        out["active_out"][min(len(r), HIST_BINS - 1)] += 1
        for p in r:
            if up[p]:
                out["active_links"] += 1
                indeg[p] += 1
                out["symmetric_links"] += 1 if i in sets[p] else 0
                parent[find(i)] = find(p)
    for i in range(n):
        if up[i]:
            out["active_in"][min(indeg[i], HIST_BINS - 1)] += 1
    sizes = {}
    for i in range(n):
        if up[i]:
            sizes[find(i)] = sizes.get(find(i), 0) + 1
    out["components"], out["largest_component"] = len(sizes), max(sizes.values(), default=0)
    return out


# ---- rows of the relay and tree getters
def relay_rows(g, common=None, conn=None):
    """_relay rows (up, act, common, conn): common defaults to the active view"""
    return [(g.up[i], list(g.adj[i]), list(g.adj[i] if common is None else common[i]),
             list(conn[i]) if conn else []) for i in range(g.n)]


def relay_inject_rows(rows):
    return [dict(up=u, act=a, common=c, conn=k) for u, a, c, k in rows]


def clique_and_outsider(k):
    """a k-clique on ids 0..k-1 and a live node k that nobody holds.  A
    transitive unicast from a clique node to it with ttl T floods the clique:
    level l carries (k-1)^l copies with ttl T - l, none is ever delivered, the
    copies of level T expire.  relays = sum of (k-1)^l over l = 1..T."""
    g = cliques(k)
    return Graph(g.adj + [[]], closed=dict(target=k))


def clique_flood(k, ttl):
    """(relays, expired, levels) of that flood"""
    return sum((k - 1) ** l for l in range(1, ttl + 1)), (k - 1) ** ttl, ttl


def bridge_relay_rows():
    """two 8-cliques and a bridge; the bridge ends hold each other (and one
    end a clique member) without a connection: restarts; two far nodes hold a
    plain connection beyond their view"""
    g = two_cliques_one_bridge(8, "random", seed=9)
    a, b = g.closed["bridge"]
    conn = [[] for _ in range(g.n)]
    conn[a] = [b | CONN_DOWN]
    conn[b] = [a | CONN_DOWN, g.adj[b][0] | CONN_DOWN]
    far = [i for i in range(g.n) if b not in g.adj[i] and i != b]
    conn[far[0]] = [b]
    conn[far[1]] = [b, far[2]]
    return relay_rows(g, conn=conn)


def bridge_relay_cases(rows):
    """64 seeded pairs, ttls 1 .. 16"""
    rng = np.random.Generator(np.random.PCG64([5, 0x72]))
    out = []
    while len(out) < 64:
        s, d = (int(x) for x in rng.integers(0, len(rows), size=2))
        if s != d:
            out.append((s, d, 1 + (3 * len(out)) % 16))
    return out


def tree_rows(n, eager, root, act=None):
    """_tree_metrics.node rows: node i holds one slot of `root` with eager[i]"""
    return [dict(up=True, act=list(act[i] if act else eager[i]), common=[],
                 slots=[(root | MAP_BIT, list(eager[i]), [])]) for i in range(n)]
