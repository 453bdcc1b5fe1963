"""Reference for psim_relay_reach (test infrastructure): every field of the
struct from node rows -- rows_of() of nodes() -- one case at a time, with plain
sets, dicts and Python ints.  It calls nothing of the engine, so a test can
apply it to the CPU oracle's rows and compare the engine against it.

A row is (up, act, common, conn): the node's active view, its pt_common entries
and its connection table, each a list of raw entries.  A case is (source,
target, ttl).  The definitions are the header's (psim_relay_reach), followed
literally:
  state(i, p), p != i and p live: conn(i) holds p | CONN_DOWN -> "down" if p is
    in act(i), else "none"; conn(i) holds plain p -> "connected"; p in act(i)
    -> "connected"; else (and for p == i or p not live) "none".
  out(i): the entries e of common(i) with e != i, each one send to e & ~MAP_BIT.
  forward(v, t, c): per e of out(v): connected -> relays += c and c copies at
    (p, t - 1) on the next level; else refused += c.
  origin: state(s, d) connected -> direct; else forward(s, T, 1).
  level l over the merged (v, t) -> c: d in act(v) and connected -> delivered;
    d in act(v) otherwise -> restarts += c, forward(v, T, c); d not in act(v)
    and t == 0 -> expired; else forward(v, t, c)."""
import numpy as np

MAP_BIT = 0x80000000
CONN_DOWN = 0x80000000
CASES = 64
MAX_TTL = 16
HIST_BINS = 64

CENSUS = ("n_up", "out_entries", "out_usable", "out_nonmember", "members_down")
SCALARS = CENSUS + ("cases_live", "live_mask", "direct_mask", "truncated_mask", "levels_max")
ARRAYS = ("delivered", "first_hop", "hop_sum", "relays", "refused", "expired", "restarts", "in_flight", "levels",
          "peak")
HISTS = ("out_degree",)


def rows_of(views):
    """(up, act, common, conn) per node from nodes()"""
    return [(bool(views["up"][i]),
             [int(x) for x in views["act"][i][: int(views["act_n"][i])]],
             [int(x) for x in views["pt_common"][i][: int(views["pt_common_n"][i])]],
             [int(x) for x in views["conn"][i][: int(views["conn_n"][i])]])
            for i in range(len(views))]


def row(act, common=None, conn=(), up=True):
    """a hand-made row; common defaults to the active view"""
    return (up, list(act), list(act if common is None else common), list(conn))


class _Net:
    def __init__(self, rows):
        self.rows = rows
        self.n = len(rows)
        self._sends = {}

    def sends(self, v):
        """forward()'s view of out(v), worked out once: [(p, connected)]"""
        if v not in self._sends:
            self._sends[v] = [(e & ~MAP_BIT, self.state(v, e & ~MAP_BIT) == "connected") for e in self.out(v)]
        return self._sends[v]

    def live(self, p):
        return 0 <= p < self.n and self.rows[p][0]

    def state(self, i, p):
        if p == i or not self.live(p):
            return "none"
        _, act, _, conn = self.rows[i]
        if (p | CONN_DOWN) in conn:
            return "down" if p in act else "none"
        if p in conn or p in act:
            return "connected"
        return "none"

    def out(self, i):
        return [e for e in self.rows[i][2] if e != i]


def zero():
    out = {k: 0 for k in SCALARS}
    for k in ARRAYS:
        out[k] = [0] * CASES
    out["out_degree"] = [0] * HIST_BINS
    return out


def reference_rows(rows, cases=(), max_levels=0):
    """rows: [(up, act, common, conn)] per node; cases: [(source, target, ttl)]"""
    net = _Net(rows)
    out = zero()
    for i in range(net.n):
        if not net.live(i):
            continue
        out["n_up"] += 1
        act = rows[i][1]
        usable = 0
        for e in net.out(i):
            p = e & ~MAP_BIT
            out["out_entries"] += 1
            if net.state(i, p) == "connected":
                usable += 1
            if p not in act:
                out["out_nonmember"] += 1
        out["out_usable"] += usable
        out["out_degree"][min(usable, HIST_BINS - 1)] += 1
        out["members_down"] += sum(1 for p in set(act) if net.state(i, p) == "down")
    cases = [tuple(int(x) for x in c) for c in cases]
    assert len(cases) <= CASES
    assert all(len(c) == 3 and 0 <= c[0] < net.n and 0 <= c[1] < net.n and c[0] != c[1] and 1 <= c[2] <= MAX_TTL
               for c in cases)
    cap = MAX_TTL if not max_levels or max_levels > MAX_TTL else int(max_levels)
    for j, (s, d, T) in enumerate(cases):
        if not (net.live(s) and net.live(d)):
            continue
        out["cases_live"] += 1
        out["live_mask"] |= 1 << j
        if net.state(s, d) == "connected":
            out["direct_mask"] |= 1 << j
            out["delivered"][j] = out["first_hop"][j] = out["hop_sum"][j] = 1
            continue
        nxt = {}

        def forward(v, t, c):
            for p, connected in net.sends(v):
                if connected:
                    out["relays"][j] += c
                    nxt[(p, t - 1)] = nxt.get((p, t - 1), 0) + c
                else:
                    out["refused"][j] += c
        forward(s, T, 1)
        lvl = 0
        while nxt and lvl < cap:
            lvl += 1
            cur, nxt = nxt, {}
            out["levels"][j] = lvl
            out["peak"][j] = max(out["peak"][j], len(cur))
            for (v, t), c in cur.items():
                if d in rows[v][1]:
                    if net.state(v, d) == "connected":
                        out["delivered"][j] += c
                        out["hop_sum"][j] += c * (lvl + 1)
                        if not out["first_hop"][j]:
                            out["first_hop"][j] = lvl + 1
                    else:
                        out["restarts"][j] += c
                        forward(v, T, c)
                elif t == 0:
                    out["expired"][j] += c
                else:
                    forward(v, t, c)
        if nxt:
            out["truncated_mask"] |= 1 << j
            out["in_flight"][j] = sum(nxt.values())
        out["levels_max"] = max(out["levels_max"], out["levels"][j])
    for k in ARRAYS + HISTS:
        out[k] = np.array(out[k], np.uint64)
    return out


def reference(views, cases=(), max_levels=0):
    return reference_rows(rows_of(views), cases, max_levels)


def slot(m, j, keys=ARRAYS):
    return {k: int(m[k][j]) for k in keys}


def compare(got, want):
    """field for field; `got` may carry more keys than the reference"""
    bad = []
    for k in ARRAYS + HISTS:
        g, x = np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)
        if not np.array_equal(g, x):
            at = int(np.flatnonzero(g != x)[0]) if g.shape == x.shape else -1
            bad.append(f"{k}[{at}]: {int(g[at])} != {int(x[at])}" if at >= 0 else k)
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append(f"{k}: {int(got[k])} != {int(want[k])}")
    assert not bad, bad


def grid(rows, seed, k=CASES):
    """k cases of seeded pairs with mixed ttls 1 .. MAX_TTL; slot 7 is a direct
    pair: a live node and a live active member of it other than itself"""
    out = [(s, d, 1 + (5 * j + seed) % MAX_TTL) for j, (s, d) in enumerate(pairs(len(rows), seed, k))]
    net = _Net(rows)
    s, d = next((i, p) for i in range(seed % len(rows), len(rows)) if rows[i][0]
                for p in rows[i][1] if net.state(i, p) == "connected")
    out[7] = (s, d, out[7][2])
    return out


def pairs(n, seed, k=CASES, salt=0x72):
    """k seeded (source, target) pairs, source != target"""
    rng = np.random.Generator(np.random.PCG64([seed, salt]))
    out = []
    while len(out) < k:
        s, d = (int(x) for x in rng.integers(0, n, size=2))
        if s != d:
            out.append((s, d))
    return out
