"""Reference for psim_gossip_reach (test infrastructure): every field of the
struct from node rows -- _graph_metrics.rows_of() of nodes() or
strategy_nodes() -- one case at a time, with plain sets, a plain BFS and
Python-int arithmetic.  It calls nothing of the engine, so a test can apply it
to the CPU oracle's rows and compare the engine against it.

A case is (source, threshold, salt, fanout).  h(i, salt) =
mix64(fail_seed ^ mix64(salt << 32 | i)), u = h >> 32 and A_j are
_resilience's.  w(i, p, salt) = mix64(h(i, salt) + 0x9E3779B97F4A7C15 (p + 1)).
S_j(i): N(i) if fanout is 0 or >= |N(i)|, else the `fanout` ids p of N(i) with
the smallest (w, p) -- chosen among all of N(i), the nodes failed in the case
included.  A node sends once, when first reached, to S_j(i); a copy to a
target outside A_j is lost.  The senders are the source and every node reached
at a distance below the cap.  Levels, `levels` and `truncated` as
_resilience.reference_rows runs them."""
import numpy as np

from _graph_metrics import MAX_LEVELS, links_of
from _resilience import CASES, M64, SRC_B, mix64, u

GOLDEN = 0x9E3779B97F4A7C15

SCALARS = ("n_up", "links", "cases_live", "live_mask", "ecc_max", "levels", "truncated")
ARRAYS = ("alive", "reached", "hop_sum", "ecc", "sent", "lost")

FANOUTS = [1, 2, 3, 4, 5, 6, 8, 0]

# the anchors of the tests: computed with a throwaway model of the definitions
# above when the call was specified, on the oracle's rows of _resilience's
# anchors A and B (fail_seed 7) and of S.pl_v1_large_view(leave_from=10**9,
# leave_to=0, rounds=40) (fail_seed 5)
ANCHOR_A = {  # q: per fanout 1, 2, 3, 4, then 5 / 6 / 8 / 0 alike: sums over k of alive, reached, hop_sum, sent, lost; max ecc
    0: [(1624, 23, 60, 31, 0, 7), (1624, 1282, 13985, 2580, 0, 36), (1624, 1588, 10110, 4597, 0, 12),
        (1624, 1614, 8051, 5724, 0, 9), (1624, 1616, 7364, 6320, 0, 9)],
    3: [(1133, 13, 24, 21, 4, 4), (1133, 175, 1485, 366, 76, 22), (1133, 773, 7472, 2260, 592, 26),
        (1133, 908, 6477, 3246, 917, 21), (1133, 1056, 6815, 4155, 1223, 15)],
    5: [(794, 9, 19, 17, 6, 4), (794, 42, 200, 100, 38, 10), (794, 101, 513, 316, 124, 11),
        (794, 252, 1734, 936, 382, 17), (794, 353, 2392, 1459, 627, 15)],
}
V1_SOURCES = (0, 7, 90, 179)
ANCHOR_V1 = {  # fanout: (reached, sent, ecc) per source
    1: [(1, 2, 1), (2, 3, 2), (3, 4, 3), (2, 3, 2)],
    2: [(5, 10, 4), (9, 18, 5), (9, 17, 5), (6, 11, 5)],
    4: [(13, 26, 4), (19, 39, 5), (21, 43, 5), (14, 27, 5)],
    8: [(36, 82, 6), (39, 88, 5), (42, 94, 5), (37, 83, 7)],
    64: [(119, 301, 3), (119, 301, 4), (120, 304, 4), (120, 302, 4)],
    127: [(139, 384, 3), (139, 384, 4), (139, 384, 4), (140, 385, 4)],
    0: [(139, 384, 3), (139, 384, 4), (139, 384, 4), (140, 385, 4)],
}


def v1_cases():
    return [(s, 0, 1, f) for f in ANCHOR_V1 for s in V1_SOURCES]


ANCHOR_B = {1: (14752, 15, 28, 22, 0), 2: (14752, 95, 537, 153, 0), 3: (14752, 238, 1753, 443, 0),
            0: (14752, 1975, 15260, 4115, 0)}


def b_cases():
    return [(s, 0, k, f) for f in ANCHOR_B for k, s in enumerate(SRC_B)]


def h(i, salt, fail_seed):
    return mix64((fail_seed & M64) ^ mix64((salt << 32) | i))


def w(i, p, salt, fail_seed):
    return mix64(h(i, salt, fail_seed) + GOLDEN * (p + 1))


def chosen(i, ni, salt, fanout, fail_seed):
    """S_j(i) of the set ni = N(i)"""
    if not fanout or fanout >= len(ni):
        return set(ni)
    return set(sorted(ni, key=lambda p: (w(i, p, salt, fail_seed), p))[:fanout])


def grid(sources, q, fanouts=FANOUTS):
    """the report's cases of failed share q / 10: slot 8 fi + k =
    (sources[k], floor(q 2^32 / 10), salt k, fanouts[fi])"""
    return [(int(s), (q << 32) // 10, k, f) for f in fanouts for k, s in enumerate(sources)]


def reference_rows(rows, cases=(), fail_seed=0, max_levels=0):
    """rows: [(up, [ids])] per node; cases: [(source, threshold, salt, fanout)]"""
    out = {k: 0 for k in SCALARS}
    for k in ARRAYS:
        out[k] = np.zeros(CASES, np.uint64)
    nb = links_of(rows)
    out["n_up"] = len(nb)
    out["links"] = sum(len(v) for v in nb.values())
    cases = [tuple(int(x) for x in c) for c in cases]
    assert len(cases) <= CASES and all(len(c) == 4 and 0 <= c[0] < len(rows) for c in cases)
    cap = MAX_LEVELS if not max_levels or max_levels > MAX_LEVELS else int(max_levels)
    deepest = 0
    for j, (src, thr, salt, fan) in enumerate(cases):
        if src not in nb:
            continue
        out["cases_live"] += 1
        out["live_mask"] |= 1 << j
        a = {v for v in nb if v == src or u(v, salt, fail_seed) >= thr}
        out["alive"][j] = len(a)
        seen, front, d, hops, sent, lost = {src}, [src], 0, 0, 0, 0
        while front and d < cap:
            d += 1
            nxt = []
            for x in front:
                s = chosen(x, nb[x], salt, fan, fail_seed)
                sent += len(s)
                lost += len(s - a)
                for p in sorted(s & a):
                    if p not in seen:
                        seen.add(p)
                        nxt.append(p)
            front = nxt
            if front:
                hops += d * len(front)
                out["ecc"][j] = d
        out["reached"][j] = len(seen) - 1
        out["hop_sum"][j] = hops
        out["sent"][j] = sent
        out["lost"][j] = lost
        deepest = max(deepest, int(out["ecc"][j]))
    if out["cases_live"]:
        out["ecc_max"] = deepest
        out["levels"] = min(deepest + 1, cap)
        out["truncated"] = 1 if deepest == cap else 0
    return out


def compare(got, want):
    """field for field; `got` may carry more keys than the reference"""
    bad = []
    for k in ARRAYS:
        g, x = np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)
        if not np.array_equal(g, x):
            at = int(np.flatnonzero(g != x)[0]) if g.shape == x.shape else -1
            bad.append(f"{k}[{at}]: {int(g[at])} != {int(x[at])}" if at >= 0 else k)
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append(f"{k}: {int(got[k])} != {int(want[k])}")
    assert not bad, bad
