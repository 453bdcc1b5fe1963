"""Reference for psim_resilience (test infrastructure): every field of the
struct from node rows -- _graph_metrics.rows_of() of nodes() or
strategy_nodes() -- one failure case at a time, with plain sets, a plain BFS
and Python-int arithmetic.  It calls nothing of the engine, so a test can apply
it to the CPU oracle's rows and compare the engine against it.

A case is (source, threshold, salt).  u(v, salt) =
(mix64(fail_seed ^ mix64(salt << 32 | v)) >> 32) & 0xFFFFFFFF.  A case whose
source is down is skipped: its slots stay zero.  A_j: the up nodes v with
v == source or u(v, salt) >= threshold; L_j: the links with both ends in A_j.
Levels as _graph_metrics.reference_rows runs them: level d = 1, 2, ... while
d <= cap; a level that finds no node in any case ends the BFS; `levels` counts
that empty level too; `truncated` is 1 when level `cap` still found a node."""
import numpy as np

from _graph_metrics import MAX_LEVELS, links_of

CASES = 64
M64 = (1 << 64) - 1

SCALARS = ("n_up", "links", "cases_live", "live_mask", "ecc_max", "levels", "truncated")
ARRAYS = ("alive", "links_alive", "no_out", "no_in", "reached", "hop_sum", "ecc")


# the anchors of the tests: computed with a throwaway model of the definitions
# above when the call was specified, on the oracle's rows of
# S.doubling(n=203, seed=3, rounds=30) (A) and S.pl_doubling(n=2048, seed=13,
# rounds=33, strategy=2, crash_at=30) (B, every 230th live id), fail_seed 7
SRC_A = [5, 17, 40, 77, 101, 150, 180, 202]
SRC_B = [0, 253, 513, 766, 1013, 1274, 1526, 1785]
GRID_A = {  # q: sums over k of alive, links_alive, reached, hop_sum, no_in; max ecc
    0: (1624, 6320, 1616, 7364, 0, 9), 1: (1449, 5004, 1430, 7258, 7, 12), 2: (1298, 3976, 1259, 6914, 13, 12),
    3: (1133, 3028, 1056, 6815, 24, 15), 4: (972, 2240, 732, 4629, 50, 13), 5: (794, 1476, 353, 2392, 91, 15),
    6: (640, 978, 212, 1517, 118, 19), 7: (466, 540, 45, 152, 134, 8),
}


def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def u(v, salt, fail_seed):
    return mix64((fail_seed & M64) ^ mix64((salt << 32) | v)) >> 32


def grid(sources, shares=8):
    """the report's cases: slot 8q + k = (sources[k], floor(q 2^32 / 10), salt k)"""
    return [(int(s), (q << 32) // 10, k) for q in range(shares) for k, s in enumerate(sources)]


def reference_rows(rows, cases=(), fail_seed=0, max_levels=0):
    """rows: [(up, [ids])] per node; cases: [(source, threshold, salt)]"""
    out = {k: 0 for k in SCALARS}
    for k in ARRAYS:
        out[k] = np.zeros(CASES, np.uint64)
    nb = links_of(rows)
    out["n_up"] = len(nb)
    out["links"] = sum(len(v) for v in nb.values())
    cases = [(int(s), int(t), int(x)) for s, t, x in cases]
    assert len(cases) <= CASES and all(0 <= s < len(rows) for s, _, _ in cases)
    cap = MAX_LEVELS if not max_levels or max_levels > MAX_LEVELS else int(max_levels)
    deepest = 0
    for j, (src, thr, salt) in enumerate(cases):
        if src not in nb:
            continue
        out["cases_live"] += 1
        out["live_mask"] |= 1 << j
        a = {v for v in nb if v == src or u(v, salt, fail_seed) >= thr}
        lj = {i: nb[i] & a for i in a}
        has_in = set().union(*lj.values()) if lj else set()
        out["alive"][j] = len(a)
        out["links_alive"][j] = sum(len(x) for x in lj.values())
        out["no_out"][j] = sum(1 for i in a if not lj[i])
        out["no_in"][j] = len(a - has_in)
        seen, front, d, hops = {src}, [src], 0, 0
        while front and d < cap:
            d += 1
            nxt = []
            for x in front:
                for p in lj[x]:
                    if p not in seen:
                        seen.add(p)
                        nxt.append(p)
            front = nxt
            if front:
                hops += d * len(front)
                out["ecc"][j] = d
        out["reached"][j] = len(seen) - 1
        out["hop_sum"][j] = hops
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
        g, w = np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0]) if g.shape == w.shape else -1
            bad.append(f"{k}[{at}]: {int(g[at])} != {int(w[at])}" if at >= 0 else k)
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append(f"{k}: {int(got[k])} != {int(want[k])}")
    assert not bad, bad
