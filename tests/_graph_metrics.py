"""Reference for psim_graph_metrics (test infrastructure): every field of the
struct from node rows -- nodes() of a HyParView / X-BOT handle (kind "hv") or
strategy_nodes() of a SCAMP handle (kind "scamp") -- with a set per row, a
plain BFS per source and Python-int arithmetic.  It calls nothing of the
engine's statistics, so a test can apply it to the CPU oracle's rows and
compare the engine against it.

The link set L: ordered pairs (i, p), i live, p in i's row, p != i, p live, a
repeated id counted once.  N(i) = the out-neighbours of i, k_i = |N(i)|.
Levels: the BFS runs level d = 1, 2, ... while d <= cap; a level that finds no
new (source, node) pair ends it.  `levels` counts the levels run, that empty
one included; `truncated` is 1 when level `cap` still found a pair."""
import numpy as np

HIST_BINS = 64
SOURCES = 64
MAX_LEVELS = 4096

SCALARS = ("n_up", "links", "cl_nodes", "cl_closed", "cl_pairs", "cl_sum_q32", "sources_live", "dist_sum",
           "pairs_reached", "pairs_unreached", "ecc_max", "levels", "truncated")
ARRAYS = ("dist", "reach", "ecc")
PATH_SUMS = ("sources_live", "dist", "dist_sum", "pairs_reached", "pairs_unreached")


def rows_of(views, kind):
    """(up, row) per node: the raw id list of its active view / SCAMP view"""
    col, cnt = ("act", "act_n") if kind == "hv" else ("view", "view_n")
    return [(bool(views["up"][i]), [int(x) for x in views[col][i][: int(views[cnt][i])]])
            for i in range(len(views))]


def links_of(rows):
    """{live i: N(i)}"""
    up = {i for i, (u, _) in enumerate(rows) if u}
    return {i: (set(rows[i][1]) - {i}) & up for i in sorted(up)}


def _zero():
    out = {k: 0 for k in SCALARS}
    out["dist"] = np.zeros(HIST_BINS, np.uint64)
    out["reach"] = np.zeros(SOURCES, np.uint64)
    out["ecc"] = np.zeros(SOURCES, np.uint64)
    return out


def reference_rows(rows, sources=(), max_levels=0):
    """rows: [(up, [ids])] per node"""
    out = _zero()
    nb = links_of(rows)
    out["n_up"] = len(nb)
    out["links"] = sum(len(v) for v in nb.values())
    for i, ni in nb.items():
        k = len(ni)
        if k < 2:
            continue
        closed = sum(len(nb[a] & ni) for a in ni)       # (a not in N(a): every b counted differs from a)
        out["cl_nodes"] += 1
        out["cl_closed"] += closed
        out["cl_pairs"] += k * (k - 1)
        out["cl_sum_q32"] += (closed << 32) // (k * (k - 1))
    sources = [int(s) for s in sources]
    assert len(sources) <= SOURCES and len(set(sources)) == len(sources)
    assert all(0 <= s < len(rows) for s in sources)
    cap = MAX_LEVELS if not max_levels or max_levels > MAX_LEVELS else int(max_levels)
    live = [(j, s) for j, s in enumerate(sources) if s in nb]
    out["sources_live"] = len(live)
    if not live:
        return out
    per_level = {}                                  # d -> pairs first reached at distance d
    for j, s in live:
        seen, front, d = {s}, [s], 0
        while front and d < cap:
            d += 1
            nxt = []
            for x in front:
                for p in nb[x]:
                    if p not in seen:
                        seen.add(p)
                        nxt.append(p)
            front = nxt
            if front:
                per_level[d] = per_level.get(d, 0) + len(front)
                out["ecc"][j] = d
        out["reach"][j] = len(seen) - 1
    deepest = max(per_level) if per_level else 0
    for d, c in per_level.items():
        out["dist"][min(d, HIST_BINS - 1)] += c
        out["dist_sum"] += d * c
        out["pairs_reached"] += c
    out["ecc_max"] = deepest
    out["levels"] = min(deepest + 1, cap)
    out["truncated"] = 1 if deepest == cap else 0
    out["pairs_unreached"] = len(live) * (out["n_up"] - 1) - out["pairs_reached"]
    return out


def reference(rows, kind, sources=(), max_levels=0):
    """rows: nodes() (kind "hv") or strategy_nodes() (kind "scamp") of every node"""
    return reference_rows(rows_of(rows, kind), sources, max_levels)


def reference_all(rows, kind, max_levels=0):
    """every id a source, in batches of 64, summed as Simulator.graph_metrics_all() sums them"""
    rr = rows_of(rows, kind)
    n = len(rr)
    out = None
    reach, ecc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for lo in range(0, n, SOURCES):
        ids = list(range(lo, min(n, lo + SOURCES)))
        m = reference_rows(rr, ids, max_levels)
        reach[ids], ecc[ids] = m["reach"][: len(ids)], m["ecc"][: len(ids)]
        if out is None:
            out = m
            continue
        for f in PATH_SUMS:
            out[f] = out[f] + m[f]
        for f in ("ecc_max", "levels", "truncated"):
            out[f] = max(out[f], m[f])
    if out is None:
        out = reference_rows(rr)
    out["reach"], out["ecc"] = reach, ecc
    return out


def compare(got, want):
    """field for field; `got` may carry more keys than the reference"""
    bad = []
    for k in ARRAYS:
        if not np.array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)):
            bad.append(k)
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append(f"{k}: {int(got[k])} != {int(want[k])}")
    assert not bad, bad
