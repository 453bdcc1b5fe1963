"""Reference for psim_strategy_histograms (test infrastructure): every field
of the struct from a strategy_nodes() array -- plus the member_bits rows of a
full-membership handle -- with a set per row and a union-find.  Plain numpy /
Python; it calls nothing of the engine's overlay statistics, so a test can
apply it to the CPU oracle's views and compare the engine against it."""
import numpy as np

HIST_BINS = 64
STRATEGY_FULL, STRATEGY_SCAMP_V1, STRATEGY_SCAMP_V2 = 0, 1, 2

HISTS = ("view_fill", "in_fill", "out_degree", "in_degree")
SCALARS = ("n_up", "view_sum", "in_sum", "view_max", "in_degree_max", "links", "mutual_links",
           "dangling_links", "self_entries", "duplicate_entries", "in_view_links", "in_view_confirmed",
           "components", "largest_component", "isolated", "members_min", "members_max", "members_sum",
           "agreeing")


def _zero():
    out = {k: np.zeros(HIST_BINS, np.uint64) for k in HISTS}
    out.update({k: 0 for k in SCALARS})
    return out


def _bump(hist, v):
    hist[min(int(v), HIST_BINS - 1)] += 1


def reference(views, strategy, member_bits=None):
    """views: strategy_nodes() of every node; strategy: cfg.strategy;
    member_bits: full strategy only, one bitset row (uint32 words) per node."""
    out = _zero()
    n = len(views)
    live = [i for i in range(n) if views["up"][i]]
    out["n_up"] = len(live)
    if strategy == STRATEGY_FULL:
        if live:
            rows = [np.asarray(member_bits[i], np.uint32) for i in live]
            sizes = [int(np.unpackbits(r.view(np.uint8)).sum()) for r in rows]
            out["members_min"], out["members_max"], out["members_sum"] = min(sizes), max(sizes), sum(sizes)
            out["agreeing"] = sum(1 for r in rows if np.array_equal(r, rows[0]))
        return out

    up = set(live)
    v2 = strategy == STRATEGY_SCAMP_V2
    link = {}                       # live i -> its distinct live targets != i
    for i in live:
        vn = int(views["view_n"][i])
        row = [int(x) for x in views["view"][i][:vn]]
        ids = set(row)
        others = ids - {i}
        link[i] = others & up
        _bump(out["view_fill"], vn)
        _bump(out["out_degree"], len(others))
        out["view_sum"] += vn
        out["view_max"] = max(out["view_max"], vn)
        out["dangling_links"] += len(others - up)
        out["self_entries"] += 1 if i in ids else 0
        out["duplicate_entries"] += vn - len(ids)
        if v2:
            _bump(out["in_fill"], int(views["in_n"][i]))
            out["in_sum"] += int(views["in_n"][i])
    indeg = {i: 0 for i in live}
    for i in live:
        for p in link[i]:
            indeg[p] += 1
            out["links"] += 1
            out["mutual_links"] += 1 if i in link[p] else 0
    for i in live:
        _bump(out["in_degree"], indeg[i])
        out["in_degree_max"] = max(out["in_degree_max"], indeg[i])
        out["isolated"] += 1 if not link[i] and not indeg[i] else 0
    if v2:
        for i in live:
            inn = int(views["in_n"][i])
            for j in (set(int(x) for x in views["in_view"][i][:inn]) - {i}) & up:
                out["in_view_links"] += 1
                out["in_view_confirmed"] += 1 if i in link[j] else 0

    parent = {i: i for i in live}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in live:
        for p in link[i]:
            a, b = find(i), find(p)
            if a != b:
                parent[max(a, b)] = min(a, b)
    sizes = {}
    for i in live:
        r = find(i)
        sizes[r] = sizes.get(r, 0) + 1
    out["components"] = len(sizes)
    out["largest_component"] = max(sizes.values()) if sizes else 0
    return out


def compare(got, want):
    """field for field; `got` may carry more keys than the reference"""
    bad = []
    for k in HISTS:
        if not np.array_equal(np.asarray(got[k], np.uint64), want[k]):
            bad.append(k)
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append(f"{k}: {int(got[k])} != {int(want[k])}")
    assert not bad, bad
