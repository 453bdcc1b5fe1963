"""Reference for psim_tree_metrics (test infrastructure): every field of the
struct from psim_node_view rows (pt_root, pt_eager_n, pt_lazy_n, pt_eager,
pt_lazy, pt_common, act, up) with Python sets, a plain BFS and Python-int
arithmetic.  It calls nothing of the engine, so a test can apply it to the CPU
oracle's rows and compare the engine against it.

Definitions (include/partisan_gpu_sim.h, psim_tree_metrics): a live node i
answers for root R with the runs of its first slot whose root is R | MAP_BIT,
else with (pt_common, []).  An entry e names p = e & ~MAP_BIT; p is live if
p < n and up[p].  E_i / Z_i: the distinct live p != i over the eager / lazy
entries.  T = {(i, p): p in E_i}.  L: the active view, p != i, p live.  Levels:
a BFS runs level d = 1, 2, ... while d <= cap; a level that finds no node ends
it.  `levels` counts the levels the BFS over T ran, that empty one included;
`truncated` is 1 when level `cap` of either BFS still found a node."""
import numpy as np

HIST_BINS = 64
MAX_LEVELS = 4096
MAP_BIT = 0x80000000
ROOTS = 4

SCALARS = ("n_up", "root_live", "slot_nodes", "eager_entries", "lazy_entries", "eager_links", "lazy_links",
           "both_links", "eager_both_forms", "self_entries", "eager_dead", "lazy_dead", "eager_nonmember",
           "lazy_nonmember", "eager_symmetric", "depth_sum", "depth_max", "reached", "unreached",
           "links_from_reached", "levels", "truncated", "overlay_reached", "both_reached", "depth_sum_both",
           "dist_sum_both", "deeper", "shallower")
ARRAYS = ("eager_out", "lazy_out", "eager_in", "depth")
# the fields that do not depend on whether the root is live
DEGREE_FIELDS = ("n_up", "eager_links", "eager_symmetric", "eager_out", "eager_in")


def node(up=True, act=(), common=(), slots=()):
    """one hand-built row: slots = [(root, [eager entries], [lazy entries])],
    the root without its MAP_BIT (it is added here, as the engine stores it)"""
    return dict(up=up, act=list(act), common=list(common), slots=[(r | MAP_BIT, list(e), list(z)) for r, e, z in slots])


def rows_of(views):
    """psim_node_view rows -> the dicts of node()"""
    out = []
    for i in range(len(views)):
        v = views[i]
        en, ln = [int(x) for x in v["pt_eager_n"]], [int(x) for x in v["pt_lazy_n"]]
        eag, laz = [int(x) for x in v["pt_eager"]], [int(x) for x in v["pt_lazy"]]
        slots = []
        for k in range(ROOTS):
            eo, zo = sum(en[:k]), sum(ln[:k])
            slots.append((int(v["pt_root"][k]), eag[eo: eo + en[k]], laz[zo: zo + ln[k]]))
        out.append(dict(up=bool(v["up"]), act=[int(x) for x in v["act"][: int(v["act_n"])]],
                        common=[int(x) for x in v["pt_common"][: int(v["pt_common_n"])]], slots=slots))
    return out


def sets_of(row, root):
    """(eager entries, lazy entries, holds a slot) of a node for `root`: all_peers/3"""
    for r, e, z in row["slots"]:
        if r == (root | MAP_BIT):
            return e, z, True
    return row["common"], [], False


def _bfs(nb, root, cap):
    """{v: depth}, the deepest level that found a node"""
    depth, front, d = {root: 0}, [root], 0
    while front and d < cap:
        d += 1
        nxt = []
        for x in front:
            for p in nb[x]:
                if p not in depth:
                    depth[p] = d
                    nxt.append(p)
        front = nxt
    return depth, max(depth.values())


def _zero():
    out = {k: 0 for k in SCALARS}
    for k in ARRAYS:
        out[k] = np.zeros(HIST_BINS, np.uint64)
    return out


def reference_rows(rows, root, max_levels=0):
    n = len(rows)
    assert 0 <= root < n
    out = _zero()
    live = {i for i, r in enumerate(rows) if r["up"]}
    E, Z = {}, {}
    for i in sorted(live):
        eag, laz, slot = sets_of(rows[i], root)
        act = set(rows[i]["act"])
        out["slot_nodes"] += 1 if slot else 0
        out["eager_entries"] += len(eag)
        out["lazy_entries"] += len(laz)
        for entries, dead in ((eag, "eager_dead"), (laz, "lazy_dead")):
            for e in entries:
                p = e & ~MAP_BIT
                if p == i:
                    out["self_entries"] += 1
                elif p not in live:
                    out[dead] += 1
        E[i] = {e & ~MAP_BIT for e in eag if e & ~MAP_BIT != i and e & ~MAP_BIT in live}
        Z[i] = {e & ~MAP_BIT for e in laz if e & ~MAP_BIT != i and e & ~MAP_BIT in live}
        out["both_links"] += len(E[i] & Z[i])
        out["eager_both_forms"] += sum(1 for p in E[i] if p in eag and (p | MAP_BIT) in eag)
        out["eager_nonmember"] += len(E[i] - act)
        out["lazy_nonmember"] += len(Z[i] - act)
        out["eager_out"][min(len(E[i]), HIST_BINS - 1)] += 1
        out["lazy_out"][min(len(Z[i]), HIST_BINS - 1)] += 1
    out["n_up"] = len(live)
    out["eager_links"] = sum(len(v) for v in E.values())
    out["lazy_links"] = sum(len(v) for v in Z.values())
    indeg = {i: 0 for i in live}
    for i, ps in E.items():
        for p in ps:
            indeg[p] += 1
            out["eager_symmetric"] += 1 if i in E[p] else 0
    for i in live:
        out["eager_in"][min(indeg[i], HIST_BINS - 1)] += 1
    out["root_live"] = 1 if root in live else 0
    if root not in live:
        return out
    cap = MAX_LEVELS if not max_levels or max_levels > MAX_LEVELS else int(max_levels)
    L = {i: {p for p in rows[i]["act"] if p != i and p in live} for i in live}
    dt, deep_t = _bfs(E, root, cap)
    dl, deep_l = _bfs(L, root, cap)
    for v, d in dt.items():
        out["links_from_reached"] += len(E[v])
        if v == root:
            continue
        out["depth"][min(d, HIST_BINS - 1)] += 1
        out["depth_sum"] += d
        out["reached"] += 1
        if v in dl:
            out["both_reached"] += 1
            out["depth_sum_both"] += d
            out["dist_sum_both"] += dl[v]
            out["deeper"] += 1 if d > dl[v] else 0
            out["shallower"] += 1 if d < dl[v] else 0
    out["depth_max"] = deep_t
    out["overlay_reached"] = len(dl) - 1
    out["unreached"] = len(live) - 1 - out["reached"]
    out["levels"] = min(deep_t + 1, cap)
    out["truncated"] = 1 if cap in (deep_t, deep_l) else 0
    return out


def reference(views, root, max_levels=0):
    """views: nodes() of every node of a HyParView / X-BOT handle"""
    return reference_rows(rows_of(views), root, max_levels)


def compare(got, want):
    """field for field, the first differing field named first; `got` may
    carry more keys than the reference"""
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
