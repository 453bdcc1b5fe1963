"""CPU checks of psim_get_latency_metrics' boundary: the struct layout of the
ctypes mirror against the header, where the entry point is declared, and the
reference (tests/_latency.py, the yardstick of tests/test_gpu_latency.py) on
rows whose numbers are worked out by hand below and on the oracle's rows --
three algorithms against each other, and anchors computed when the call was
specified."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _latency as P
import _scenarios as S
from _oracle import Oracle
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
SEED = 3
# the torus cells (x, y) of the ids the hand-built rows use, under SEED
CELLS = {0: (240, 266), 1: (193, 151), 2: (713, 416), 3: (925, 888), 4: (463, 754), 5: (441, 109),
         523: (516, 805), 541: (516, 805)}


def test_struct_layout_matches_header(tmp_path):
    m = _abi.PsimLatencyMetrics
    names = [n for n, _ in m._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%d %%d\\n", sizeof(psim_latency_metrics), PSIM_LAT_SOURCES, PSIM_HIST_BINS);\n'
        '%s return 0;}\n'
        % (HDR, "".join('printf("%%zu\\n", offsetof(psim_latency_metrics, %s));\n' % n for n in names)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [C.sizeof(m), _abi.LAT_SOURCES, _abi.HIST_BINS] and got[1:3] == [P.SOURCES, P.HIST_BINS]
    assert got[3:] == [getattr(m, n).offset for n in names]
    assert names[-1] == "reserved"
    assert sorted(n for n in names if n != "reserved") == sorted(P.SCALARS + P.ARRAYS)
    assert all(t in (C.c_uint64, C.c_uint64 * 64, C.c_uint64 * 8) for _, t in m._fields_)
    assert C.sizeof(m) == 8 * (len(P.SCALARS) + 64 * len(P.ARRAYS) + 8)


def test_entry_point_is_gpu_only():
    assert "get_latency_metrics" in _abi.GPU_ONLY
    assert "get_latency_metrics" not in _abi.SIGNATURES
    hdr = open(HDR).read()
    assert re.search(r"\bpsim_get_latency_metrics\s*\(", hdr)
    assert re.search(r"#define\s+PSIM_LAT_SOURCES\s+64\b", hdr)
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", hdr)
    res, args = _abi.GPU_ONLY["get_latency_metrics"]
    assert res is C.c_int and len(args) == 6 and args[3] is C.c_uint32 and args[4] is C.c_uint32


# ---- the latency oracle restated
def test_latency_is_the_torus_distance_of_the_cells():
    for i, (x, y) in CELLS.items():
        assert (P.cell(SEED, i) & 1023, P.cell(SEED, i) >> 10) == (x, y)
    # |240 - 193| + |266 - 151|; 713 - 193 = 520 wraps to 504, + 265
    assert P.latency(SEED, 0, 1) == 47 + 115 == 162 and P.latency(SEED, 1, 2) == 504 + 265 == 769
    assert P.latency(SEED, 5, 5) == 0 and P.latency(SEED, 2, 1) == 769
    assert max(P.latency(SEED, 0, p) for p in range(1, 3000)) <= 1024


def test_latency_is_the_librarys():
    """the restatement agrees with the oracle library's orc_xbot_latency, the
    twin of psim_xbot_latency, on seeded triples"""
    import _oracle
    fn = _oracle.load().orc_xbot_latency
    fn.restype, fn.argtypes = C.c_uint32, [C.c_uint64, C.c_uint32, C.c_uint32]
    rng = np.random.Generator(np.random.PCG64(11))
    for _ in range(500):
        seed, a, b = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 27)), int(rng.integers(0, 1 << 27))
        assert fn(seed, a, b) == P.latency(seed, a, b)
    assert fn(SEED, 523, 541) == 0 and fn(SEED, 0, 1) == 162


# ---- hand-built rows
def _rows(n, links):
    rows = [(True, []) for _ in range(n)]
    for i, ps in links.items():
        rows[i] = (True, list(ps))
    return rows


def _slot(m, j=0):
    return tuple(int(m[k][j]) for k in P.SLOTS)


def test_line_of_five():
    """0 - 1 - 2 - 3 - 4, links both ways, source 0.  w(0,1) = 162, w(1,2) =
    769, w(2,3) = 212 + 472 = 684, w(3,4) = 462 + 134 = 596: D = 162, 931, 1615,
    2211, one more node a sweep; sweep 5 finds nothing."""
    nb = P.links_rows(_rows(5, {0: [1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3]}))
    m = P.reference_links(nb, SEED, [0])
    assert _slot(m) == (4, 162 + 931 + 1615 + 2211, 2211, 4) and m["sweeps"] == 5 and m["truncated_mask"] == 0
    assert (m["n_up"], m["links"], m["link_cost_sum"]) == (5, 8, 2 * (162 + 769 + 684 + 596))
    assert (m["link_nodes"], m["worst_sum"], m["best_sum"]) == (5, 162 + 769 + 769 + 684 + 596, 162 + 162 + 684 + 596 + 596)
    assert {i: int(v) for i, v in enumerate(m["link_cost"]) if v} == {162 >> 4: 2, 769 >> 4: 2, 684 >> 4: 2, 596 >> 4: 2}
    assert {i: int(v) for i, v in enumerate(m["lat"]) if v} == {0: 1, 3: 1, 6: 1, 8: 1}
    assert (m["pairs_reached"], m["pairs_unreached"], m["lat_sum_all"], m["lat_max"]) == (4, 0, 4919, 2211)
    # a cap of 2: D_2, and sweep 2 still lowered a distance
    m = P.reference_links(nb, SEED, [0], 2)
    assert _slot(m) == (2, 162 + 931, 931, 2) and m["sweeps"] == 2 and m["truncated_mask"] == 1
    assert m["pairs_unreached"] == 2
    # two sources, the second in slot 1; a cap past the end equals none
    m = P.reference_links(nb, SEED, [0, 4], 99)
    assert _slot(m, 1) == (4, 596 + 1280 + 2049 + 2211, 2211, 4) and m["live_mask"] == 3 and m["sweeps"] == 5
    for k in P.SCALARS + P.ARRAYS:
        assert np.array_equal(m[k], P.reference_links(nb, SEED, [0, 4])[k]), k


def test_diamond_cheaper_path_has_more_links():
    """0 -> 3 -> 4 costs 741 + 596 = 1337; 0 -> 1 -> 5 -> 4 costs 162 + 290 +
    401 = 853.  D_1(4) is infinite, D_2(4) = 1337, D_3(4) = 853: every cap
    shows another struct."""
    nb = P.links_rows(_rows(6, {0: [3, 1], 3: [4], 1: [5], 5: [4]}))
    w = lambda a, b: P.latency(SEED, a, b)                              # noqa: E731
    assert (w(0, 3), w(3, 4), w(0, 1), w(1, 5), w(5, 4)) == (741, 596, 162, 290, 401)
    m1, m2, m3, m = (P.reference_links(nb, SEED, [0], cap) for cap in (1, 2, 3, 0))
    assert _slot(m1) == (2, 741 + 162, 741, 1) and m1["pairs_unreached"] == 3 and m1["truncated_mask"] == 1
    assert _slot(m2) == (4, 741 + 162 + 452 + 1337, 1337, 2) and m2["truncated_mask"] == 1 and m2["sweeps"] == 2
    assert _slot(m3) == (4, 741 + 162 + 452 + 853, 853, 3) and m3["truncated_mask"] == 1 and m3["sweeps"] == 3
    assert _slot(m) == _slot(m3) and m["truncated_mask"] == 0 and m["sweeps"] == 4
    assert m["pairs_unreached"] == 1                                    # (node 2 has no link)
    # Dijkstra and the uncapped Bellman-Ford agree on distances and on the last sweep
    d, hops = P.dijkstra(nb, w, 0)
    assert (d, max(hops.values())) == P.bellman_ford(nb, w, 0, P.MAX_SWEEPS) and hops[4] == 3


def test_zero_weight_link_ends_the_sweeps():
    """523 and 541 are the first two ids under SEED that hash to one torus cell
    (found by the search below): w = 0 both ways.  0 -> 523 <-> 541: sweep 1
    gives 523 its 761, sweep 2 gives 541 the same 761, sweep 3 offers 523 its
    own 761 again -- not strictly lower, so it is the last."""
    seen, pair = {}, None
    for i in range(5000):
        c = P.cell(SEED, i)
        if c in seen:
            pair = (seen[c], i)
            break
        seen[c] = i
    assert pair == (523, 541) and P.latency(SEED, 523, 541) == 0 and P.latency(SEED, 0, 523) == 761
    nb = P.links_rows(_rows(542, {0: [523], 523: [541], 541: [523]}))
    for cap in (0, 50):
        m = P.reference_links(nb, SEED, [0], cap)
        assert _slot(m) == (2, 761 + 761, 761, 2) and m["sweeps"] == 3 and m["truncated_mask"] == 0
    assert m["link_cost"][0] == 2 and m["best_sum"] == 761 and m["worst_sum"] == 761
    # from 523 the other end is reached at latency 0, and counts as reached
    m = P.reference_links(nb, SEED, [523])
    assert _slot(m) == (1, 0, 0, 1) and m["lat"][0] == 1 and m["sweeps"] == 2


def test_dead_nodes_and_repeats():
    rows = _rows(5, {0: [1, 1, 0, 2], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3]})
    rows[2] = (False, [1, 3])
    m = P.reference_links(P.links_rows(rows), SEED, [2, 0, 4])
    assert (m["n_up"], m["links"], m["sources_live"], m["live_mask"]) == (4, 4, 2, 0b110)
    assert _slot(m, 0) == (0, 0, 0, 0) and _slot(m, 1) == (1, 162, 162, 1) and _slot(m, 2) == (1, 596, 596, 1)
    assert m["pairs_unreached"] == 2 * 3 - 2 and m["sweeps"] == 2
    m = P.reference_links(P.links_rows(rows), SEED, [2])
    assert m["sources_live"] == 0 and m["sweeps"] == 0 and not m["reach"].any()


def test_tree_half_by_hand():
    """L: 0 <-> 1 <-> 5 <-> 4, 0 <-> 3 <-> 4; T from root 0: 0 -> 3 -> 4 and
    0 -> 1.  Over T node 4 costs 1337, over L 853: slower; 5 is off the tree."""
    L = P.links_rows(_rows(6, {0: [1, 3], 1: [0, 5], 5: [1, 4], 4: [5, 3], 3: [0, 4]}))
    T = P.links_rows(_rows(6, {0: [3, 1], 3: [4]}))
    m = P.reference_links(L, SEED, [], 0, T, 0)
    assert {k: m[k] for k in P.TREE} == dict(
        tree_root_live=1, tree_links=3, tree_link_cost_sum=741 + 162 + 596, tree_reached=3,
        tree_lat_sum=741 + 162 + 1337, tree_lat_max=1337, tree_sweeps=3, overlay_reached=4, both_reached=3,
        tree_lat_sum_both=741 + 162 + 1337, overlay_lat_sum_both=741 + 162 + 853, slower=1, faster=0, tree_truncated=0)
    assert m["sources_live"] == 0 and m["sweeps"] == 0
    # a tree link that is no overlay link: the tree is faster there
    T2 = P.links_rows(_rows(6, {0: [5]}))
    m = P.reference_links(L, SEED, [], 0, T2, 0)
    assert (m["tree_reached"], m["faster"], m["slower"]) == (1, 1, 0)
    assert (m["tree_lat_sum_both"], m["overlay_lat_sum_both"]) == (P.latency(SEED, 0, 5), 452) and m["tree_lat_sum_both"] == 358
    # the cap holds for both passes: the overlay pass still lowers node 4 in sweep 3
    m = P.reference_links(L, SEED, [], 3, T, 0)
    assert m["tree_truncated"] == 1 and m["tree_sweeps"] == 3
    # a dead root
    rows = _rows(6, {0: [1, 3]})
    rows[0] = (False, [1, 3])
    m = P.reference_links(P.links_rows(rows), SEED, [], 0, {}, 0)
    assert not any(m[k] for k in P.TREE)


# ---- the oracle's rows
_VIEWS = {}


def _views():
    if "a" not in _VIEWS:
        o = S.doubling(Oracle, n=203, seed=3, rounds=30)[0]
        _VIEWS["a"] = o.nodes()
        o.close()
    return _VIEWS["a"]


def test_three_algorithms_agree_on_the_oracles_rows():
    """Dijkstra == uncapped Bellman-Ford == Floyd-Warshall, all pairs of doubling(203)"""
    nb = P.links_hv(_views())
    w = lambda a, b: P.latency(SEED, a, b)                              # noqa: E731
    fw = P.floyd_warshall(nb, w)
    for s in sorted(nb):
        d, hops = P.dijkstra(nb, w, s)
        assert (d, max(hops.values())) == P.bellman_ford(nb, w, s, P.MAX_SWEEPS)
        assert d == {v: c for (a, v), c in fw.items() if a == s}


ANCHORS = {0: (202, 513205, 3642, 10), 5: (202, 394997, 3103, 9), 202: (202, 452314, 3521, 11)}


def test_anchors_of_doubling_203():
    nb = P.links_hv(_views())
    m = P.reference(_views(), SEED, list(ANCHORS))
    assert (m["n_up"], m["links"], m["link_cost_sum"], m["link_nodes"]) == (203, 790, 407750, 203)
    assert min(P.latency(SEED, i, p) for i in nb for p in nb[i]) > 0 and m["link_cost"][0] == 0
    assert int(m["link_cost"].sum()) == 790
    for j, s in enumerate(ANCHORS):
        assert _slot(m, j) == ANCHORS[s], s
    assert m["sweeps"] == 12 and m["truncated_mask"] == 0 and m["pairs_unreached"] == 0
    assert int(m["lat"].sum()) == m["pairs_reached"] == 606
    # capped at 4 every slot is truncated and short of its uncapped reach
    m4 = P.reference(_views(), SEED, list(ANCHORS), 4)
    assert m4["truncated_mask"] == 0b111 and m4["sweeps"] == 4 and (m4["reach"][:3] < 202).all()
    assert [int(x) for x in m4["last_sweep"][:3]] == [4, 4, 4]
