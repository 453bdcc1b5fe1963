"""CPU checks of psim_get_graph_metrics' boundary: the struct layout of the
ctypes mirror against the header, where the entry point is declared, the NIF
table, and the reference (tests/_graph_metrics.py, the yardstick of
tests/test_gpu_graph_metrics.py) on graphs whose numbers are worked out by
hand below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _graph_metrics as R
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
NIF = os.path.join(ROOT, "erlang", "c_src", "partisan_gpu_sim_nif.c")


def test_struct_layout_matches_header(tmp_path):
    m = _abi.PsimGraphMetrics
    names = [n for n, _ in m._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%d %%d\\n", sizeof(psim_graph_metrics), PSIM_GRAPH_SOURCES, PSIM_GRAPH_MAX_LEVELS);\n'
        '%s return 0;}\n'
        % (HDR, "".join('printf("%%zu\\n", offsetof(psim_graph_metrics, %s));\n' % n for n in names)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [C.sizeof(m), _abi.GRAPH_SOURCES, _abi.GRAPH_MAX_LEVELS]
    assert got[3:] == [getattr(m, n).offset for n in names]
    assert (R.SOURCES, R.MAX_LEVELS, R.HIST_BINS) == (_abi.GRAPH_SOURCES, _abi.GRAPH_MAX_LEVELS, _abi.HIST_BINS)
    assert sorted(n for n in names if n != "reserved") == sorted(R.SCALARS + R.ARRAYS)
    assert m.ecc.size == 4 * 64 and m.reserved.size == 8 * 8


def test_entry_point_is_gpu_only():
    assert "get_graph_metrics" in _abi.GPU_ONLY
    assert "get_graph_metrics" not in _abi.SIGNATURES
    assert re.search(r"\bpsim_get_graph_metrics\s*\(", open(HDR).read())
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", open(HDR).read())


def test_nif_table_and_erlang_stub():
    table = {(n, int(a)): f for n, a, f in re.findall(r'\{"(\w+)",\s*(\d+),\s*nif_\w+,\s*(\w+)\}', open(NIF).read())}
    assert table.get(("graph_metrics_nif", 3)) == "ERL_NIF_DIRTY_JOB_CPU_BOUND"
    erl = open(os.path.join(ROOT, "erlang", "src", "partisan_gpu_sim.erl")).read()
    assert re.search(r"^graph_metrics_nif\(_Sim, _Sources, _MaxLevels\)\s*->\s*erlang:nif_error", erl, re.M)
    assert re.search(r"^graph_metrics\(Sim, Sources, MaxLevels\)\s*->", erl, re.M)
    assert "graph_metrics/3" in erl


def _arr(pairs, n=64):
    h = np.zeros(n, np.uint64)
    for k, c in pairs:
        h[k] = c
    return h


def _up(rows):
    return [(True, r) for r in rows]


CYCLE = _up([[1], [2], [3], [4], [0]])         # 0 -> 1 -> 2 -> 3 -> 4 -> 0


def test_directed_cycle():
    """every source reaches the other four at distances 1, 2, 3, 4; no node
    has two neighbours"""
    got = R.reference_rows(CYCLE, sources=[0, 1, 2, 3, 4])
    want = dict(n_up=5, links=5, cl_nodes=0, cl_closed=0, cl_pairs=0, cl_sum_q32=0, sources_live=5,
                dist=_arr([(1, 5), (2, 5), (3, 5), (4, 5)]), dist_sum=5 * 10, pairs_reached=20, pairs_unreached=0,
                reach=_arr([(j, 4) for j in range(5)]), ecc=_arr([(j, 4) for j in range(5)]), ecc_max=4,
                levels=5,                  # levels 1..4 find a pair each, level 5 finds none
                truncated=0)
    R.compare(got, want)


def test_cycle_truncated_at_two_levels():
    got = R.reference_rows(CYCLE, sources=[0, 3], max_levels=2)
    want = dict(n_up=5, links=5, cl_nodes=0, cl_closed=0, cl_pairs=0, cl_sum_q32=0, sources_live=2,
                dist=_arr([(1, 2), (2, 2)]), dist_sum=6, pairs_reached=4,
                pairs_unreached=2 * 4 - 4,          # distances 3 and 4 lie past the cap
                reach=_arr([(0, 2), (1, 2)]), ecc=_arr([(0, 2), (1, 2)]), ecc_max=2, levels=2, truncated=1)
    R.compare(got, want)
    # a cap the BFS never meets: as without one; a cap past the largest: clamped
    R.compare(R.reference_rows(CYCLE, [0, 3], 5), R.reference_rows(CYCLE, [0, 3]))
    R.compare(R.reference_rows(CYCLE, [0, 3], 10**6), R.reference_rows(CYCLE, [0, 3]))


def test_k4():
    """every ordered pair is a link: each node's 3 * 2 neighbour pairs are all closed"""
    rows = _up([[j for j in range(4) if j != i] for i in range(4)])
    got = R.reference_rows(rows, sources=[2, 0])
    want = dict(n_up=4, links=12, cl_nodes=4, cl_closed=24, cl_pairs=24, cl_sum_q32=4 << 32, sources_live=2,
                dist=_arr([(1, 6)]), dist_sum=6, pairs_reached=6, pairs_unreached=0,
                reach=_arr([(0, 3), (1, 3)]), ecc=_arr([(0, 1), (1, 1)]), ecc_max=1, levels=2, truncated=0)
    R.compare(got, want)


def test_two_disjoint_triangles():
    """{0, 1, 2} and {3, 4, 5}, each a directed 3-cycle plus one chord (0 -> 2):
    node 0 has N = {1, 2} and 1 -> 2 is a link, 2 -> 1 is not"""
    rows = _up([[1, 2], [2], [0], [4], [5], [3]])
    got = R.reference_rows(rows, sources=[0, 4])
    want = dict(n_up=6, links=7, cl_nodes=1, cl_closed=1, cl_pairs=2, cl_sum_q32=1 << 31, sources_live=2,
                dist=_arr([(1, 3), (2, 1)]),        # 0: 1, 2 at 1;  4: 5 at 1, 3 at 2
                dist_sum=5, pairs_reached=4, pairs_unreached=2 * 5 - 4,
                reach=_arr([(0, 2), (1, 2)]), ecc=_arr([(0, 1), (1, 2)]), ecc_max=2, levels=3, truncated=0)
    R.compare(got, want)


def test_repeat_self_and_dead_entries():
    """node 0's row holds 1 twice, itself, and the dead node 3: N(0) = {1, 2};
    the dead node's own row counts for nothing, and as a source it is skipped"""
    rows = [(True, [1, 1, 0, 3, 2]), (True, [2, 3]), (True, [0]), (False, [0, 1, 2])]
    got = R.reference_rows(rows, sources=[3, 0, 1])
    want = dict(n_up=3, links=4,                    # 0->1, 0->2, 1->2, 2->0
                cl_nodes=1, cl_closed=1, cl_pairs=2, cl_sum_q32=1 << 31, sources_live=2,
                dist=_arr([(1, 3), (2, 1)]),        # 0: 1, 2 at 1;  1: 2 at 1, 0 at 2
                dist_sum=5, pairs_reached=4, pairs_unreached=0,
                reach=_arr([(1, 2), (2, 2)]), ecc=_arr([(1, 1), (2, 2)]), ecc_max=2, levels=3, truncated=0)
    R.compare(got, want)


def test_no_sources_and_fixed_point_floor():
    """without sources only the clustering half is filled; the per-node
    quotient is floored: N(0) = {1, 2, 3} with the one closed pair (1, 2)"""
    rows = _up([[1, 2, 3], [2], [], []])
    got = R.reference_rows(rows)
    want = dict(n_up=4, links=4, cl_nodes=1, cl_closed=1, cl_pairs=6, cl_sum_q32=(1 << 32) // 6, sources_live=0,
                dist=_arr([]), dist_sum=0, pairs_reached=0, pairs_unreached=0, reach=_arr([]), ecc=_arr([]),
                ecc_max=0, levels=0, truncated=0)
    R.compare(got, want)
    assert got["cl_sum_q32"] == 715827882


def _hv_views(rows):
    v = np.zeros(len(rows), _abi.NODE_VIEW_DTYPE)
    for i, (up, act) in enumerate(rows):
        v["up"][i], v["act_n"][i] = up, len(act)
        v["act"][i][: len(act)] = act
    return v


def _scamp_views(rows):
    v = np.zeros(len(rows), _abi.STRATEGY_VIEW_DTYPE)
    for i, (up, view) in enumerate(rows):
        v["up"][i], v["view_n"][i] = up, len(view)
        v["view"][i][: len(view)] = view
    return v


def test_reference_reads_both_kinds_of_rows_and_sums_batches():
    rows = [(True, [1, 1, 0, 3, 2]), (True, [2, 3]), (True, [0]), (False, [0, 1, 2])]
    want = R.reference_rows(rows, [3, 0, 1])
    R.compare(R.reference(_hv_views(rows), "hv", [3, 0, 1]), want)
    R.compare(R.reference(_scamp_views(rows), "scamp", [3, 0, 1]), want)
    # 70 nodes on a directed cycle, every id a source in two batches (64 + 6):
    # each source reaches 69 nodes at distances 1..69, the bins saturate at 63
    cyc = _scamp_views(_up([[(i + 1) % 70] for i in range(70)]))
    allp = R.reference_all(cyc, "scamp")
    assert allp["sources_live"] == 70 and allp["pairs_reached"] == 70 * 69 and allp["pairs_unreached"] == 0
    assert allp["dist_sum"] == 70 * (69 * 70 // 2) and allp["ecc_max"] == 69 and allp["levels"] == 70
    assert allp["dist"][62] == 70 and allp["dist"][63] == 70 * 7 and allp["dist"][0] == 0
    assert len(allp["reach"]) == 70 and (allp["reach"] == 69).all() and (allp["ecc"] == 69).all()
