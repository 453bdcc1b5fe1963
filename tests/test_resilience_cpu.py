"""CPU checks of psim_get_resilience's boundary: the struct layout of the
ctypes mirror against the header, where the entry point is declared, and the
reference (tests/_resilience.py, the yardstick of tests/test_gpu_resilience.py)
on rows whose numbers are worked out by hand below and on the oracle's rows,
pinned to anchors computed when the call was specified."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _graph_metrics as G
import _resilience as R
import _scenarios as S
from _oracle import Oracle
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
FULL = 0xFFFFFFFF


def test_struct_layout_matches_header(tmp_path):
    m, c = _abi.PsimResilience, _abi.PsimFailureCase
    names, cnames = [n for n, _ in m._fields_], [n for n, _ in c._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%zu %%d\\n", sizeof(psim_resilience), sizeof(psim_failure_case), PSIM_FAIL_CASES);\n'
        '%s%s return 0;}\n'
        % (HDR, "".join('printf("%%zu\\n", offsetof(psim_resilience, %s));\n' % n for n in names),
           "".join('printf("%%zu\\n", offsetof(psim_failure_case, %s));\n' % n for n in cnames)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [C.sizeof(m), C.sizeof(c), _abi.FAIL_CASES] and C.sizeof(c) == 16
    assert got[3:] == [getattr(m, n).offset for n in names] + [getattr(c, n).offset for n in cnames]
    assert cnames == ["source", "threshold", "salt", "reserved"]
    assert R.CASES == _abi.FAIL_CASES == _abi.GRAPH_SOURCES and G.MAX_LEVELS == _abi.GRAPH_MAX_LEVELS
    assert sorted(n for n in names if n != "reserved") == sorted(R.SCALARS + R.ARRAYS)
    assert all(t in (C.c_uint64, C.c_uint64 * 64, C.c_uint64 * 8) for _, t in m._fields_)
    assert C.sizeof(m) == 8 * (4 + 7 * 64 + 3 + 8)


def test_entry_point_is_gpu_only():
    assert "get_resilience" in _abi.GPU_ONLY
    assert "get_resilience" not in _abi.SIGNATURES
    assert re.search(r"\bpsim_get_resilience\s*\(", open(HDR).read())
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", open(HDR).read())


def test_mix64_is_splitmix64s_finalizer():
    # (the published splitmix64 stream from state 0: its first output is mix64 of the golden-ratio increment)
    assert R.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert R.mix64(0) == 0 and 0 <= R.u(5, 3, 7) <= FULL


# ---- hand-built rows
def _ring(lo, hi):
    """a directed ring over ids lo .. hi - 1"""
    return [(True, [lo + (i + 1 - lo) % (hi - lo)]) for i in range(lo, hi)]


def _slot(m, j):
    return {k: int(m[k][j]) for k in R.ARRAYS}


def _lowest(n, src, salt, seed):
    """the node != src that fails first as the threshold rises, and the
    threshold that fails it alone"""
    us = sorted((R.u(v, salt, seed), v) for v in range(n) if v != src)
    assert us[0][0] < us[1][0]
    return us[0][1], us[0][0] + 1


def test_directed_ring():
    rows = _ring(0, 10)
    w, thr = _lowest(10, 3, 0, 11)
    m = R.reference_rows(rows, [(3, 0, 0), (3, thr, 0)], fail_seed=11)
    assert (m["n_up"], m["links"], m["cases_live"], m["live_mask"]) == (10, 10, 2, 3)
    assert _slot(m, 0) == dict(alive=10, links_alive=10, no_out=0, no_in=0, reached=9, hop_sum=45, ecc=9)
    # w alone fails: its two links go, the flood stops before it
    r = (w - 3 - 1) % 10
    assert _slot(m, 1) == dict(alive=9, links_alive=8, no_out=1, no_in=1, reached=r, hop_sum=r * (r + 1) // 2, ecc=r)
    assert (m["ecc_max"], m["levels"], m["truncated"]) == (9, 10, 0)
    assert not any(m[k][2:].any() for k in R.ARRAYS)


def test_star_whose_hub_fails():
    rows = [(True, list(range(1, 10)))] + [(True, [0])] * 9
    seed, src = 5, 4
    thr = R.u(0, 0, seed) + 1
    kept = 1 + sum(1 for v in range(1, 10) if v != src and R.u(v, 0, seed) >= thr)
    m = R.reference_rows(rows, [(src, 0, 0), (src, thr, 0)], fail_seed=seed)
    assert _slot(m, 0) == dict(alive=10, links_alive=18, no_out=0, no_in=0, reached=9, hop_sum=1 + 2 * 8, ecc=2)
    assert _slot(m, 1) == dict(alive=kept, links_alive=0, no_out=kept, no_in=kept, reached=0, hop_sum=0, ecc=0)
    assert (m["ecc_max"], m["levels"]) == (2, 3)
    # the hub as the source never fails in its own case, whatever its u
    m = R.reference_rows(rows, [(0, thr, 0)], fail_seed=seed)
    kept = 1 + sum(1 for v in range(1, 10) if R.u(v, 0, seed) >= thr)
    assert _slot(m, 0) == dict(alive=kept, links_alive=2 * (kept - 1), no_out=0 if kept > 1 else 1,
                               no_in=0 if kept > 1 else 1, reached=kept - 1, hop_sum=kept - 1,
                               ecc=1 if kept > 1 else 0)


def test_two_parts_never_meet():
    rows = _ring(0, 5) + _ring(5, 12)
    m = R.reference_rows(rows, [(0, 0, 0), (7, 0, 9)], fail_seed=1)
    assert _slot(m, 0) == dict(alive=12, links_alive=12, no_out=0, no_in=0, reached=4, hop_sum=10, ecc=4)
    assert _slot(m, 1) == dict(alive=12, links_alive=12, no_out=0, no_in=0, reached=6, hop_sum=21, ecc=6)
    assert (m["ecc_max"], m["levels"], m["truncated"]) == (6, 7, 0)


def test_repeated_source_and_salts():
    rows = _ring(0, 10)
    w, thr = _lowest(10, 3, 0, 11)
    m = R.reference_rows(rows, [(3, thr, 0), (3, 0, 0), (3, thr, 0), (3, thr, 1)], fail_seed=11)
    assert m["live_mask"] == 15 and _slot(m, 0) == _slot(m, 2)
    assert _slot(m, 1)["reached"] == 9
    # another salt fails another set: the nodes below thr under salt 1
    gone = {v for v in range(10) if v != 3 and R.u(v, 1, 11) < thr}
    assert _slot(m, 3)["alive"] == 10 - len(gone)


def test_dead_source_and_dead_nodes():
    rows = _ring(0, 10)
    rows[2] = (False, [3])
    m = R.reference_rows(rows, [(2, 0, 0), (3, 0, 0), (0, 0, 0)], fail_seed=3)
    assert (m["n_up"], m["links"], m["cases_live"], m["live_mask"]) == (9, 8, 2, 0b110)
    assert _slot(m, 0) == dict(alive=0, links_alive=0, no_out=0, no_in=0, reached=0, hop_sum=0, ecc=0)
    # from 3 the ring runs to 1, which points at the dead node; from 0 it ends at 1
    assert _slot(m, 1) == dict(alive=9, links_alive=8, no_out=1, no_in=1, reached=8, hop_sum=36, ecc=8)
    assert _slot(m, 2) == dict(alive=9, links_alive=8, no_out=1, no_in=1, reached=1, hop_sum=1, ecc=1)
    # self-links, repeats and links to ids that are down count nowhere
    rows = [(True, [0, 1, 1, 2]), (True, [1]), (False, [0])]
    m = R.reference_rows(rows, [(0, 0, 0)])
    assert (m["n_up"], m["links"]) == (2, 1)
    assert _slot(m, 0) == dict(alive=2, links_alive=1, no_out=1, no_in=1, reached=1, hop_sum=1, ecc=1)
    # no case at all, and only dead ones
    m = R.reference_rows(_ring(0, 4))
    assert (m["n_up"], m["links"], m["cases_live"], m["levels"]) == (4, 4, 0, 0)
    m = R.reference_rows([(False, [1]), (False, [0])], [(0, 0, 0)])
    assert all(not np.any(v) for v in m.values())


def test_threshold_zero_and_full():
    rows = _ring(0, 10)
    assert all(R.u(v, 0, 0) < FULL for v in range(10))
    m = R.reference_rows(rows, [(6, 0, 0), (6, FULL, 0)])
    assert _slot(m, 0) == dict(alive=10, links_alive=10, no_out=0, no_in=0, reached=9, hop_sum=45, ecc=9)
    assert _slot(m, 1) == dict(alive=1, links_alive=0, no_out=1, no_in=1, reached=0, hop_sum=0, ecc=0)


def test_level_cap_truncates():
    rows = _ring(0, 10)
    m = R.reference_rows(rows, [(3, 0, 0), (4, FULL, 0)], max_levels=3)
    assert _slot(m, 0) == dict(alive=10, links_alive=10, no_out=0, no_in=0, reached=3, hop_sum=6, ecc=3)
    assert (m["ecc_max"], m["levels"], m["truncated"]) == (3, 3, 1)
    m = R.reference_rows(rows, [(3, 0, 0)], max_levels=9)
    assert (int(m["reached"][0]), m["levels"], m["truncated"]) == (9, 9, 1)
    m = R.reference_rows(rows, [(3, 0, 0)], max_levels=10)
    assert (int(m["reached"][0]), m["levels"], m["truncated"]) == (9, 10, 0)
    # a cap past the largest is clamped to it
    assert R.reference_rows(rows, [(3, 0, 0)], max_levels=1 << 20)["levels"] == 10


# ---- the oracle's rows against the anchors
SRC_A, SRC_B, GRID_A = R.SRC_A, R.SRC_B, R.GRID_A


def _q(m, q, key):
    return int(m[key][8 * q: 8 * q + 8].sum())


def test_anchor_a_hyparview():
    o = S.doubling(Oracle, n=203, seed=3, rounds=30)[0]
    rows = G.rows_of(o.nodes(), "hv")
    o.close()
    m = R.reference_rows(rows, [(5, 0, 0)], fail_seed=7)
    assert (m["n_up"], m["links"]) == (203, 790)
    assert _slot(m, 0) == dict(alive=203, links_alive=790, no_out=0, no_in=0, reached=202, hop_sum=831, ecc=7)
    m = R.reference_rows(rows, [(5, 0, 0)], fail_seed=7, max_levels=3)
    assert (int(m["reached"][0]), int(m["hop_sum"][0]), m["levels"], m["truncated"]) == (57, 146, 3, 1)
    m = R.reference_rows(rows, [(5, FULL, 0)], fail_seed=7)
    assert _slot(m, 0) == dict(alive=1, links_alive=0, no_out=1, no_in=1, reached=0, hop_sum=0, ecc=0)
    m = R.reference_rows(rows, R.grid(SRC_A), fail_seed=7)
    assert m["cases_live"] == 64 and m["live_mask"] == (1 << 64) - 1
    assert np.array_equal(m["no_in"], m["no_out"])      # (the overlay's links are symmetric)
    for q, want in GRID_A.items():
        got = tuple(_q(m, q, k) for k in ("alive", "links_alive", "reached", "hop_sum", "no_in"))
        assert got + (int(m["ecc"][8 * q: 8 * q + 8].max()),) == want, q


def test_anchor_b_scamp_v2_with_dead_nodes():
    o = S.pl_doubling(Oracle, n=2048, seed=13, rounds=33, strategy=2, crash_at=30)[0]
    views = o.strategy_nodes()
    o.close()
    assert SRC_B == [int(x) for x in np.flatnonzero(views["up"])[::230]][:8]
    m = R.reference_rows(G.rows_of(views, "scamp"), R.grid(SRC_B), fail_seed=7)
    assert m["n_up"] == 1844 and m["cases_live"] == 64
    keys = ("alive", "reached", "hop_sum", "no_in", "no_out")
    assert tuple(_q(m, 0, k) for k in keys) == (14752, 1975, 15260, 3496, 840)
    assert tuple(_q(m, 3, k) for k in keys) == (10272, 442, 2562, 3761, 2656)
