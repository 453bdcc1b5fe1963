"""CPU checks of psim_get_gossip_reach's boundary: the struct layout of the
ctypes mirror against the header, where the entry point is declared, and the
reference (tests/_gossip.py, the yardstick of tests/test_gpu_gossip.py) on rows
whose numbers are worked out by hand below and on the oracle's rows, pinned to
anchors computed when the call was specified."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _gossip as P
import _graph_metrics as G
import _resilience as R
import _scenarios as S
from _oracle import Oracle
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
FULL = 0xFFFFFFFF


def test_struct_layout_matches_header(tmp_path):
    m, c = _abi.PsimGossipReach, _abi.PsimGossipCase
    names, cnames = [n for n, _ in m._fields_], [n for n, _ in c._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%zu\\n", sizeof(psim_gossip_reach), sizeof(psim_gossip_case));\n'
        '%s%s return 0;}\n'
        % (HDR, "".join('printf("%%zu\\n", offsetof(psim_gossip_reach, %s));\n' % n for n in names),
           "".join('printf("%%zu\\n", offsetof(psim_gossip_case, %s));\n' % n for n in cnames)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [C.sizeof(m), C.sizeof(c)]
    assert got[2:] == [getattr(m, n).offset for n in names] + [getattr(c, n).offset for n in cnames]
    assert cnames == ["source", "threshold", "salt", "fanout"]
    assert sorted(n for n in names if n != "reserved") == sorted(P.SCALARS + P.ARRAYS)
    assert all(t in (C.c_uint64, C.c_uint64 * 64, C.c_uint64 * 8) for _, t in m._fields_)
    assert C.sizeof(m) == 8 * (4 + 6 * 64 + 3 + 8) and C.sizeof(c) == 16


def test_entry_point_is_gpu_only():
    assert "get_gossip_reach" in _abi.GPU_ONLY
    assert "get_gossip_reach" not in _abi.SIGNATURES
    assert re.search(r"\bpsim_get_gossip_reach\s*\(", open(HDR).read())
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", open(HDR).read())


def test_keys_and_choice():
    assert P.GOLDEN == 0x9E3779B97F4A7C15 and R.mix64(P.GOLDEN) == 0xE220A8397B1DCDAF
    assert P.h(9, 3, 7) >> 32 == R.u(9, 3, 7)
    assert P.w(9, 4, 3, 7) == R.mix64((P.h(9, 3, 7) + P.GOLDEN * 5) & R.M64)
    ni = {1, 2, 3, 5, 8, 13}
    by_key = sorted(ni, key=lambda p: (P.w(0, p, 2, 1), p))
    for f in range(1, 6):
        assert P.chosen(0, ni, 2, f, 1) == set(by_key[:f])
    assert P.chosen(0, ni, 2, 0, 1) == P.chosen(0, ni, 2, 6, 1) == P.chosen(0, ni, 2, FULL, 1) == ni
    # equal salts choose alike whatever the threshold; the choice is nested in the fanout
    assert P.chosen(0, ni, 2, 2, 1) < P.chosen(0, ni, 2, 3, 1)
    assert P.chosen(0, set(), 2, 3, 1) == set()


# ---- hand-built rows
def _ring(lo, hi):
    """a directed ring over ids lo .. hi - 1"""
    return [(True, [lo + (i + 1 - lo) % (hi - lo)]) for i in range(lo, hi)]


def _star():
    return [(True, list(range(1, 10)))] + [(True, [0])] * 9


def _slot(m, j):
    return {k: int(m[k][j]) for k in P.ARRAYS}


@pytest.mark.parametrize("fanout", [0, 1, 2, 128, FULL])
def test_directed_ring(fanout):
    m = P.reference_rows(_ring(0, 10), [(3, 0, 0, fanout)], fail_seed=11)
    assert (m["n_up"], m["links"], m["cases_live"], m["live_mask"]) == (10, 10, 1, 1)
    # the last node's copy comes back to the source: the one duplicate
    assert _slot(m, 0) == dict(alive=10, reached=9, hop_sum=45, ecc=9, sent=10, lost=0)
    assert (m["ecc_max"], m["levels"], m["truncated"]) == (9, 10, 0)
    assert not any(m[k][1:].any() for k in P.ARRAYS)


@pytest.mark.parametrize("f", range(1, 10))
def test_star_from_its_hub(f):
    """the hub sends f copies, each leaf reached sends its one copy back"""
    m = P.reference_rows(_star(), [(0, 0, 0, f)], fail_seed=5)
    assert _slot(m, 0) == dict(alive=10, reached=f, hop_sum=f, ecc=1, sent=2 * f, lost=0)
    assert (m["levels"], m["truncated"]) == (2, 0)


def test_star_whose_hub_fails():
    seed, src = 5, 4
    thr = R.u(0, 0, seed) + 1
    kept = 1 + sum(1 for v in range(1, 10) if v != src and R.u(v, 0, seed) >= thr)
    m = P.reference_rows(_star(), [(src, 0, 0, 1), (src, thr, 0, 1), (src, thr, 0, 0), (src, 0, 0, 3)], fail_seed=seed)
    # the leaf's only link is the hub, the hub picks one leaf, which answers it
    one = next(iter(P.chosen(0, set(range(1, 10)), 0, 1, seed)))
    back = 1 if one == src else 2
    assert _slot(m, 0) == dict(alive=10, reached=back, hop_sum=1 + 2 * (back - 1), ecc=back, sent=1 + back, lost=0)
    # the hub failed: the leaf's copy is lost, before anybody detects the failure
    for j in (1, 2):
        assert _slot(m, j) == dict(alive=kept, reached=0, hop_sum=0, ecc=0, sent=1, lost=1)
    three = P.chosen(0, set(range(1, 10)), 0, 3, seed)
    r = 1 + len(three - {src})
    assert _slot(m, 3) == dict(alive=10, reached=r, hop_sum=1 + 2 * (r - 1), ecc=2 if r > 1 else 1,
                               sent=1 + 3 + (r - 1), lost=0)
    # the hub as the source never fails in its own case; its copies to failed leaves are lost
    m = P.reference_rows(_star(), [(0, thr, 0, 0), (0, thr, 0, 4)], fail_seed=seed)
    kept = 1 + sum(1 for v in range(1, 10) if R.u(v, 0, seed) >= thr)
    assert _slot(m, 0) == dict(alive=kept, reached=kept - 1, hop_sum=kept - 1, ecc=1 if kept > 1 else 0,
                               sent=9 + kept - 1, lost=10 - kept)
    four = P.chosen(0, set(range(1, 10)), 0, 4, seed)
    ok = sum(1 for v in four if R.u(v, 0, seed) >= thr)
    assert _slot(m, 1) == dict(alive=kept, reached=ok, hop_sum=ok, ecc=1 if ok else 0, sent=4 + ok, lost=4 - ok)


def test_dead_source_and_dead_nodes():
    rows = _ring(0, 10)
    rows[2] = (False, [3])
    m = P.reference_rows(rows, [(2, 0, 0, 1), (3, 0, 0, 1), (0, 0, 0, 0)], fail_seed=3)
    assert (m["n_up"], m["links"], m["cases_live"], m["live_mask"]) == (9, 8, 2, 0b110)
    assert _slot(m, 0) == dict(alive=0, reached=0, hop_sum=0, ecc=0, sent=0, lost=0)
    # node 1's entry names the down node: no candidate, so no copy and none lost
    assert _slot(m, 1) == dict(alive=9, reached=8, hop_sum=36, ecc=8, sent=8, lost=0)
    assert _slot(m, 2) == dict(alive=9, reached=1, hop_sum=1, ecc=1, sent=1, lost=0)
    m = P.reference_rows(_ring(0, 4))
    assert (m["n_up"], m["links"], m["cases_live"], m["levels"]) == (4, 4, 0, 0)
    m = P.reference_rows([(False, [1]), (False, [0])], [(0, 0, 0, 2)])
    assert all(not np.any(v) for v in m.values())


def test_level_cap_nodes_at_the_cap_do_not_send():
    rows = _ring(0, 10)
    m = P.reference_rows(rows, [(3, 0, 0, 1), (4, FULL, 0, 0)], max_levels=3)
    # 3, 4 and 5 sent; 6 was reached at distance 3 == the cap and keeps its copy
    assert _slot(m, 0) == dict(alive=10, reached=3, hop_sum=6, ecc=3, sent=3, lost=0)
    assert _slot(m, 1) == dict(alive=1, reached=0, hop_sum=0, ecc=0, sent=1, lost=1)
    assert (m["ecc_max"], m["levels"], m["truncated"]) == (3, 3, 1)
    m = P.reference_rows(rows, [(3, 0, 0, 0)], max_levels=9)
    assert (_slot(m, 0)["reached"], _slot(m, 0)["sent"], m["levels"], m["truncated"]) == (9, 9, 9, 1)
    m = P.reference_rows(rows, [(3, 0, 0, 0)], max_levels=10)
    assert (_slot(m, 0)["reached"], _slot(m, 0)["sent"], m["levels"], m["truncated"]) == (9, 10, 10, 0)
    assert P.reference_rows(rows, [(3, 0, 0, 0)], max_levels=1 << 20)["levels"] == 10


# ---- the oracle's rows
_ROWS = {}


def _rows_a():
    if "a" not in _ROWS:
        o = S.doubling(Oracle, n=203, seed=3, rounds=30)[0]
        _ROWS["a"] = G.rows_of(o.nodes(), "hv")
        o.close()
    return _ROWS["a"]


def test_row_order_and_repeats_change_nothing():
    rows = _rows_a()
    rng = random.Random(4)
    mixed = []
    for up, ids in rows:
        ids = ids + ids[:2]
        rng.shuffle(ids)
        mixed.append((up, ids))
    cases = P.grid(R.SRC_A, 3)
    a, b = P.reference_rows(rows, cases, 7), P.reference_rows(mixed, cases, 7)
    P.compare(a, b)
    assert a["sent"].any() and a["lost"].any()


def test_flood_and_wide_fanout_are_resilience():
    rows = _rows_a()
    want = R.reference_rows(rows, R.grid(R.SRC_A), fail_seed=7)
    widest = max(len(v) for v in G.links_of(rows).values())
    assert widest == 5
    for f in (0, widest, widest + 1, FULL):
        m = P.reference_rows(rows, [c + (f,) for c in R.grid(R.SRC_A)], fail_seed=7)
        for k in ("alive", "reached", "hop_sum", "ecc") + P.SCALARS:
            assert np.array_equal(m[k], want[k]), (f, k)
        assert int(m["sent"][:8].sum()) == 8 * 790 and not m["lost"][:8].any()


def _sums(m, s):
    return tuple(int(m[k][s].sum()) for k in ("alive", "reached", "hop_sum", "sent", "lost")) + (int(m["ecc"][s].max()),)


@pytest.mark.parametrize("q", [0, 3, 5])
def test_anchor_a_hyparview(q):
    rows = _rows_a()
    m = P.reference_rows(rows, P.grid(R.SRC_A, q), fail_seed=7)
    assert (m["n_up"], m["links"], m["cases_live"], m["live_mask"]) == (203, 790, 64, (1 << 64) - 1)
    ks = [len(v) for v in G.links_of(rows).values()]
    assert (min(ks), max(ks)) == (2, 5)
    for fi in range(8):
        assert _sums(m, slice(8 * fi, 8 * fi + 8)) == P.ANCHOR_A[q][min(fi, 4)], (q, P.FANOUTS[fi])


def test_anchor_a_single_cases():
    rows = _rows_a()
    want = {2: (131, 1602, 21, 264), 3: (198, 1261, 12, 574), 0: (202, 831, 7, 790)}
    for f, x in want.items():
        m = P.reference_rows(rows, [(5, 0, 0, f)], fail_seed=7)
        assert tuple(int(m[k][0]) for k in ("reached", "hop_sum", "ecc", "sent")) == x, f
        assert m["lost"][0] == 0 and m["alive"][0] == 203
    m = P.reference_rows(rows, [(5, 0, 0, 2)], fail_seed=7, max_levels=3)
    assert (int(m["reached"][0]), int(m["hop_sum"][0]), int(m["sent"][0]), m["truncated"], m["levels"]) == (7, 15, 10, 1, 3)


def test_anchor_v1_large_view():
    o = S.pl_v1_large_view(Oracle, leave_from=10**9, leave_to=0, rounds=40)[0]
    rows = G.rows_of(o.strategy_nodes(), "scamp")
    o.close()
    m = P.reference_rows(rows, P.v1_cases(), fail_seed=5)
    assert (m["n_up"], m["links"], max(len(v) for v in G.links_of(rows).values())) == (180, 424, 108)
    got = [(int(m["reached"][j]), int(m["sent"][j]), int(m["ecc"][j])) for j in range(28)]
    assert got == [x for f in P.ANCHOR_V1 for x in P.ANCHOR_V1[f]]
    assert not m["lost"].any()


def test_anchor_b_scamp_v2_with_dead_nodes():
    o = S.pl_doubling(Oracle, n=2048, seed=13, rounds=33, strategy=2, crash_at=30)[0]
    rows = G.rows_of(o.strategy_nodes(), "scamp")
    o.close()
    m = P.reference_rows(rows, P.b_cases(), fail_seed=7)
    assert m["n_up"] == 1844 and m["cases_live"] == 32
    for fi, f in enumerate(P.ANCHOR_B):
        assert _sums(m, slice(8 * fi, 8 * fi + 8))[:5] == P.ANCHOR_B[f], f
