"""CPU checks of psim_get_relay_reach's boundary: the struct layout of the
ctypes mirror against the header, where the entry point is declared, and the
reference (tests/_relay.py, the yardstick of tests/test_gpu_relay.py) on rows
whose numbers are worked out by hand below and on the oracle's rows, pinned to
anchors computed when the call was specified."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _relay as P
import _scenarios as S
from _oracle import Oracle
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
MAP, DOWN = P.MAP_BIT, P.CONN_DOWN


def test_struct_layout_matches_header(tmp_path):
    m, c = _abi.PsimRelayReach, _abi.PsimRelayCase
    names, cnames = [n for n, _ in m._fields_], [n for n, _ in c._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%zu %%d %%d\\n", sizeof(psim_relay_reach), sizeof(psim_relay_case),\n'
        'PSIM_RELAY_CASES, PSIM_RELAY_MAX_TTL);\n'
        '%s%s return 0;}\n'
        % (HDR, "".join('printf("%%zu\\n", offsetof(psim_relay_reach, %s));\n' % n for n in names),
           "".join('printf("%%zu\\n", offsetof(psim_relay_case, %s));\n' % n for n in cnames)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [C.sizeof(m), C.sizeof(c), _abi.RELAY_CASES, _abi.RELAY_MAX_TTL] and got[2:4] == [P.CASES, P.MAX_TTL]
    assert got[4:] == [getattr(m, n).offset for n in names] + [getattr(c, n).offset for n in cnames]
    assert cnames == ["source", "target", "ttl", "reserved"]
    assert sorted(n for n in names if n != "reserved") == sorted(P.SCALARS + P.ARRAYS + P.HISTS)
    assert all(t in (C.c_uint64, C.c_uint64 * 64, C.c_uint64 * 8) for _, t in m._fields_)
    assert C.sizeof(m) == 8 * (5 + 64 + 5 + 10 * 64 + 8) and C.sizeof(c) == 16


def test_entry_point_is_gpu_only():
    assert "get_relay_reach" in _abi.GPU_ONLY
    assert "get_relay_reach" not in _abi.SIGNATURES
    assert re.search(r"\bpsim_get_relay_reach\s*\(", open(HDR).read())
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", open(HDR).read())


# ---- hand-built rows
def _slot(m, j=0, **kw):
    want = dict.fromkeys(P.ARRAYS, 0)
    want.update(kw)
    assert P.slot(m, j) == want
    return True


def _line():
    return [P.row([1]), P.row([0, 2]), P.row([1, 3]), P.row([2, 4]), P.row([3])]


def test_line_of_five():
    """0 - 1 - 2 - 3 - 4, the out-links are the active views, case (0, 4, ttl 5).
    level 1: (1, 4) x1                        [origin: 1 relay]
    level 2: (0, 3) x1, (2, 3) x1             [2 relays]
    level 3: (1, 2) x2, (3, 2) x1             [1 + 2 relays]; 3 holds 4: delivered 1 after 4 sends
    level 4: (0, 1) x2, (2, 1) x2             [2 x 2 relays]
    level 5: (1, 0) x4, (3, 0) x2             [2 + 2 x 2 relays]; 3 delivers 2 after 6 sends, 4 expire at 1"""
    m = P.reference_rows(_line(), [(0, 4, 5)])
    assert _slot(m, delivered=3, first_hop=4, hop_sum=4 + 2 * 6, relays=1 + 2 + 3 + 4 + 6, expired=4, levels=5, peak=2)
    assert {k: m[k] for k in P.SCALARS} == dict(n_up=5, out_entries=8, out_usable=8, out_nonmember=0, members_down=0,
                                                cases_live=1, live_mask=1, direct_mask=0, truncated_mask=0,
                                                levels_max=5)
    assert {i: int(v) for i, v in enumerate(m["out_degree"]) if v} == {1: 2, 2: 3}
    # ttl 3: the copy that reaches node 3 arrives with ttl 0 and is still delivered; the two at node 1 expire
    m = P.reference_rows(_line(), [(0, 4, 3)])
    assert _slot(m, delivered=1, first_hop=4, hop_sum=4, relays=1 + 2 + 3, expired=2, levels=3, peak=2)
    # ttl 2 ends before node 3
    m = P.reference_rows(_line(), [(0, 4, 2)])
    assert _slot(m, relays=1 + 2, expired=2, levels=2, peak=2)
    # the cap: level 3 is cut off with its 3 copies, already counted as relays
    m = P.reference_rows(_line(), [(0, 4, 5)], max_levels=2)
    assert _slot(m, relays=1 + 2 + 3, in_flight=3, levels=2, peak=2) and m["truncated_mask"] == 1
    assert P.reference_rows(_line(), [(0, 4, 5)], max_levels=99)["levels_max"] == 5


def test_triangle_with_a_stale_entry():
    """0, 1, 2 hold each other; 0's common set still names 3 (both of its
    other entries in the map form), which no view holds.  Case (0, 3, ttl 2):
    origin: 2 relays, the send to 3 refused; level 1: (1, 1), (2, 1), two
    relays each; level 2: (0, 0) x2, (2, 0), (1, 0): 4 copies expire."""
    rows = [P.row([1, 2], [1, 2 | MAP, 3 | MAP]), P.row([0, 2]), P.row([0, 1]), P.row([])]
    m = P.reference_rows(rows, [(0, 3, 2)])
    assert _slot(m, relays=2 + 4, refused=1, expired=4, levels=2, peak=3)
    assert (m["n_up"], m["out_entries"], m["out_usable"], m["out_nonmember"]) == (4, 7, 6, 1)
    assert {i: int(v) for i, v in enumerate(m["out_degree"]) if v} == {0: 1, 2: 3}
    # the atom self leaves out(i), the map self stays and is refused; a repeated peer is two sends
    rows[1] = P.row([0, 2], [1, 1 | MAP, 0, 0 | MAP])
    m = P.reference_rows(rows, [(1, 3, 1)])
    assert _slot(m, relays=2, refused=1, expired=2, levels=1, peak=1)
    assert (m["out_entries"], m["out_usable"], m["out_nonmember"]) == (8, 6, 2)
    assert {i: int(v) for i, v in enumerate(m["out_degree"]) if v} == {0: 1, 2: 3}


def _down():
    return [P.row([1]), P.row([0, 2], conn=[2 | DOWN]), P.row([1])]


def test_member_without_a_connection_restarts_the_flood():
    """0 - 1 - 2, 1 holds 2 as an active member whose connection is down.
    ttl 1: level 1: (1, 0): restart, forward(1, 1): the send to 0 relayed, the
    one to 2 refused; level 2: (0, 0) expires.
    ttl 2: (1, 1) restarts -> (0, 1) -> (1, 0) restarts -> ...: a cycle of two
    levels, one relay a level, a restart and a refusal every other one."""
    m = P.reference_rows(_down(), [(0, 2, 1)])
    assert _slot(m, relays=2, refused=1, restarts=1, expired=1, levels=2, peak=1)
    assert (m["members_down"], m["out_usable"], m["out_entries"], m["truncated_mask"]) == (1, 3, 4, 0)
    m = P.reference_rows(_down(), [(0, 2, 2)])
    assert _slot(m, relays=17, refused=8, restarts=8, in_flight=1, levels=16, peak=1)
    assert (m["truncated_mask"], m["levels_max"]) == (1, 16)
    m = P.reference_rows(_down(), [(0, 2, 2)], max_levels=3)
    assert _slot(m, relays=4, refused=2, restarts=2, in_flight=1, levels=3, peak=1) and m["truncated_mask"] == 1
    # a down mark for a peer outside the active view: no state at all, and no restart
    rows = [P.row([1]), P.row([0], [0, 2], conn=[2 | DOWN]), P.row([1])]
    m = P.reference_rows(rows, [(0, 2, 1)])
    assert _slot(m, relays=1, expired=1, levels=1, peak=1) and m["members_down"] == 0 and m["out_nonmember"] == 1


def test_lingering_peer_and_direct():
    """a connection beyond the active view delivers directly; at a relay the
    lingering target is no active member, so the relay only forwards to it"""
    rows = [P.row([1], conn=[3]), P.row([0, 2]), P.row([1], [1, 3], conn=[3]), P.row([])]
    m = P.reference_rows(rows, [(0, 3, 5), (1, 0, 5), (1, 3, 1), (3, 0, 4)])
    assert (m["cases_live"], m["live_mask"], m["direct_mask"]) == (4, 0b1111, 0b0011)
    for j in (0, 1):
        assert _slot(m, j, delivered=1, first_hop=1, hop_sum=1)
    # 1 -> 0, 2 with ttl 0; 2 does not hold 3 in its view: expired, like the copy at 0
    assert _slot(m, 2, relays=2, expired=2, levels=1, peak=2)
    # 3 has no out-link: nothing is sent at all
    assert _slot(m, 3)
    assert (m["out_entries"], m["out_usable"], m["out_nonmember"]) == (5, 5, 1)


def test_dead_source_and_dead_target():
    rows = _line()
    rows[2] = P.row([1, 3], up=False)
    m = P.reference_rows(rows, [(2, 4, 5), (0, 2, 5), (0, 1, 5), (0, 4, 5)])
    assert (m["n_up"], m["cases_live"], m["live_mask"], m["direct_mask"]) == (4, 2, 0b1100, 0b0100)
    assert _slot(m, 0) and _slot(m, 1) and _slot(m, 2, delivered=1, first_hop=1, hop_sum=1)
    # 0 -> 1 -> 0 -> ...: node 1's send to the dead node is refused every other level
    assert _slot(m, 3, relays=5, refused=2, expired=1, levels=5, peak=1)
    assert (m["out_entries"], m["out_usable"]) == (6, 4)
    m = P.reference_rows([P.row([1], up=False), P.row([0], up=False)], [(0, 1, 3)])
    assert all(not np.any(v) for v in m.values())
    assert P.reference_rows(_line())["cases_live"] == 0


# ---- the oracle's rows
_ROWS = {}


def _rows(key):
    if key not in _ROWS:
        run = {"a": lambda: S.doubling(Oracle, n=203, seed=3, rounds=30),
               "b": lambda: S.churn_partition(Oracle, n=512, rounds=60),
               "c": lambda: S.crash_only(Oracle)}[key]
        o = run()[0]
        _ROWS[key] = P.rows_of(o.nodes())
        o.close()
    return _ROWS[key]


ANCHOR_A = {  # (s, d, ttl, cap): delivered, first_hop, hop_sum, relays, refused, expired, levels, truncated
    (5, 100, 5, 0): (48, 2, 271, 1593, 175, 1170, 5, 0),
    (5, 100, 8, 0): (2400, 2, 20737, 108407, 12957, 80101, 8, 0),
    (0, 202, 3, 0): (0, 0, 0, 41, 2, 31, 3, 0),
    (17, 64, 16, 0): (45794999, 6, 764730062, 13597090566, 1011236305, 10394417266, 16, 0),
    (17, 64, 16, 3): (0, 0, 0, 362, 55, 0, 3, 1),
}
ANCHOR_B = {  # (ttl, cap): relays, refused, expired, restarts, levels, truncated
    (1, 0): (8, 1, 7, 1, 2, 0),
    (3, 6): (1706, 153, 568, 72, 6, 1),
    (5, 6): (9627, 590, 2215, 215, 6, 1),
    (5, 0): (200105280, 12796992, 29688977, 4242794, 16, 1),
}


def test_anchor_a_census():
    m = P.reference_rows(_rows("a"))
    assert [m[k] for k in P.CENSUS] == [203, 908, 790, 118, 0]
    assert {i: int(v) for i, v in enumerate(m["out_degree"]) if v} == {2: 26, 3: 44, 4: 59, 5: 74}


@pytest.mark.parametrize("case", list(ANCHOR_A), ids=lambda c: "-".join(map(str, c)))
def test_anchor_a_cases(case):
    s, d, ttl, cap = case
    m = P.reference_rows(_rows("a"), [(s, d, ttl)], cap)
    got = tuple(int(m[k][0]) for k in ("delivered", "first_hop", "hop_sum", "relays", "refused", "expired", "levels"))
    assert got + (m["truncated_mask"],) == ANCHOR_A[case]
    assert m["restarts"][0] == 0 and m["direct_mask"] == 0 and m["levels_max"] == ANCHOR_A[case][6]


def test_anchor_a_direct():
    m = P.reference_rows(_rows("a"), [(5, 50, 5)])
    assert m["direct_mask"] == 1 and _slot(m, delivered=1, first_hop=1, hop_sum=1)


def test_anchor_b_restart_cycle():
    rows = _rows("b")
    m = P.reference_rows(rows)
    assert [m[k] for k in P.CENSUS] == [512, 2072, 1962, 109, 1]
    assert rows[275][3] == [119 | DOWN] and 119 in rows[275][1]
    for (ttl, cap), want in ANCHOR_B.items():
        m = P.reference_rows(rows, [(295, 119, ttl)], cap)
        got = tuple(int(m[k][0]) for k in ("relays", "refused", "expired", "restarts", "levels"))
        assert got + (m["truncated_mask"],) == want, (ttl, cap)
        assert m["delivered"][0] == 0 and m["first_hop"][0] == 0


def test_anchor_c_dead_ids():
    rows = _rows("c")
    assert len(rows) == 1024 and not any(rows[i][0] for i in (3, 20, 37))
    cases = [(3, 100, 5), (100, 20, 5), (37, 3, 5), (100, 200, 5)]
    m = P.reference_rows(rows, cases)
    assert [m[k] for k in P.CENSUS[:4]] == [963, 4256, 3842, 414]
    assert (m["cases_live"], m["live_mask"]) == (1, 0b1000)
    assert not any(m[k][:3].any() for k in P.ARRAYS) and m["relays"][3] > 0
