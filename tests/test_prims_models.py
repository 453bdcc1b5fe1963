"""CPU checks behind tests/test_gpu_prims.py: the pinned Philox tie triples,
the plain models against hand-worked cases and against each other, the test
module's honesty about testing the product's text, and its launchers' domain
checks (which return before any HIP call, so they run without a GPU)."""
import json
import os
import re

import numpy as np
import pytest

import _prims as P

HERE = os.path.dirname(os.path.abspath(__file__))
TIES = json.load(open(os.path.join(HERE, "golden", "philox_ties.json")))


def test_tie_triples_are_ties_in_o1_only():
    """every pinned (node, c, d): the second Philox words of counters c and
    c + d are equal, the full 53-bit keys differ, and no other pair that a
    30-counter window around them can hold ties"""
    seed, win = TIES["seed"], TIES["window"]
    assert win == 30 and len(TIES["triples"]) >= 6
    for t in TIES["triples"]:
        node, c, d = t["node"], t["c"], t["d"]
        assert 0 < d < win
        lo = max(0, c + d - (win - 1))
        w = {x: P.philox(x & 0xFFFFFFFF, x >> 32, node, 0, seed & 0xFFFFFFFF, seed >> 32) for x in range(lo, c + win)}
        assert w[c][1] == w[c + d][1] == t["o1"]
        key = {x: P.draw58(x, node, seed) >> 5 for x in w}
        assert all(key[x] >> 21 == w[x][1] for x in w)         # the rank's 32 bits are o1
        assert key[c] != key[c + d]
        ties = [(a, b) for a in w for b in w if a < b < a + win and w[a][1] == w[b][1]]
        assert ties == [(c, c + d)]
    ds = sorted(t["d"] for t in TIES["triples"])
    assert ds[0] <= 7 and ds[-1] >= 22                          # spread over the window


def test_uniform_model_boundaries():
    T = P.TWO58
    # v < n: v + 1, whatever the range test would say
    assert P.uniform([0], 7) == (1, 1)
    assert P.uniform([6], 7) == (7, 1)
    # v >= n: i = v rem n, accepted iff v - i <= 2^58 - n
    assert P.uniform([7], 7) == (1, 1)
    assert P.uniform([23], 7) == (3, 1)
    # n = 7: 2^58 rem 7 = 2, so the last whole block of 7 is 2^58 - 9 .. 2^58 - 3
    # and the two values above it redraw
    assert T % 7 == 2
    assert P.uniform([T - 9], 7) == (1, 1)                      # v - i = 2^58 - 9 <= 2^58 - 7
    assert P.uniform([T - 3], 7) == (7, 1)
    assert P.uniform([T - 2, 3], 7) == (4, 2)                   # v - i = 2^58 - 2 > 2^58 - 7
    assert P.uniform([T - 1, T - 2, T - 1, 9], 7) == (3, 4)
    # a power of two never redraws: 2^58 - n is itself a block start
    assert P.uniform([T - 1], 64) == (64, 1)
    assert P.uniform([T - 64], 64) == (1, 1)
    # n = 30: 2^58 rem 30 = 4; v = 2^58 - 4 is the first redraw
    assert T % 30 == 4
    assert P.uniform([T - 5], 30) == (30, 1)
    assert P.uniform([T - 4, 29], 30) == (30, 2)
    assert P.uniform([T - 4, 30], 30) == (1, 2)
    # n = 1 takes any draw but the very last
    assert P.uniform([12345], 1) == (1, 1)
    assert P.uniform([T - 1], 1) == (1, 1)                      # v - 0 <= 2^58 - 1


def test_sublist_model_orders_by_key_then_element():
    V = [50, 40, 30, 20]
    # keys are draw >> 5: draws 0..31 all key 0 -- the element decides
    assert P.sublist(V, 4, 3, [31, 0, 17, 5]) == [20, 30, 40]
    assert P.sublist(V, 4, 9, [32, 0, 64, 33]) == [40, 20, 50, 30]
    assert P.sublist(V, 3, 2, [0, 0, 0, 0]) == [30, 40]
    assert P.sublist(V, 0, 2, []) == [] and P.sublist(V, 4, 0, [1, 2, 3, 4]) == []


def test_list_models():
    assert P.usort([5, 3, 5, 1, 3]) == [1, 3, 5] and P.usort([]) == []
    assert P.list_ins([1, 2, 3], 0, 9) == [9, 1, 2, 3] and P.list_ins([1, 2, 3], 3, 9) == [1, 2, 3, 9]
    assert P.list_del([1, 2, 3], 0) == [2, 3] and P.list_del([1, 2, 3], 2) == [1, 2]
    tab = np.array([0, 3, 3, 1, 3 + 16, 0, 15], np.uint8)
    b = P.bucket_of(tab)
    assert [b(e) for e in range(7)] == [0, 3, 3, 1, 3, 0, 15]
    assert P.make_view([1, 3, 2, 6, 4, 5], b) == [5, 3, 1, 2, 4, 6]     # equal buckets: oldest first
    assert P.pas_step([5, 3, 1], 3, None, b) == ([5, 3, 1], 0)
    assert P.pas_step([5, 3, 1], 2, 0, b) == ([3, 1, 2], 1)
    assert P.pas_step([5, 3, 1], 0, 2, b) == ([5, 0, 3], 1)


@pytest.mark.parametrize("seed", range(3))
def test_view_add_is_sets_v1_order_up_to_80(seed):
    """view_add on a 16-slot table is OtpSetsV1.add_element's to_list order
    while the set has its first 16 slots (<= 80 elements)"""
    rng = np.random.Generator(np.random.PCG64([seed, 0x9815]))
    tab = rng.integers(0, 256, 4096, dtype=np.uint8)
    ids = [int(e) for e in rng.permutation(4096)[:80]]
    s, V, b = P.otp_set(tab), [], P.bucket_of(tab)
    for e in ids:
        s.add_element(e)
        V = P.view_add(V, e, b)
        assert s.n == 16 and V == s.to_list()
    for e in ids[:40]:
        assert P.set_slot(tab, e, 16) == b(e)


def test_merge_model_by_hand():
    tab = np.arange(64, dtype=np.uint8)               # bucket = id & 15
    b = P.bucket_of(tab)
    D = P.Draws(1, 23, 32, base=100, vals=[7, P.TWO58 - 1, 5] + [0] * 29)
    # maxp 3, full view [16, 1, 2]; candidates usort([9, 2, 40, 1, 3]) - A {40} - me 9 = [1, 2, 3]:
    # 1, 2 members; 3 evicts index 7 rem 3 = 1 (-> [16, 2]) and goes in after bucket 2
    assert P.merge_exchange(D, 100, 9, [40], [16, 1, 2], [9, 2, 40, 1, 3], 3, b) == ([16, 2, 3], 101, 1)
    # a rejected draw (2^58 - 1 at counter 101) costs one more: 5 rem 3 = 2
    assert P.merge_exchange(D, 101, 9, [], [16, 1, 2], [3], 3, b) == ([16, 1, 3], 103, 1)
    # below the bound nothing is drawn; the insert that fills the view makes the next one evict
    assert P.merge_exchange(D, 100, 9, [], [16, 1], [0], 3, b) == ([16, 0, 1], 100, 1)
    assert P.merge_exchange(D, 100, 9, [], [16, 1], [3, 0], 3, b) == ([16, 1, 3], 101, 1)


def test_module_sources_define_no_device_function():
    """the test module calls the product's device functions and has none of
    its own: only __global__ kernels and host launchers"""
    d = os.path.join(HERE, "prims")
    srcs = [f for f in sorted(os.listdir(d)) if f.endswith((".hip", ".h", ".cpp"))]
    assert "prims_consume.hip" in srcs and "prims_strategy.hip" in srcs
    for f in srcs:
        text = open(os.path.join(d, f)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"\bDEV\b", code), f
        assert not re.search(r"__device__|__forceinline__|__host__", code), f
        assert not re.search(r"#\s*include\s*\"[^\"]*\.hip\"", code) or f.endswith(".hip")
    inc = re.findall(r"#\s*include\s*\"([^\"]+)\"", open(os.path.join(d, "prims_consume.hip")).read())
    assert inc[0] == "psim_consume.hip"
    inc = re.findall(r"#\s*include\s*\"([^\"]+)\"", open(os.path.join(d, "prims_strategy.hip")).read())
    assert inc[0] == "psim_strategy.hip"


def test_loader_names_the_make_target(monkeypatch, tmp_path):
    monkeypatch.setattr(P, "_lib", None)
    monkeypatch.setattr(P, "LIB_PATH", str(tmp_path / "libpsim_prims_test.so"))
    with pytest.raises(RuntimeError, match="make -C partisan_amd/csrc prims"):
        P.load()


def test_launchers_refuse_cases_outside_the_domain():
    """a wrong parameter comes back as a domain error before anything is
    launched (no GPU is touched: this runs anywhere the module is built)"""
    c = P.cfg()
    z = [0] * 64

    def refused(name, row, words, *pre, groups=1, cfg=c, post=()):
        with pytest.raises(P.DomainError):
            P.run_rows(name, cfg, [row], words, *pre, groups=groups, post=post)

    refused("list32", [0, 64, 0, 1] + z, P.L32_OUT)                    # vins into 64 entries
    refused("list32", [0, 3, 4, 1] + z, P.L32_OUT)                     # pos > n
    refused("list32", [1, 3, 3, 0] + z, P.L32_OUT)                     # k >= n
    refused("list32", [1, 0, 0, 0] + z, P.L32_OUT)                     # delete from nothing
    refused("list32", [4, 2, 0, 0] + [1, 2, 3] + z[3:], P.L32_OUT)     # an entry past the count
    tab = np.zeros(16, np.uint8)
    refused("list32", [3, 1, 0, 16] + [1] + z[1:], P.L32_OUT, cfg=P.cfg(table=tab))   # id past the table
    refused("list64", [0, 64, 0, 1, 1] + z + z, P.L64_OUT)
    refused("mod", [0, 0, 65, 0], 1)
    refused("mod", [0, 0, 0, 0], 1)
    refused("mod", [0, 1 << 26, 5, 0], 1)
    refused("mod", [0, 0, 65536, 1], 1)
    refused("set_slot", [5, 15], 1)
    refused("wv_uniform", P.rc_row(p=[65]), P.RC_OUT)
    refused("wv_uniform", P.rc_row(p=[0]), P.RC_OUT)
    refused("lite_uniform", P.rc_row(p=[32]), P.RC_OUT, 32, groups=2)
    refused("lite_uniform", P.rc_row(p=[5]), P.RC_OUT, 24, groups=2)   # no such width
    refused("lite_select", P.rc_row(p=[17]), P.RC_OUT, 16, groups=4)
    refused("wv_sublist", P.rc_row(p=[65, 1, 0]), P.RC_OUT)
    refused("wv_sublist", P.rc_row(p=[64, 40, 30]), P.RC_OUT)          # on + m past the scratch
    refused("lite_sublist", P.rc_row(p=[9, 1, 0]), P.RC_OUT, 16, 8, groups=4)
    refused("lite_sublist", P.rc_row(p=[9, 1, 0]), P.RC_OUT, 16, 30, groups=4)   # <30, 16> does not exist
    refused("lite_sublist", P.rc_row(p=[31, 1, 0]), P.RC_OUT, 32, 30, groups=2)
    refused("pas_sublist", P.rc_row(p=[31, 1, 0]), P.RC_OUT, 16, groups=4)
    refused("pas_sublist", P.rc_row(p=[30, 1, 9]), P.RC_OUT, 16, groups=4)
    refused("lite_merge", P.rc_row(p=[0, 31, 1, 0]), P.RC_OUT, 32, groups=2)     # pas_n > max_passive
    refused("lite_merge", P.rc_row(p=[0, 0, 9, 0]), P.RC_OUT, 32, groups=2)      # nex > 8
    refused("lite_merge", P.rc_row(p=[0, 0, 2, 1], r2=[5, 5]), P.RC_OUT, 32, groups=2)   # "sorted" with a repeat
    refused("lite_merge", P.rc_row(p=[0, 0, 1, 0], r2=[1 << 27]), P.RC_OUT, 16, groups=4)
    refused("wv_merge", P.rc_row(p=[9, 0, 0]), P.RC_OUT)
    refused("wv_merge", P.rc_row(p=[0, 0, 1]), P.RC_OUT, cfg=P.cfg(max_passive=31))
    refused("wv_uniform", P.rc_row(p=[5], dc=[1 << 58]), P.RC_OUT)     # no 58-bit draw
    refused("lite_usort", P.rc_row(p=[0x100]), P.RC_OUT, 32, groups=2)
    refused("lite_usort", P.rc_row(p=[1], r0=[P.NONE]), P.RC_OUT, 16, groups=4)
    # Pas<W>::step: a plain insert into 30 entries, an eviction at n
    b = P.bucket_of(None)
    full = P.make_view(range(1, 31), b)
    steps = lambda *s: [x for e, k in s for x in (e, P.NONE if k is None else k)] + [0, P.NONE] * (64 - len(s))
    refused("pas_step", [30] + full + [0, 0] + steps((99, None)), P.PS_NSTEP * P.PS_SOUT, 32, groups=2, post=(1,))
    refused("pas_step", [30] + full + [0, 0] + steps((99, 30)), P.PS_NSTEP * P.PS_SOUT, 16, groups=4, post=(1,))
    refused("pas_step", [31] + full + [31, 0] + steps(), P.PS_NSTEP * P.PS_SOUT, 16, groups=4, post=(0,))
    refused("pas_step", [0] + [0] * 32 + steps((1 << 27, None)), P.PS_NSTEP * P.PS_SOUT, 32, groups=2, post=(1,))
    refused("l2", [0, 128, 0, 1] + z + z, P.L2_OUT)
    refused("l2", [0, 5, 6, 1] + z + z, P.L2_OUT)
    refused("l2", [2, 5, 128, 0] + z + z, P.L2_OUT)
    refused("set2", [2, 7, 7] + [0] * (P.S2_MAXOPS - 2), P.S2_MAXOPS * P.S2_SOUT)        # add of a member
    refused("set2", [P.S2_MAXOPS + 1] + [0] * P.S2_MAXOPS, P.S2_MAXOPS * P.S2_SOUT)
    refused("pw_uniform", P.rc_row(p=[65536]), P.RC_OUT)
    refused("pw_sublist", P.rc_row(p=[129, 1]), P.RC_OUT)
    refused("pw_sublist", P.rc_row(p=[100, 65]), P.RC_OUT)
    with pytest.raises(P.DomainError):
        P.call("modstep", c, 2, 1, 32, P._ptr(np.zeros(640, np.uint32)))             # Grp<W>::magic: n <= 31
    with pytest.raises(P.DomainError):
        P.call("modstep", c, 0, 0, 64, P._ptr(np.zeros(640, np.uint32)))
