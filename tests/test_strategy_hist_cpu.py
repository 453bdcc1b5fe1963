"""CPU checks of psim_get_strategy_histograms' boundary: the struct layout of
the ctypes mirror against the header, where the entry point is declared, the
NIF table, and the numpy reference (tests/_strategy_stats.py, the yardstick
of tests/test_gpu_strategy_hist.py) on a hand-made overlay whose statistics
are worked out by hand below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _strategy_stats as R
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
NIF = os.path.join(ROOT, "erlang", "c_src", "partisan_gpu_sim_nif.c")


def test_struct_layout_matches_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%zu %%zu\\n", sizeof(psim_strategy_histograms),'
        'offsetof(psim_strategy_histograms, view_sum), offsetof(psim_strategy_histograms, agreeing));'
        'return 0;}\n' % HDR)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    m = _abi.PsimStrategyHistograms
    assert got == [C.sizeof(m), m.view_sum.offset, m.agreeing.offset]
    assert _abi.HIST_BINS == R.HIST_BINS
    names = [n for n, _ in m._fields_ if n != "reserved"]
    assert sorted(names) == sorted(R.HISTS + R.SCALARS)


def test_entry_point_is_gpu_only():
    assert "get_strategy_histograms" in _abi.GPU_ONLY
    assert "get_strategy_histograms" not in _abi.SIGNATURES
    assert re.search(r"\bpsim_get_strategy_histograms\s*\(", open(HDR).read())
    assert _abi.PSIM_ABI_VERSION == 12


def test_nif_table_has_strategy_histograms():
    table = {(n, int(a)) for n, a in re.findall(r'\{"(\w+)",\s*(\d+),\s*nif_\w+', open(NIF).read())}
    assert ("strategy_histograms", 1) in table
    erl = open(os.path.join(ROOT, "erlang", "src", "partisan_gpu_sim.erl")).read()
    assert re.search(r"^strategy_histograms\(_Sim\)\s*->\s*erlang:nif_error", erl, re.M)
    assert "strategy_histograms/1" in erl


def _views(rows):
    """rows: per node (up, view, in_view)"""
    v = np.zeros(len(rows), _abi.STRATEGY_VIEW_DTYPE)
    for i, (up, view, inv) in enumerate(rows):
        v["up"][i] = up
        v["view_n"][i], v["in_n"][i] = len(view), len(inv)
        v["view"][i][: len(view)] = view
        v["in_view"][i][: len(inv)] = inv
    return v


# 7 nodes: 4 is down, 5 is isolated (its view holds only itself), 0 <-> 1 is
# the mutual pair, 0 holds itself, 2 holds 3 twice, 3 -> 4 points at the
# down node; 6 -> 0 is one-way.  Live links: 0->1, 1->0, 2->3, 2->0, 3->2 is
# absent (3 holds only 4), 6->0.
HAND = [
    (1, [0, 1], [1, 6, 2]),      # view: self + 1; in_view: 1, 6, 2 (all hold 0)
    (1, [0], [0, 3]),            # in_view: 0 holds 1 (confirmed), 3 does not
    (1, [3, 0, 3], []),          # 3 twice
    (1, [4], [2, 4]),            # dangling link; in_view: 2 (confirmed), 4 is down
    (0, [0, 1, 2], [0]),         # down: nothing of it counts
    (1, [5], [5]),               # isolated, self only; in_view holds only itself
    (1, [0], []),
]


def _hist(pairs):
    h = np.zeros(R.HIST_BINS, np.uint64)
    for k, c in pairs:
        h[k] = c
    return h


def test_reference_on_a_hand_made_overlay():
    got = R.reference(_views(HAND), R.STRATEGY_SCAMP_V2)
    want = {
        "n_up": 6,
        "view_fill": _hist([(1, 4), (2, 1), (3, 1)]),      # lengths 2, 1, 3, 1, 1, 1
        "in_fill": _hist([(0, 2), (1, 1), (2, 2), (3, 1)]),  # lengths 3, 2, 0, 2, 1, 0
        "out_degree": _hist([(0, 1), (1, 4), (2, 1)]),     # 1, 1, 2, 1, 0, 1
        "in_degree": _hist([(0, 3), (1, 2), (3, 1)]),      # node 0: 3 (1, 2, 6); 1: 1; 2: 0; 3: 1; 5: 0; 6: 0
        "view_sum": 9, "in_sum": 8, "view_max": 3, "in_degree_max": 3,
        "links": 5,                  # 0->1, 1->0, 2->3, 2->0, 6->0
        "mutual_links": 2,           # 0->1 and 1->0
        "dangling_links": 1,         # 3->4
        "self_entries": 2,           # nodes 0 and 5
        "duplicate_entries": 1,      # the second 3 in node 2's view
        "in_view_links": 6,          # (0,1) (0,6) (0,2) (1,0) (1,3) (3,2)
        "in_view_confirmed": 5,      # all but (1,3): 3 does not hold 1
        "components": 2,             # {0, 1, 2, 3, 6} and {5}
        "largest_component": 5,
        "isolated": 1,               # node 5
        "members_min": 0, "members_max": 0, "members_sum": 0, "agreeing": 0,
    }
    R.compare(got, want)
    # the same rows as a v1 handle: the in_view fields stay zero
    v1 = R.reference(_views(HAND), R.STRATEGY_SCAMP_V1)
    want1 = dict(want, in_fill=_hist([]), in_sum=0, in_view_links=0, in_view_confirmed=0)
    R.compare(v1, want1)


def test_reference_saturating_bin_and_full():
    # node 0 holds 70 others: the last bin; each of them has in-degree 1
    rows = [(1, list(range(71)), [])] + [(1, [i], []) for i in range(1, 71)]
    got = R.reference(_views(rows), R.STRATEGY_SCAMP_V1)
    assert got["view_fill"][63] == 1 and got["out_degree"][63] == 1 and got["view_max"] == 71
    assert got["links"] == 70 and got["in_degree"][1] == 70 and got["components"] == 1
    # full: nodes 0, 1 agree on {0, 1, 2}; node 2 knows itself only; node 3 is down
    v = _views([(1, [], []), (1, [], []), (1, [], []), (0, [], [])])
    bits = [np.array([7], np.uint32), np.array([7], np.uint32), np.array([4], np.uint32), np.array([15], np.uint32)]
    got = R.reference(v, R.STRATEGY_FULL, bits)
    assert (got["n_up"], got["members_min"], got["members_max"], got["members_sum"], got["agreeing"]) == (3, 1, 3, 7, 2)
    assert got["links"] == 0 and got["components"] == 0 and not got["view_fill"].any()
