"""CPU checks of psim_get_tree_metrics' boundary: the struct layout of the
ctypes mirror against the header, where the entry point is declared, and the
reference (tests/_tree_metrics.py, the yardstick of
tests/test_gpu_tree_metrics.py) on hand-built rows whose numbers are worked
out below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import _tree_metrics as R
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")
M = R.MAP_BIT


def test_struct_layout_matches_header(tmp_path):
    m = _abi.PsimTreeMetrics
    names = [n for n, _ in m._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
        'int main(){printf("%%zu %%d %%d %%u %%d\\n", sizeof(psim_tree_metrics), PSIM_HIST_BINS,\n'
        'PSIM_GRAPH_MAX_LEVELS, PSIM_MAP_BIT, PSIM_PT_ROOTS);\n'
        '%s return 0;}\n'
        % (HDR, "".join('printf("%%zu\\n", offsetof(psim_tree_metrics, %s));\n' % n for n in names)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:5] == [C.sizeof(m), R.HIST_BINS, R.MAX_LEVELS, R.MAP_BIT, R.ROOTS]
    assert got[5:] == [getattr(m, n).offset for n in names]
    assert (R.MAX_LEVELS, R.HIST_BINS) == (_abi.GRAPH_MAX_LEVELS, _abi.HIST_BINS)
    assert sorted(n for n in names if n != "reserved") == sorted(R.SCALARS + R.ARRAYS)
    assert all(t in (C.c_uint64, C.c_uint64 * 64, C.c_uint64 * 8) for _, t in m._fields_)
    assert names[-1] == "reserved" and m.reserved.size == 8 * 8
    assert set(R.DEGREE_FIELDS) <= set(names)


def test_entry_point_is_gpu_only():
    assert "get_tree_metrics" in _abi.GPU_ONLY
    assert "get_tree_metrics" not in _abi.SIGNATURES
    assert re.search(r"\bint\s+psim_get_tree_metrics\s*\(psim_handle \*h, uint32_t root, uint32_t max_levels,\s*"
                     r"psim_tree_metrics \*out\);", open(HDR).read())
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", open(HDR).read())


def _want(**kw):
    """every field zero but those given; a histogram as [(bin, count)]"""
    out = {k: 0 for k in R.SCALARS}
    for k in R.ARRAYS:
        out[k] = np.zeros(R.HIST_BINS, np.uint64)
    for k, v in kw.items():
        assert k in out, k
        if k in R.ARRAYS:
            for b, c in v:
                out[k][b] = c
        else:
            out[k] = v
    return out


def _chain(n):
    """node i holds a slot for root 0 with the one eager entry i + 1 (map
    form); the active views are the chain's two neighbours"""
    return [R.node(act=[j for j in (i - 1, i + 1) if 0 <= j < n],
                   slots=[(0, [M | (i + 1)] if i + 1 < n else [], [])]) for i in range(n)]


def test_chain():
    """0 -> 1 -> 2 -> 3: a tree, depth = overlay distance for every node"""
    got = R.reference_rows(_chain(4), 0)
    R.compare(got, _want(
        n_up=4, root_live=1, slot_nodes=4, eager_entries=3, eager_links=3,
        eager_out=[(0, 1), (1, 3)], lazy_out=[(0, 4)], eager_in=[(0, 1), (1, 3)],
        depth=[(1, 1), (2, 1), (3, 1)], depth_sum=6, depth_max=3, reached=3, unreached=0, links_from_reached=3,
        levels=4,                           # levels 1..3 find a node each, level 4 none
        overlay_reached=3, both_reached=3, depth_sum_both=6, dist_sum_both=6))


def test_star_with_one_redundant_link():
    """0 -> 1, 2, 3, the redundant 1 -> 2, and 2 -> 0 back to the root: five
    links deliver to three nodes; all entries in atom form"""
    rows = [R.node(act=[1, 2, 3], slots=[(0, [1, 2, 3], [])]), R.node(act=[0], slots=[(0, [2], [])]),
            R.node(act=[0], slots=[(0, [0], [])]), R.node(act=[0], slots=[(0, [], [])])]
    got = R.reference_rows(rows, 0)
    R.compare(got, _want(
        n_up=4, root_live=1, slot_nodes=4, eager_entries=5, eager_links=5,
        eager_nonmember=1,                  # 1 -> 2: 2 is not in 1's active view
        eager_symmetric=2,                  # (0, 2) and (2, 0)
        eager_out=[(0, 1), (1, 2), (3, 1)], lazy_out=[(0, 4)],
        eager_in=[(1, 3), (2, 1)],          # 0: from 2; 1, 3: from 0; 2: from 0 and 1
        depth=[(1, 3)], depth_sum=3, depth_max=1, reached=3, links_from_reached=5, levels=2,
        overlay_reached=3, both_reached=3, depth_sum_both=3, dist_sum_both=3))
    # the redundancy estimate links_from_reached / reached - 1: two spare copies over three nodes
    assert (got["links_from_reached"] - got["reached"], got["reached"]) == (2, 3)


def test_peer_in_both_forms_is_one_link():
    rows = [R.node(act=[1], slots=[(0, [1, M | 1], [])]), R.node(act=[0], slots=[(0, [], [])])]
    R.compare(R.reference_rows(rows, 0), _want(
        n_up=2, root_live=1, slot_nodes=2, eager_entries=2, eager_links=1, eager_both_forms=1,
        eager_out=[(0, 1), (1, 1)], lazy_out=[(0, 2)], eager_in=[(0, 1), (1, 1)],
        depth=[(1, 1)], depth_sum=1, depth_max=1, reached=1, links_from_reached=1, levels=2,
        overlay_reached=1, both_reached=1, depth_sum_both=1, dist_sum_both=1))


def test_map_form_lazy_atom_form_eager():
    """the PRUNE moved 1's map identity to the lazy set; the atom stays eager"""
    rows = [R.node(act=[1], slots=[(0, [1], [M | 1])]), R.node(act=[0], slots=[(0, [], [])])]
    R.compare(R.reference_rows(rows, 0), _want(
        n_up=2, root_live=1, slot_nodes=2, eager_entries=1, lazy_entries=1, eager_links=1, lazy_links=1,
        both_links=1, eager_out=[(0, 1), (1, 1)], lazy_out=[(0, 1), (1, 1)], eager_in=[(0, 1), (1, 1)],
        depth=[(1, 1)], depth_sum=1, depth_max=1, reached=1, links_from_reached=1, levels=2,
        overlay_reached=1, both_reached=1, depth_sum_both=1, dist_sum_both=1))


def test_node_without_a_slot_answers_from_common():
    """node 1 holds a slot for root 2 only (ignored) and answers root 0 with
    its common set; node 2 has neither"""
    rows = [R.node(act=[1], slots=[(0, [M | 1], [])]),
            R.node(act=[0, 2], common=[2], slots=[(2, [0], [0])]),
            R.node(act=[1])]
    R.compare(R.reference_rows(rows, 0), _want(
        n_up=3, root_live=1, slot_nodes=1, eager_entries=2, eager_links=2,
        eager_out=[(0, 1), (1, 2)], lazy_out=[(0, 3)], eager_in=[(0, 1), (1, 2)],
        depth=[(1, 1), (2, 1)], depth_sum=3, depth_max=2, reached=2, links_from_reached=2, levels=3,
        overlay_reached=2, both_reached=2, depth_sum_both=3, dist_sum_both=3))
    # root 2: node 1's slot (eager 0, lazy 0), nodes 0 and 2 from common ([] and [])
    R.compare(R.reference_rows(rows, 2), _want(
        n_up=3, root_live=1, slot_nodes=1, eager_entries=1, lazy_entries=1, eager_links=1, lazy_links=1,
        both_links=1, eager_out=[(0, 2), (1, 1)], lazy_out=[(0, 2), (1, 1)], eager_in=[(0, 2), (1, 1)],
        unreached=2, levels=1,              # level 1 finds nothing: node 2 has no eager entry
        overlay_reached=2))


DEAD = [R.node(act=[1, 2], common=[1], slots=[(0, [1, M | 2], [2])]),
        R.node(act=[0], slots=[(0, [0, 1], [])]),
        R.node(up=False, act=[0, 1], common=[0], slots=[(0, [0, 1], [1])])]


def test_dead_peer():
    """node 2 is down: 0's eager map entry and lazy entry for it are dead
    entries, its own row counts for nothing; node 1 holds itself"""
    R.compare(R.reference_rows(DEAD, 0), _want(
        n_up=2, root_live=1, slot_nodes=2, eager_entries=4, lazy_entries=1, eager_links=2, eager_symmetric=2,
        self_entries=1, eager_dead=1, lazy_dead=1,
        eager_out=[(1, 2)], lazy_out=[(0, 2)], eager_in=[(1, 2)],
        depth=[(1, 1)], depth_sum=1, depth_max=1, reached=1, links_from_reached=2, levels=2,
        overlay_reached=1, both_reached=1, depth_sum_both=1, dist_sum_both=1))


def test_dead_root():
    """root 2 is down: nobody holds a slot for it, the common sets answer (0:
    [1], 1: []), and every BFS field stays zero"""
    R.compare(R.reference_rows(DEAD, 2), _want(
        n_up=2, root_live=0, eager_entries=1, eager_links=1,
        eager_out=[(0, 1), (1, 1)], lazy_out=[(0, 2)], eager_in=[(0, 1), (1, 1)]))


def test_reachable_in_the_overlay_but_not_in_the_tree():
    """2 is 0's neighbour in L, but no eager entry names it: only a graft reaches it"""
    rows = [R.node(act=[1, 2], slots=[(0, [1], [])]), R.node(act=[0], slots=[(0, [], [])]),
            R.node(act=[0], slots=[(0, [0], [])])]
    R.compare(R.reference_rows(rows, 0), _want(
        n_up=3, root_live=1, slot_nodes=3, eager_entries=2, eager_links=2,
        eager_out=[(0, 1), (1, 2)], lazy_out=[(0, 3)], eager_in=[(0, 1), (1, 2)],
        depth=[(1, 1)], depth_sum=1, depth_max=1, reached=1, unreached=1, links_from_reached=1, levels=2,
        overlay_reached=2, both_reached=1, depth_sum_both=1, dist_sum_both=1))


def test_deeper_and_shallower():
    """L is the chain 0 - 1 - 2; T is 0 -> 2 -> 1 through the non-member 2"""
    rows = [R.node(act=[1], slots=[(0, [2], [])]), R.node(act=[0, 2], slots=[(0, [], [])]),
            R.node(act=[1], slots=[(0, [M | 1], [])])]
    R.compare(R.reference_rows(rows, 0), _want(
        n_up=3, root_live=1, slot_nodes=3, eager_entries=2, eager_links=2, eager_nonmember=1,
        eager_out=[(0, 1), (1, 2)], lazy_out=[(0, 3)], eager_in=[(0, 1), (1, 2)],
        depth=[(1, 1), (2, 1)], depth_sum=3, depth_max=2, reached=2, links_from_reached=2, levels=3,
        overlay_reached=2, both_reached=2, depth_sum_both=3, dist_sum_both=3,
        deeper=1,                           # 1: depth 2, distance 1
        shallower=1))                       # 2: depth 1, distance 2


def test_level_cap():
    rows = _chain(6)
    R.compare(R.reference_rows(rows, 0, max_levels=2), _want(
        n_up=6, root_live=1, slot_nodes=6, eager_entries=5, eager_links=5,
        eager_out=[(0, 1), (1, 5)], lazy_out=[(0, 6)], eager_in=[(0, 1), (1, 5)],
        depth=[(1, 1), (2, 1)], depth_sum=3, depth_max=2, reached=2,
        unreached=3,                        # depths 3, 4, 5 lie past the cap
        links_from_reached=3, levels=2, truncated=1,
        overlay_reached=2, both_reached=2, depth_sum_both=3, dist_sum_both=3))
    full = R.reference_rows(rows, 0)
    assert (full["levels"], full["truncated"], full["depth_max"], full["unreached"]) == (6, 0, 5, 0)
    # level 5 = the cap still finds node 5: truncated, though nothing lies beyond
    at = R.reference_rows(rows, 0, max_levels=5)
    assert (at["levels"], at["truncated"], at["reached"]) == (5, 1, 5)
    # a cap the BFS never meets: as without one; a cap past the largest: clamped
    R.compare(R.reference_rows(rows, 0, 6), full)
    R.compare(R.reference_rows(rows, 0, 10**6), full)


def test_depth_bins_saturate():
    got = R.reference_rows(_chain(70), 0)
    assert got["depth"][62] == 1 and got["depth"][63] == 7 and got["depth"][0] == 0
    assert got["depth_sum"] == 69 * 70 // 2 and got["depth_max"] == 69 and got["levels"] == 70


def test_reference_reads_node_views():
    """the same rows as psim_node_view records: slot runs pooled in slot order"""
    rows = [R.node(act=[1, 2], common=[1], slots=[(7, [3], []), (0, [1, M | 2, M | 1], [2])]),
            R.node(act=[0], slots=[(0, [0], [M | 0])]), R.node(act=[0], common=[0, 1])]
    v = np.zeros(len(rows), _abi.NODE_VIEW_DTYPE)
    v["pt_root"][:] = 0xFFFFFFFF
    for i, r in enumerate(rows):
        v["up"][i], v["act_n"][i], v["pt_common_n"][i] = r["up"], len(r["act"]), len(r["common"])
        v["act"][i][: len(r["act"])] = r["act"]
        v["pt_common"][i][: len(r["common"])] = r["common"]
        eo = zo = 0
        for k, (root, e, z) in enumerate(r["slots"]):
            v["pt_root"][i][k], v["pt_eager_n"][i][k], v["pt_lazy_n"][i][k] = root, len(e), len(z)
            v["pt_eager"][i][eo: eo + len(e)] = e
            v["pt_lazy"][i][zo: zo + len(z)] = z
            eo, zo = eo + len(e), zo + len(z)
    want = R.reference_rows(rows, 0)
    assert want["eager_both_forms"] == 1 and want["both_links"] == 2 and want["slot_nodes"] == 2
    R.compare(R.reference(v, 0), want)
    try:
        R.compare(dict(want, both_links=3), want)
    except AssertionError as e:
        assert "both_links: 3 != 2" in str(e)
    else:
        raise AssertionError("compare accepted a differing field")
