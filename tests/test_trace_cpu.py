"""CPU checks of the message trace's boundary (psim_trace_watch /
psim_trace_read / psim_trace_clear): where the entry points and constants are
declared and how the ctypes mirror binds them, and the reference of
tests/test_gpu_trace.py (tests/_trace.py: the filter and the capacity rule)
on the oracle's config A.

The oracle has no trace entry point (its inbox getter is the reference), so
the three signatures are bound with the GPU library's other own symbols
(_abi.GPU_ONLY) and not in _abi.SIGNATURES, which the oracle binds too."""
import os
import re

import numpy as np
import pytest

import _scenarios as S
import _trace as T
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "partisan_gpu_sim.h")


def _decl(name):
    """the argument list of a function declared in the header"""
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, open(HDR).read())
    assert m, f"{name} is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_trace_calls():
    assert len(_decl("psim_trace_watch")) == 6
    assert len(_decl("psim_trace_read")) == 6
    assert len(_decl("psim_trace_clear")) == 1
    text = open(HDR).read()
    assert re.search(r"#define\s+PSIM_TRACE_TO\s+1u\b", text)
    assert re.search(r"#define\s+PSIM_TRACE_FROM\s+2u\b", text)


def test_abi_binds_the_trace_calls():
    for name in ("trace_watch", "trace_read", "trace_clear"):
        assert name in _abi.GPU_ONLY and name not in _abi.SIGNATURES
        res, args = _abi.GPU_ONLY[name]
        assert res is not None and len(args) == len(_decl("psim_" + name))
    assert (_abi.PSIM_TRACE_TO, _abi.PSIM_TRACE_FROM) == (1, 2)


def test_abi_version_is_still_12():
    assert _abi.PSIM_ABI_VERSION == 12
    assert re.search(r"#define\s+PSIM_ABI_VERSION\s+12\b", open(HDR).read())


@pytest.fixture(scope="module")
def tape_a():
    sim, _ = S.config_a(T.TapedOracle)
    tape = sim.tape
    sim.close()
    return tape


def test_watch_all_is_the_concatenated_inboxes(tape_a):
    recs, rounds, lost = T.Reference(32).feed(tape_a).read()
    assert lost == 0 and len(recs) == sum(len(x) for _, x in tape_a) > 0
    assert np.array_equal(recs, np.concatenate([x for _, x in tape_a]))
    assert np.array_equal(rounds, np.concatenate([np.full(len(x), r, np.uint32) for r, x in tape_a]))
    # ascending (round, dst, src, seq), and (dst, src, seq) names a record of a round
    key = np.stack([rounds, recs[:, 0], recs[:, 1], recs[:, 3]], 1).astype(np.int64)
    order = np.lexsort((key[:, 3], key[:, 2], key[:, 1], key[:, 0]))
    assert np.array_equal(order, np.arange(len(key)))
    assert len(np.unique(key, axis=0)) == len(key)


def test_both_directions_are_the_union_of_each(tape_a):
    nodes = [0, 5, 31]
    both, rb, _ = T.Reference(32, nodes).feed(tape_a).read()
    to, rt, _ = T.Reference(32, nodes, frm=False).feed(tape_a).read()
    frm, rf, _ = T.Reference(32, nodes, to=False).feed(tape_a).read()
    assert 0 < len(to) < len(both) and 0 < len(frm) < len(both)
    assert np.isin(to[:, 0], nodes).all() and np.isin(frm[:, 1], nodes).all()
    rows = np.concatenate([np.column_stack([rt, to]), np.column_stack([rf, frm])])
    union = np.unique(rows, axis=0)
    assert len(union) < len(rows)                     # (a record between two watched nodes is in both)
    k = np.lexsort((union[:, 4], union[:, 2], union[:, 1], union[:, 0]))
    assert np.array_equal(union[k], np.column_stack([rb, both]))


def test_type_mask_filters_by_type(tape_a):
    mask = T.mask_of([7, 9])                          # SHUFFLE, PT_BROADCAST
    recs, _, _ = T.Reference(32, type_mask=mask).feed(tape_a).read()
    every, _, _ = T.Reference(32).feed(tape_a).read()
    assert set(np.unique(recs[:, 2] & 0xFF)) == {7, 9}
    assert np.array_equal(recs, every[np.isin(every[:, 2] & 0xFF, [7, 9])])


def test_truncation_keeps_a_prefix(tape_a):
    every, rounds, _ = T.Reference(32).feed(tape_a).read()
    ref = T.Reference(32, capacity=100).feed(tape_a)
    recs, rr, lost = ref.read()
    assert np.array_equal(recs, every[:100]) and np.array_equal(rr, rounds[:100])
    assert lost == len(every) - 100
    # a read empties the buffer: the capacity is free again from the next round on
    half = tape_a[len(tape_a) // 2][0]
    ref.feed(tape_a, last=half)
    a, ra, la = ref.read()
    ref.feed(tape_a, first=half)
    b, rb_, lb = ref.read()
    assert np.array_equal(a, every[:100]) and (rb_ >= half).all() and len(b) == 100
    assert np.array_equal(b, every[rounds >= half][:100])
    assert la + lb + 200 == len(every)
