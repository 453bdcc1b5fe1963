"""What no parity run reaches: the branch outcomes of
oracle/psim_oracle.c that the registry of parity runs (tests/_parity_registry.py)
never takes are exactly the ledger tests/golden/oracle_unreached.json, every
entry of which is classed and argued; and each scenario written for a rare
outcome (tests/test_gpu_rare_branches.py runs them GPU == oracle) takes it.
CPU only: the oracle is built with gcc -O0 --coverage in a temporary
directory (tests/_oracle_coverage.py)."""
import os
import re
import subprocess
import tempfile

import pytest

import _oracle_coverage as T
import _parity_registry as P

pytestmark = pytest.mark.skipif(bool(T.tools_missing()),
                                reason="needs " + " and ".join(T.tools_missing()) + " on the PATH")


@pytest.fixture(scope="module")
def coverage():
    per_run, _ = T.run_registry()
    return per_run, T.total(per_run)


@pytest.fixture(scope="module")
def ledger():
    return T.load_ledger()["entries"]


def test_every_never_taken_outcome_is_in_the_ledger(coverage, ledger):
    _, tot = coverage
    known = {e["key"] for e in ledger}
    missing = [f":{T.line_of(k)}  {k}" for k in T.never_taken(tot) if k not in known]
    assert not missing, "never taken and not in the ledger:\n" + "\n".join(missing)


def test_the_ledger_holds_no_outcome_a_run_takes(coverage, ledger):
    _, tot = coverage
    gone = [e["key"] for e in ledger if e["key"] not in tot]
    assert not gone, "no such outcome (the source line changed?):\n" + "\n".join(gone)
    taken = [f"{tot[e['key']]} times  {e['key']}" for e in ledger if tot[e["key"]] > 0]
    assert not taken, "in the ledger but taken:\n" + "\n".join(taken)
    assert len({e["key"] for e in ledger}) == len(ledger)


def test_every_entry_is_classed_and_argued(ledger):
    # a citation: a line of the oracle, a clause of the reference (module:line),
    # a section of DESIGN.md, or a file of the tests
    cite = re.compile(r"line \d+|lines \d+|[a-z_0-9]+(\.erl)?:\d+|DESIGN\.md section \d|tests/\w+")
    for e in ledger:
        assert e["class"] in T.CLASSES, e
        assert len(e["reason"].split()) >= 6, e
        if e["class"] in ("impossible", "unreachable-by-protocol"):
            assert cite.search(e["reason"]), f"no citation: {e}"


@pytest.mark.parametrize("name", list(P.RARE))
def test_rare_scenario_takes_its_outcome(coverage, name):
    per_run, _ = coverage
    rec = per_run["rare:" + name]
    assert P.RARE_TARGETS[name]
    for key in P.RARE_TARGETS[name]:
        assert key in rec, f"no such outcome: {key}"
        print(f"{name}: {rec[key]:>8}  {key}")
        assert rec[key] > 0, key


def test_rare_targets_are_taken_by_no_older_run(coverage):
    """each target was never taken before its scenario existed: no run outside
    tests/test_gpu_rare_branches.py takes it -- of the runs that are older
    than the scenarios.  The id-window runs (tests/test_gpu_high_ids.py,
    `high-ids...`) came later and are other overlays: one of them takes the
    GRAFT for a message the receiver does not hold."""
    per_run, _ = coverage
    assert any(k.startswith("high-ids") for k in per_run)
    others = T.total({k: v for k, v in per_run.items() if not k.startswith(("rare:", "high-ids"))})
    for name, keys in P.RARE_TARGETS.items():
        for key in keys:
            assert others.get(key, 0) == 0, (name, key)


SAMPLE = r"""
#include <stdio.h>
static int id(int x) { return x; }
static int f(int a, int b, int c) {
    int r = 0;
    if (!id(a) || !(b || id(c) || a == 9)) r += 1;
    if (!id(a) && b) r += 4;
    while (b < 0 && a < 0) b++;
    return r;
}
static int g(int a, int b, int c) {
    return !(a == 1 || b >= 2 || !id(c) ||
             c != 3);
}
static int h(const int *v, int n, int x) {
    for (int i = 0; i < n; i++) if (v[i] == x || v[i] < 0) return i;
    return -1;
}
int main(void) {
    int v[4] = {1, 2, 3, -1};
    int s = f(1, 1, 0) + f(1, 1, 0) + f(1, 0, 1) + f(0, 0, 0);
    s += g(1, 0, 0) + g(0, 2, 0) + g(0, 0, 0) + g(2, 0, 3) + g(2, 0, 4);
    s += h(v, 4, 3) + h(v, 4, 9) + h(v, 2, 9);
    printf("%d\n", s);
    return 0;
}
"""
# (function, leaf) -> (times true, times false), counted by hand from main's calls
EXPECT = {
    ("f", "id(a)"): (3, 1), ("f", "b"): (2, 1), ("f", "id(c)"): (1, 0), ("f", "a == 9"): (0, 0),
    ("f", "id(a) #2"): (3, 1), ("f", "b #2"): (0, 1),
    ("f", "b < 0"): (0, 4), ("f", "a < 0"): (0, 0),
    ("g", "a == 1"): (1, 4), ("g", "b >= 2"): (1, 3), ("g", "id(c)"): (2, 1), ("g", "c != 3"): (1, 1),
    ("h", "v[i] == x"): (1, 8), ("h", "v[i] < 0"): (1, 7), ("h", "i < n"): (9, 1),
}


def test_the_tool_resolves_which_side_was_taken():
    """the outcome names (T / F of the leaf as written) against a program
    whose counts are known: `!` on a leaf and on a group, `&&` inside `||`,
    a loop's test, a value spread over two lines, a loop with its body's
    condition on one line"""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sample.c")
        with open(src, "w") as f:
            f.write(SAMPLE)
        exe = T.build(tmp, src=src, stem="sample", shared=False)
        subprocess.run([exe], check=True, capture_output=True)
        rec = T.records(T.gcov_json(tmp, src=src, stem="sample"), src=src)
    got, seen = {}, {}
    for key, count in rec.items():
        fn, _, leaf, out = key.split(" | ")
        assert out in ("T", "F"), key               # every condition of the sample is resolved
        leaf = leaf.split(": ", 1)[1]
        if out == "T":
            seen[(fn, leaf)] = seen.get((fn, leaf), 0) + 1
        tag = leaf if seen[(fn, leaf)] == 1 else f"{leaf} #{seen[(fn, leaf)]}"
        t, f_ = got.get((fn, tag), (0, 0))
        got[(fn, tag)] = (count, f_) if out == "T" else (t, count)
    assert got == EXPECT
