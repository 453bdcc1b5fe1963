"""Which branch outcomes of oracle/psim_oracle.c does no parity run take?

Every GPU test compares the engine with the oracle, so a handler outcome the
oracle never enters in those runs is one on which the kernels have never been
compared with anything.  This tool (test-only, CPU) finds them:

  * it compiles the oracle with `gcc -O0 --coverage` into a temporary
    directory (nothing is written into oracle/; liborc.so is left alone) and
    lets tests/_oracle.py load that build (PSIM_ORACLE_LIB);
  * it runs every entry of the registry (tests/_parity_registry.py: the oracle
    side of the scenarios the GPU parity files use) in a child process of its
    own, each writing its counters into its own directory (GCOV_PREFIX);
  * it reduces `gcov -b -c --json-format` to records
        (function, normalized source text of the line, n-th condition on it,
         outcome) -> count
    keyed by function and text, never by line number, so that unrelated edits
    do not move them.

Which side of a condition is missing: gcov lists the two outcomes of a
two-way branch by destination block, and at -O0 the blocks stand in source
order, so the first one is the outcome that goes to the earlier code.  An
`&&` / `||` chain is one such branch a leaf, left to right; where a leaf goes
on true and on false follows from the short-circuit rules (`leaves` below
parses the condition: `!` swaps the two targets).  A record's outcome `T` /
`F` therefore says whether the leaf *as written*, without its `!`, came out
true or false (a loop's test: T goes round again).  Where the leaf count of a
line does not match gcov's branch count (a switch, a `?:` inside a call) the
outcomes are numbered instead: `case0`, `case1`, ...
tests/test_oracle_coverage.py checks the rule on a program whose counts are
known.

    python -m tests._oracle_coverage              never-taken outcomes of the registry
    python -m tests._oracle_coverage --diff       ... against tests/golden/oracle_unreached.json
    python -m tests._oracle_coverage --run NAME   the outcomes only run NAME takes
    python -m tests._oracle_coverage --list       the registry's run names
"""
import argparse
import collections
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SRC = os.path.join(ROOT, "oracle", "psim_oracle.c")
LEDGER = os.path.join(HERE, "golden", "oracle_unreached.json")
CLASSES = ("refusal", "alloc", "impossible", "unreachable-by-protocol")
STEM = "psim_oracle"


def tools_missing():
    return [t for t in ("gcc", "gcov") if shutil.which(t) is None]


# ---------------------------------------------------------------- the build
def build(tmp, src=SRC, stem=STEM, shared=True):
    """the instrumented build of `src` in `tmp`; returns the library (or program)"""
    obj = os.path.join(tmp, stem + ".o")
    out = os.path.join(tmp, stem + (".so" if shared else ""))
    flags = ["-O0", "--coverage", "-std=c11"]
    subprocess.check_call(["gcc", *flags, "-fPIC", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", obj], cwd=tmp)
    subprocess.check_call(["gcc", "--coverage", *(["-shared"] if shared else []), obj, "-o", out, "-lm"], cwd=tmp)
    return out


def child_env(lib, outdir):
    env = dict(os.environ, GCOV_PREFIX=outdir, GCOV_PREFIX_STRIP="64")
    if lib:
        env["PSIM_ORACLE_LIB"] = lib
    return env


# ---------------------------------------------------------------- the source side
def _strip(lines):
    """source lines without comments, strings and char literals"""
    out, in_c = [], False
    for ln in lines:
        s, i = "", 0
        while i < len(ln):
            if in_c:
                j = ln.find("*/", i)
                if j < 0:
                    i = len(ln)
                else:
                    in_c, i = False, j + 2
            elif ln.startswith("/*", i):
                in_c, i = True, i + 2
            elif ln.startswith("//", i):
                break
            elif ln[i] in "\"'":
                q, i = ln[i], i + 1
                while i < len(ln) and ln[i] != q:
                    i += 2 if ln[i] == "\\" else 1
                i += 1
                s += "0"
            else:
                s += ln[i]
                i += 1
        out.append(s)
    return out


# The order of a condition's two outcomes in gcov's list: gcov sorts a block's
# arcs by destination block, and at -O0 the blocks stand in source order, so
# the outcome listed first is the one whose control goes to the *earlier*
# code.  Where a leaf goes on true and on false follows from the short-circuit
# rules: the next leaf of the chain, the guarded statement (which follows the
# condition -- in a loop it precedes it: the test stands below the body), or
# whatever comes after the statement.
_THEN, _ELSE, _BODY = 1 << 40, (1 << 40) + 1, -1


def _tokens(text, pos0):
    """(kind, text, position) with kind in `( ) ! && || x`"""
    out, i = [], 0
    while i < len(text):
        ch = text[i]
        if ch.isspace():
            i += 1
        elif text[i:i + 2] in ("&&", "||"):
            out.append((text[i:i + 2], text[i:i + 2], pos0 + i))
            i += 2
        elif ch == "!" and text[i:i + 2] != "!=":
            out.append(("!", "!", pos0 + i))
            i += 1
        elif ch in "()":
            out.append((ch, ch, pos0 + i))
            i += 1
        else:
            j = i
            while j < len(text) and not text[j].isspace() and text[j] not in "()" \
                    and text[j:j + 2] not in ("&&", "||") \
                    and not (text[j] == "!" and text[j:j + 2] != "!=" and j > i):
                j += 1
            out.append(("x", text[i:j], pos0 + i))
            i = j
    return out


class _Parse:
    """or := and ('||' and)*; and := not ('&&' not)*; not := '!' not | primary;
    primary := a run of tokens with balanced parentheses.  A parenthesized
    group that holds a chain is a node; any other run is one leaf."""

    def __init__(self, toks):
        self.t, self.i = toks, 0

    def peek(self):
        return self.t[self.i][0] if self.i < len(self.t) else None

    def p_or(self):
        n = self.p_and()
        while self.peek() == "||":
            self.i += 1
            n = ("or", n, self.p_and())
        return n

    def p_and(self):
        n = self.p_not()
        while self.peek() == "&&":
            self.i += 1
            n = ("and", n, self.p_not())
        return n

    def _chain_inside(self, i):
        """does the group opening at token i hold a top-level-of-group && / ||, and is
        it followed by an operator or the end (a whole operand)?"""
        d, j, chain = 0, i, False
        while j < len(self.t):
            k = self.t[j][0]
            d += k == "("
            d -= k == ")"
            if d == 1 and k in ("&&", "||"):
                chain = True
            if d == 0:
                break
            j += 1
        nxt = self.t[j + 1][0] if j + 1 < len(self.t) else None
        return chain and nxt in (None, "&&", "||", ")"), j

    def p_not(self):
        if self.peek() == "!":
            self.i += 1
            return ("not", self.p_not())
        if self.peek() == "(":
            chain, close = self._chain_inside(self.i)
            if chain:
                self.i += 1
                n = self.p_or()
                assert self.peek() == ")"
                self.i += 1
                return n
        # a leaf: tokens up to the next && / || / unbalanced ) at depth 0
        d, start = 0, self.i
        while self.i < len(self.t):
            k = self.t[self.i][0]
            if d == 0 and k in ("&&", "||", ")"):
                break
            d += k == "("
            d -= k == ")"
            self.i += 1
        assert self.i > start
        last = self.t[self.i - 1]
        return ("leaf", self.t[start][2], last[2] + len(last[1]))


def _first(n):
    while n[0] != "leaf":
        n = n[1]
    return n[1]


def _targets(n, t, f, out):
    if n[0] == "leaf":
        out.append((n[1], n[2], t, f))
    elif n[0] == "not":
        _targets(n[1], f, t, out)
    elif n[0] == "and":
        _targets(n[1], _first(n[2]), f, out)
        _targets(n[2], t, f, out)
    else:
        _targets(n[1], t, _first(n[2]), out)
        _targets(n[2], t, f, out)


def _match(text, i):
    """index of the parenthesis closing the one at i"""
    d = 0
    for j in range(i, len(text)):
        d += text[j] == "("
        d -= text[j] == ")"
        if d == 0:
            return j
    return -1


def _top_split(text, ch):
    d, out, last = 0, [], 0
    for j, c in enumerate(text):
        d += c in "(["
        d -= c in ")]"
        if d == 0 and c == ch:
            out.append((last, j))
            last = j + 1
    out.append((last, len(text)))
    return out


def leaves(code_lines):
    """per line: [(leaf text, true_first)] for the conditions' leaves that begin
    on it, in order; true_first: gcov lists the leaf's true outcome first."""
    text = "\n".join(code_lines)
    line_at, ln = [], 0
    for c in text:
        line_at.append(ln)
        ln += c == "\n"
    sites = []                                    # (start, end, loop, a value: return / assignment)
    for m in re.finditer(r"\b(if|while|for)\s*\(", text):
        o = m.end() - 1
        c = _match(text, o)
        if c < 0:
            continue
        if m.group(1) == "for":
            parts = _top_split(text[o + 1:c], ";")
            if len(parts) == 3:
                sites.append((o + 1 + parts[1][0], o + 1 + parts[1][1], True, False))
        else:
            sites.append((o + 1, c, m.group(1) == "while", False))
    for m in re.finditer(r"(\breturn\b|[^=!<>]=(?!=))([^;{}]*);", text):
        sites.append((m.start(2), m.end(2), False, True))
    covered, found = [], []
    for a, b, loop, value in sorted(sites):
        if any(x <= a and b <= y for x, y in covered):
            continue                              # (an assignment inside a for clause or a condition)
        covered.append((a, b))
        body = text[a:b]
        q = _top_split(body, "?")
        if len(q) > 1:                            # cond ? x : y -- the condition alone
            b = a + q[0][1]
            body = text[a:b]
        if not re.search(r"\w", body):
            continue
        if value and len(q) == 1 and not re.search(r"&&|\|\|", body):
            continue                              # a plain value: no branch
        try:
            tree = _Parse(_tokens(body, a)).p_or()
        except (AssertionError, IndexError):
            continue
        out = []
        _targets(tree, _BODY if loop else _THEN, _ELSE, out)
        for pos, end, t, f in out:
            # a loop's test stands below its body: on a line that holds both
            # (for (..) if (..) ..;) gcov lists the body's conditions first
            found.append((line_at[pos], loop, pos, text[pos:end], t < f))
    res = [[] for _ in code_lines]
    for ln, _, pos, leaf, tf in sorted(found):
        res[ln].append((norm(leaf), tf))
    return res


def norm(text):
    return re.sub(r"\s+", " ", text).strip()


# ---------------------------------------------------------------- the gcov side
def gcov_json(objdir, src=SRC, stem=STEM):
    """gcov's JSON for the counters in `objdir` (needs the .gcno beside them)"""
    cmd = ["gcov", "-b", "-c", "--json-format", "--stdout", "-o", objdir, os.path.join(objdir, stem + ".o")]
    r = subprocess.run(cmd, cwd=objdir, capture_output=True, text=True, check=True)
    data = json.loads(r.stdout)
    for f in data["files"]:
        if os.path.basename(f["file"]) == os.path.basename(src):
            return f
    raise RuntimeError("gcov reported nothing for " + src)


def records(gfile, src=SRC):
    """{key: count} with key = "function | line text | condition k | outcome";
    a text that occurs twice in one function gets " #2", ... in order"""
    with open(src) as f:
        raw = f.read().split("\n")
    code = _strip(raw)
    lv = leaves(code)
    out, seen = collections.OrderedDict(), collections.Counter()
    with_br = {ln["line_number"] for ln in gfile["lines"] if ln["branches"]}
    for ln in sorted(gfile["lines"], key=lambda x: x["line_number"]):
        br = [b for b in ln["branches"] if not b["throw"]]
        if not br:
            continue
        no = ln["line_number"] - 1
        text = norm(code[no])
        fn = ln.get("function_name") or "?"
        seen[(fn, text)] += 1
        if seen[(fn, text)] > 1:
            text += f" #{seen[(fn, text)]}"
        lf, nxt = list(lv[no]), no + 1
        # a value spread over lines (return a || b ||\n c): gcov counts it on one line
        while len(br) > 2 * len(lf) and nxt < len(lv) and nxt + 1 not in with_br and nxt < no + 4:
            lf += lv[nxt]
            nxt += 1
        if len(br) == 2 * len(lf):
            for k, (leaf, true_first) in enumerate(lf):
                t, f_ = br[2 * k]["count"], br[2 * k + 1]["count"]
                if not true_first:
                    t, f_ = f_, t
                out[f"{fn} | {text} | {k}: {leaf} | T"] = t
                out[f"{fn} | {text} | {k}: {leaf} | F"] = f_
                LINES[f"{fn} | {text} | {k}: {leaf} | T"] = LINES[f"{fn} | {text} | {k}: {leaf} | F"] = no + 1
        else:
            for k, b in enumerate(br):
                out[f"{fn} | {text} | - | case{k}"] = b["count"]
                LINES[f"{fn} | {text} | - | case{k}"] = no + 1
    return out


LINES = {}                 # record -> its current line number (for reading; no part of the key)


def line_of(key):
    return LINES.get(key, 0)


# ---------------------------------------------------------------- the runs
def _child(name):
    import _parity_registry as P
    from _oracle import Oracle
    P.runs()[name](Oracle)


def run_one(lib, tmp, name):
    """run one registry entry in a child; returns (name, records, seconds)"""
    d = os.path.join(tmp, "run_" + re.sub(r"\W", "_", name))
    os.makedirs(d, exist_ok=True)
    shutil.copy(os.path.join(tmp, STEM + ".gcno"), d)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=child_env(lib, d),
                       capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError(f"run {name} failed:\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    dt = time.time() - t0
    rec = records(gcov_json(d))
    shutil.rmtree(d, ignore_errors=True)
    return name, rec, dt


def run_registry(names=None, jobs=None, tmp=None):
    """{run name: records} of the named runs (default: all)"""
    import _parity_registry as P
    names = list(P.runs()) if names is None else list(names)
    own = tmp is None
    tmp = tmp or tempfile.mkdtemp(prefix="orc_cov_")
    try:
        lib = build(tmp)
        jobs = jobs or min(8, os.cpu_count() or 1)
        out, times = {}, {}
        with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
            for name, rec, dt in ex.map(lambda n: run_one(lib, tmp, n), names):
                out[name], times[name] = rec, dt
        return out, times
    finally:
        if own:
            shutil.rmtree(tmp, ignore_errors=True)


def total(per_run):
    tot = collections.OrderedDict()
    for rec in per_run.values():
        for k, v in rec.items():
            tot[k] = tot.get(k, 0) + v
    return tot


def never_taken(tot):
    return [k for k, v in tot.items() if v == 0]


def load_ledger():
    with open(LEDGER) as f:
        return json.load(f)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--run", help="show the outcomes only this run takes")
    ap.add_argument("--diff", action="store_true", help="compare with the ledger")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--times", action="store_true", help="print each run's wall time")
    ap.add_argument("--jobs", type=int)
    a = ap.parse_args(argv)
    if a.child:
        _child(a.child)
        return 0
    import _parity_registry as P
    if a.list:
        print("\n".join(P.runs()))
        return 0
    miss = tools_missing()
    if miss:
        print("missing: " + ", ".join(miss))
        return 2
    t0 = time.time()
    per_run, times = run_registry(jobs=a.jobs)
    tot = total(per_run)
    if a.times:
        for n, dt in sorted(times.items(), key=lambda x: -x[1]):
            print(f"{dt:7.1f} s  {n}")
    if a.run:
        others = total({k: v for k, v in per_run.items() if k != a.run})
        only = [k for k, v in per_run[a.run].items() if v and not others.get(k)]
        print(f"{a.run}: {len(only)} outcomes no other run takes")
        for k in only:
            print(f"  {per_run[a.run][k]:>9}  :{line_of(k)}  {k}")
        return 0
    nt = never_taken(tot)
    print(f"{len(tot)} outcomes, {len(nt)} never taken by {len(per_run)} runs ({time.time() - t0:.0f} s)")
    if a.diff:
        led = {e["key"]: e for e in load_ledger()["entries"]}
        for k in nt:
            if k not in led:
                print(f"  not in the ledger  :{line_of(k)}  {k}")
        for k in led:
            if tot.get(k, 0) > 0:
                print(f"  ledgered but taken {tot[k]} times  {k}")
            elif k not in tot:
                print(f"  ledgered but no such outcome  {k}")
        return 0
    for k in nt:
        print(f"  :{line_of(k)}  {k}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
