"""The device primitives one by one against plain models (tests/_prims.py), at
the branches no scenario reaches: the sublists' exact recount after a tie in
the top 32 key bits (on real Philox counters that tie,
golden/philox_ties.json, and on injected draws), the ?uniform_range redraw and
merge_exchange's sequential fallback, the exact small modulo with its
multiplier fetched every way the product fetches it, the lane-shift list
operations at the ends of their registers, and device Philox itself.

The kernels are tests/prims/*.hip, which include the product's text; every
comparison is exact.  A launcher refuses a case outside its primitive's domain
(tests/test_prims_models.py), which raises here: no case is filtered."""
import json
import os
import random

import numpy as np
import pytest

import _prims as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T58 = P.TWO58
M32 = 0xFFFFFFFF
SEED = 23
TIES = json.load(open(os.path.join(HERE, "golden", "philox_ties.json")))
assert TIES["seed"] == SEED


def pad(v, n=64):
    return list(v) + [0] * (n - len(v))


def ids_distinct(r, n, hi=1 << 27, lo=1):
    out = set()
    while len(out) < n:
        out.add(r.randrange(lo, hi))
    out = list(out)
    r.shuffle(out)
    return out


# ------------------------------------------------------------------ Philox --
def test_philox_known_answers():
    kat = json.load(open(os.path.join(HERE, "golden", "philox4x32_10_kat.json")))["vectors"]
    out = P.run_rows("philox", P.cfg(), [v["ctr"] + v["key"] for v in kat], 2)
    assert len(kat) >= 3
    for v, o in zip(kat, out):
        assert [int(o[0]), int(o[1])] == v["out"][:2]


def test_draw58_at_random_counters():
    r = random.Random(581)
    rows, want = [], []
    for i in range(1 << 16):
        ctr = r.getrandbits(64) if i & 1 else r.getrandbits(30)
        seed = r.getrandbits(64) if i & 2 else r.getrandbits(31)
        node = r.getrandbits(32) if i & 4 else r.getrandbits(20)
        rows.append([ctr & M32, ctr >> 32, node, seed & M32, seed >> 32])
        want.append(P.draw58(ctr, node, seed))
    out = P.run_rows("draw58", P.cfg(), rows, 2)
    got = [int(o[0]) | (int(o[1]) << 32) for o in out]
    assert got == want
    assert max(want) < T58 and max(want) > T58 // 2


# ------------------------------------------------------------------ modulo --
@pytest.mark.parametrize("mode,hi,cover", [(0, 64, 1), (1, 64, 1), (2, 31, 2), (3, 31, 4)],
                         ids=["kMagic", "readlane", "Grp32", "Grp16"])
def test_mod_step_exhaustive(mode, hi, cover):
    """one Horner step against the compiler's % for every x < n 2^20, the
    multiplier fetched the product's way (`cover` lane groups sweep each n)"""
    res = np.zeros(640, np.uint32)
    P.call("modstep", P.cfg(), mode, 1, hi, P._ptr(res))
    r64 = res[128:].view(np.uint64)
    for n in range(1, hi + 1):
        assert int(res[n]) == (0 if n == 1 else -((-1 << 32) // n)), n
        assert int(r64[2 * n]) == 0, (n, int(r64[2 * n]))
        assert int(r64[2 * n + 1]) == (0 if n == 1 else cover * (n << 20)), n


def _mod_values(r, n):
    vs = {0, n - 1, n, (1 << 20) - 1, 1 << 20, (1 << 40) - 1, 1 << 40}
    vs.update(range(T58 - n - 1, T58))
    return sorted(vs) + [r.getrandbits(58) for _ in range(1 << 14)]


def test_mod_small_whole_function():
    r = random.Random(64)
    rows = [[v & M32, v >> 32, n, 0] for n in range(1, 65) for v in _mod_values(r, n)]
    out = P.run_rows("mod", P.cfg(), rows, 1)
    bad = [(x[0] | (x[1] << 32), x[2], int(o[0])) for x, o in zip(rows, out) if (x[0] | (x[1] << 32)) % x[2] != int(o[0])]
    assert bad == []


def test_mod58_whole_function():
    r = random.Random(58)
    rows = [[v & M32, v >> 32, n, 1] for n in (65, 66, 255, 256, 257, 32767, 32768, 65521, 65534, 65535)
            for v in _mod_values(r, n)]
    out = P.run_rows("mod", P.cfg(), rows, 1)
    bad = [(x[0] | (x[1] << 32), x[2], int(o[0])) for x, o in zip(rows, out) if (x[0] | (x[1] << 32)) % x[2] != int(o[0])]
    assert bad == []


# ---------------------------------------------------------------- wave_min --
def test_wave_min():
    r = random.Random(63)
    special = [0, 1, (1 << 31) - 1, 1 << 31, M32]
    rows = []
    for l in range(64):                                   # the minimum at every lane in turn
        for lo in (0, 5, (1 << 31) + 5):
            v = [r.randrange(lo + 1, 1 << 32) for _ in range(64)]
            v[l] = lo
            rows.append(v)
        v = [M32] * 64                                    # ... below a wave of all-ones
        v[l] = M32 - 1
        rows.append(v)
    rows += [[s] * 64 for s in special]                   # all lanes equal
    for _ in range(64):
        rows.append([r.choice(special) for _ in range(64)])
        rows.append([r.choice(special[2:]) for _ in range(64)])
        rows.append([r.getrandbits(32) for _ in range(64)])
        v = [r.randrange(1 << 31, 1 << 32) for _ in range(64)]          # two equal minima
        a, b = r.sample(range(64), 2)
        v[a] = v[b] = min(v) - 1
        rows.append(v)
    out = P.run_rows("wave_min", P.cfg(), rows, 1)
    assert [int(o[0]) for o in out] == [min(v) for v in rows]


# ------------------------------------------------------- 32-bit wave lists --
INS_N = (0, 1, 2, 31, 32, 33, 62, 63)
DEL_N = (1, 2, 32, 63, 64)


def _vals32(r, n):
    v = ids_distinct(r, n, 1 << 32)
    if n:
        v[r.randrange(n)] = M32                           # >= 2^31, and the all-ones word
    return v


def test_list32_insert_delete_every_position():
    r = random.Random(32)
    rows, want = [], []
    for n in INS_N:
        for pos in range(n + 1):
            V, e = _vals32(r, n), r.randrange(1, 1 << 32)
            rows.append([0, n, pos, e] + pad(V))
            want.append((n + 1, pad(P.list_ins(V, pos, e))))
    for n in DEL_N:
        for k in range(n):
            V = _vals32(r, n)
            rows.append([1, n, k, 0] + pad(V))
            want.append((n - 1, pad(P.list_del(V, k))))
    out = P.run_rows("list32", P.cfg(), rows, P.L32_OUT)
    for row, o, (n, V) in zip(rows, out, want):
        assert (int(o[0]), [int(x) for x in o[2:]]) == (n, V), row[:4]


def test_list32_lookup_and_delete_by_value():
    r = random.Random(33)
    rows, want = [], []
    for n in (0,) + DEL_N:
        V = _vals32(r, n)
        probes = [(e, i) for i, e in enumerate(V) if i in (0, 1, 30, 31, 32, n - 2, n - 1)]
        probes += [(0, -1), (r.randrange(1, 1 << 32), -1)]             # 0 sits in every lane past the count
        if n >= 2:
            W = list(V)
            W[n - 1] = W[0]                                           # a repeat: the first index counts
            probes_w = [(W[0], 0)]
        else:
            W, probes_w = V, []
        for lst, pr in ((V, probes), (W, probes_w)):
            for e, i in pr:
                if e in lst:
                    i = lst.index(e)
                rows.append([4, n, 0, e] + pad(lst)); want.append((n, int(i >= 0), pad(lst)))
                rows.append([5, n, 0, e] + pad(lst)); want.append((n, i & M32, pad(lst)))
                rows.append([2, n, 0, e] + pad(lst))
                want.append((n - 1, 1, pad(P.list_del(lst, i))) if i >= 0 else (n, 0, pad(lst)))
    out = P.run_rows("list32", P.cfg(), rows, P.L32_OUT)
    for row, o, w in zip(rows, out, want):
        assert (int(o[0]), int(o[1]), [int(x) for x in o[2:]]) == w, row[:4]


@pytest.mark.parametrize("tabled", [False, True], ids=["default-hash", "table"])
def test_view_add(tabled):
    r = random.Random(34 + tabled)
    tab = None
    if tabled:
        tab = np.array([r.getrandbits(8) for _ in range(4096)], np.uint8)
        tab[1000:1200] = 0x35                             # a run of equal buckets
        tab[1200:1300] = 0xF0                             # bucket 0: goes in front
        tab[1300:1400] = 0x0F                             # bucket 15: goes to the end
    b = P.bucket_of(tab)
    rows, want = [], []
    for n in INS_N:
        for rep in range(6):
            lo, hi = (1000, 1400) if tabled and rep % 2 else (1, 4096 if tabled else 1 << 27)
            ids = ids_distinct(r, n + 1, hi, lo)
            if not tabled and rep == 0:
                ids[-1] = 0 if n % 2 else (1 << 27) - 1
            V = P.make_view(ids[:-1], b)
            rows.append([3, n, 0, ids[-1]] + pad(V))
            want.append((n + 1, pad(P.view_add(V, ids[-1], b))))
    out = P.run_rows("list32", P.cfg(table=tab), rows, P.L32_OUT)
    for row, o, (n, V) in zip(rows, out, want):
        assert (int(o[0]), [int(x) for x in o[2:]]) == (n, V), row[:4]


def test_list64_insert_delete_every_position():
    r = random.Random(64)
    v64 = lambda: (r.randrange(1, 1 << 32) << 32) | r.randrange(1, 1 << 32)
    split = lambda V: pad([v & M32 for v in V]) + pad([v >> 32 for v in V])
    rows, want = [], []
    for n in INS_N:
        for pos in range(n + 1):
            V, e = [v64() for _ in range(n)], v64()
            rows.append([0, n, pos, e & M32, e >> 32] + split(V))
            want.append((n + 1, split(P.list_ins(V, pos, e))))
    for n in DEL_N:
        for k in range(n):
            V = [v64() for _ in range(n)]
            rows.append([1, n, k, 0, 0] + split(V))
            want.append((n - 1, split(P.list_del(V, k))))
    out = P.run_rows("list64", P.cfg(), rows, P.L64_OUT)
    for row, o, (n, V) in zip(rows, out, want):
        assert (int(o[0]), [int(x) for x in o[2:]]) == (n, V), row[:5]


# ------------------------------------------------------------------- usort --
def _usort_patterns(r, m):
    """value lists of length m: random, all equal, sorted, reversed, repeats
    of the largest and of the smallest; values >= 2^31 among them"""
    base = sorted(ids_distinct(r, max(m, 1), M32, 0))[:m]           # (M32 itself is PSIM_NONE)
    if m:
        base[-1] = M32 - 1
    out = [list(base), list(reversed(base)), [base[0] if m else 0] * m]
    sh = list(base)
    r.shuffle(sh)
    out.append(sh)
    if m >= 3:
        hi, lo = list(sh), list(sh)
        for i in r.sample(range(m), 2):
            hi[i], lo[i] = max(sh), min(sh)
        out += [hi, lo]
    return out


def test_usort_wave():
    r = random.Random(70)
    rows, want = [], []
    for m in list(range(0, 10)) + [31, 32, 33, 63, 64]:
        for vals in _usort_patterns(r, m):
            rows.append(P.rc_row(p=[1, m], r0=pad(vals + [r.getrandbits(32) for _ in range(64 - m)])))
            want.append(P.usort(vals))
            lanes = sorted(r.sample(range(64), m))                     # a sparse mask
            E = [r.getrandbits(32) for _ in range(64)]
            for l, v in zip(lanes, vals):
                E[l] = v
            mask = sum(1 << l for l in lanes)
            rows.append(P.rc_row(p=[0, mask & M32, mask >> 32], r0=E))
            want.append(P.usort(vals))
    out = P.rc_run("wv_usort", P.cfg(), rows)
    for row, (s, arr), w in zip(rows, out, want):
        assert (s[0], arr) == (len(w), pad(w)), row[P.RC_P:P.RC_P + 3]


@pytest.mark.parametrize("width", [32, 16])
def test_usort_lite(width):
    r = random.Random(71 + width)
    rows, want = [], []
    for m in range(9):
        for vals in _usort_patterns(r, m):
            rows.append(P.rc_row(p=[(1 << m) - 1], r0=vals + [r.getrandbits(31) for _ in range(width - m)]))
            want.append(P.usort(vals))
    for _ in range(64):                                                # sparse valid lanes
        mask = r.getrandbits(8)
        E = [r.choice([3, 9, 1 << 31, r.getrandbits(31)]) for _ in range(8)]
        rows.append(P.rc_row(p=[mask], r0=E + [r.getrandbits(31) for _ in range(width - 8)]))
        want.append(P.usort([E[l] for l in range(8) if (mask >> l) & 1]))
    out = P.rc_run("lite_usort", P.cfg(), rows, width, groups=64 // width)
    for row, (s, arr), w in zip(rows, out, want):
        assert (s[0], arr[:width]) == (len(w), pad(w, width)), row[P.RC_P]


# ---------------------------------------------------------- Pas<W>::step --
def _step_rows(view, steps):
    row = [len(view)] + pad(view, 32)
    for e, k in steps:
        row += [e, P.NONE if k is None else k]
    return row + [0, P.NONE] * (P.PS_NSTEP - len(steps))


def _step_want(view, steps, bucket):
    out, dirty = [], 0
    for e, k in steps:
        view, ch = P.pas_step(view, e, k, bucket)
        dirty |= ch
        out.append((pad(view, 32), len(view), dirty))
    return out


def _step_check(width, c, cases, bucket, nstep):
    rows = [_step_rows(v, s) for v, s in cases]
    out = P.run_rows("pas_step", c, rows, P.PS_NSTEP * P.PS_SOUT, width, groups=64 // width, post=(nstep,))
    for ci, ((view, steps), o) in enumerate(zip(cases, out)):
        o = o.reshape(P.PS_NSTEP, P.PS_SOUT)
        for s, w in enumerate(_step_want(view, steps, bucket)):
            got = ([int(x) for x in o[s][:32]], int(o[s][32]), int(o[s][33]))
            assert got == w, (ci, s, steps[s], view)


def _random_chain(r, bucket, view, fresh):
    """64 steps from `view`: member no-ops, plain inserts while n <= 29,
    evictions at k = 0, n - 1 and anywhere"""
    steps, cur = [], list(view)
    for _ in range(P.PS_NSTEP):
        n, x = len(cur), r.random()
        if n and x < 0.15:
            step = (r.choice(cur), r.choice([None, 0, n - 1]))         # a member: no eviction happens
        elif n <= 29 and (n == 0 or x < 0.55):
            step = (fresh(), None)
        else:
            step = (fresh(), r.choice([0, n - 1, r.randrange(n)]))
        steps.append(step)
        cur, _ = P.pas_step(cur, step[0], step[1], bucket)
    return steps


@pytest.mark.parametrize("tabled", [False, True], ids=["default-hash", "table"])
@pytest.mark.parametrize("width", [32, 16])
def test_pas_step_chains(width, tabled):
    r = random.Random(width * 2 + tabled)
    tab = None
    if tabled:
        tab = np.array([i & 0xFF for i in range(1 << 14)], np.uint8)   # bucket = id & 15
        tab[8192:] = 0x77                                              # ... and 8192 ids of one bucket
    b = P.bucket_of(tab)
    top = (1 << 14) if tabled else (1 << 27)
    pool = iter(ids_distinct(r, 6000, top))
    fresh = lambda: next(pool)
    big = lambda n: P.make_view([top - 1 - i for i in range(n)], b)    # a view full of the largest ids
    cases = []
    for i in range(8):
        # neighbours in a wave: from an empty view, from a full one, and equal buckets
        cases.append(([], _random_chain(r, b, [], fresh)))
        v = big(30) if i % 2 else P.make_view([fresh() for _ in range(30)], b)
        cases.append((v, _random_chain(r, b, v, fresh)))
        if tabled:
            eq = lambda: r.randrange(8192, 1 << 14)
            cases.append(([], _random_chain(r, b, [], eq)))
        else:
            v = P.make_view([0, top - 1] + [fresh() for _ in range(10)], b)        # ids 0 and 2^27 - 1
            cases.append((v, _random_chain(r, b, v, fresh)))
    for n in range(1, 31):                                 # every k of every n, the insert anywhere
        v = big(n) if n % 3 == 0 else P.make_view([fresh() for _ in range(n)], b)
        steps, cur = [], list(v)
        for s in range(P.PS_NSTEP):
            step = (fresh(), s % n)
            steps.append(step)
            cur, _ = P.pas_step(cur, step[0], step[1], b)
        cases.append((v, steps))
    _step_check(width, P.cfg(table=tab), cases, b, P.PS_NSTEP)


@pytest.mark.parametrize("width", [32, 16])
def test_pas_step_ends(width):
    """the candidate at position 0 and at position n, k = 0 and k = n - 1
    with the insert at n - 1, for every n; every group's neighbour is an
    empty view or one full of the largest tags"""
    tab = np.array([i & 0xFF for i in range(1 << 15)], np.uint8)       # bucket = id & 15
    b = P.bucket_of(tab)
    idb = lambda bucket, j: 16 * (j + 1) + bucket                      # the j-th id of a bucket
    full15 = [idb(15, 200 + j) for j in range(30)]                     # 30 entries of the last bucket
    cases = []
    for n in range(0, 31):
        view = [idb(1 + (j * 14) // max(n, 1), j) for j in range(n)]   # buckets 1..14, ascending
        assert view == P.make_view(view, b)
        steps = []
        if n <= 29:
            steps += [[(idb(0, 99), None)], [(idb(15, 99), None)], [(idb(7, 99), None)]]
        if n >= 1:
            steps += [[(idb(0, 99), 0)], [(idb(15, 99), n - 1)], [(idb(15, 99), 0)], [(idb(0, 99), n - 1)],
                      [(view[n // 2], None)]]
            steps += [[(idb(b(view[n - 1]), 99), n - 1)]]              # the last entry's bucket: in at n - 1
        for s in steps:
            cases += [(view, s), ([], [(idb(3, 1), None)]), (view, s), (full15, [(idb(15, 999), 29)])]
    _step_check(width, P.cfg(table=tab), cases, b, 1)


# ------------------------------------------------------------- uniform_n --
FORMS = {"wv": ("wv_uniform", (), 1, 64), "lite32": ("lite_uniform", (32,), 2, 32),
         "lite16": ("lite_uniform", (16,), 4, 16), "pw": ("pw_uniform", (), 1, 64)}


def _uniform_cases(r, n, width):
    """(rng, cache base, cached draws) of rand:uniform(n)"""
    rej = T58 % n                                          # the top `rej` values redraw
    acc = [T58 - n - 1, T58 - n, T58 - rej - 1, n, n - 1, 0, r.randrange(n, T58 - n)]
    seqs = [[a] for a in acc]
    if rej:
        bad = [T58 - rej, T58 - 1, T58 - 1 - r.randrange(rej)]
        seqs += [bad[:i] + [a] for i in (1, 2, 3) for a in (T58 - rej - 1, 0, r.randrange(n, T58 - n))]
    out = []
    for s in seqs:
        base = r.getrandbits(40)
        fill = [r.getrandbits(58) for _ in range(width)]
        out.append((base, base, s + fill[len(s):]))                    # from the cache's first slot
        if len(s) <= 2:
            at = width - len(s)                                        # the accepted draw in the last slot
            out.append((base + at, base, fill[:at] + s))
    if rej:                                                # a rejected draw in the last slot: the
        for k in (1, 2):                                   # redraw refills from Philox
            base = r.getrandbits(40) + (1 << 32) * (k - 1)
            fill = [r.getrandbits(58) for _ in range(width)]
            out.append((base + width - k, base, fill[:width - k] + [T58 - 1] * k))
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_uniform_n(form):
    name, pre, groups, width = FORMS[form]
    r = random.Random(len(form) * 7 + width)
    ns = {"wv": (1, 2, 3, 7, 30, 31, 33, 63, 64), "pw": (1, 2, 3, 7, 30, 33, 63, 64, 65, 128, 65535)}.get(
        form, (1, 2, 3, 7, 15, 16, 17, 29, 30, 31))
    rows, want = [], []
    for n in ns:
        for rng, base, vals in _uniform_cases(r, n, width):
            me = r.randrange(1 << 20)
            rows.append(P.rc_row(me=me, rng=rng, dcb=base, dc=vals, p=[n]))
            want.append(P.uniform_at(P.Draws(me, SEED, width, base, vals), rng, n))
    assert any(w[1] - (rows[i][1] | rows[i][2] << 32) >= 4 for i, w in enumerate(want))   # three redraws in a row
    r.shuffle(order := list(range(len(rows))))             # the groups of a wave get unrelated cases
    out = P.rc_run(name, P.cfg(seed=SEED), [rows[i] for i in order], *pre, groups=groups)
    for i, (s, _) in zip(order, out):
        assert (s[0], P.rng_of(s)) == want[i], (rows[i][P.RC_P], rows[i][:5])


# ---------------------------------------------------------- select_random --
@pytest.mark.parametrize("form", ["wv", "lite32", "lite16"])
def test_select_random(form):
    name, pre, groups, width = {"wv": ("wv_select", (), 1, 64), "lite32": ("lite_select", (32,), 2, 32),
                                "lite16": ("lite_select", (16,), 4, 16)}[form]
    r = random.Random(90 + width)
    nmax = {"wv": 64, "lite32": 31, "lite16": 16}[form]
    nomit = 3 if form == "wv" else 2
    rows, want = [], []
    for n in sorted({0, 1, 2, 3, 8, nmax - 1, nmax}):
        V = ids_distinct(r, n, 1 << 27)
        omits = [[P.NONE] * nomit]
        if n:
            omits += [[V[0]] * nomit, [V[-1]] * nomit, [V[0], V[-1]] + [V[n // 2]] * (nomit - 2),
                      [V[-1], P.NONE] + [V[0]] * (nomit - 2)]
        if 1 <= n <= nomit:
            omits.append(pad(V, nomit)[:nomit] if n == nomit else V + [V[0]] * (nomit - n))   # nothing eligible
        for om in omits:
            elig = len([e for e in V if e not in om])
            for seq in ([r.randrange(64, T58 - 64)], [0], [max(elig, 1) - 1],
                        [T58 - 1, r.randrange(64, T58 - 64)]):
                me, rng = r.randrange(1 << 20), r.getrandbits(40)
                vals = seq + [r.getrandbits(58) for _ in range(width - len(seq))]
                rows.append(P.rc_row(me=me, rng=rng, dcb=rng, dc=vals, p=[n] + om, r0=V))
                want.append(P.select_random(P.Draws(me, SEED, width, rng, vals), rng, V, n, om))
    none = [i for i, w in enumerate(want) if w[0] == P.NONE]
    assert none and all(want[i][1] == rows[i][1] | rows[i][2] << 32 for i in none)    # nothing eligible: no draw
    r.shuffle(order := list(range(len(rows))))
    out = P.rc_run(name, P.cfg(seed=SEED), [rows[i] for i in order], *pre, groups=groups)
    for i, (s, _) in zip(order, out):
        assert (s[0], P.rng_of(s)) == want[i], rows[i][P.RC_P:P.RC_P + 4]


# ----------------------------------------------------------------- sublist --
# form -> launcher, its leading arguments, cases a wave, the OUT register's
# lanes, the cache's depth (None: Philox in place), the largest n
SUB = {
    "wv": ("wv_sublist", (), 1, 64, 64, 64),
    "lite<30,32>": ("lite_sublist", (32, 30), 2, 32, 32, 30),
    "lite<8,32>": ("lite_sublist", (32, 8), 2, 32, 32, 8),
    "lite<8,16>": ("lite_sublist", (16, 8), 4, 16, 16, 8),
    "Pas<32>": ("pas_sublist", (32,), 2, 32, 32, 30),
    "Pas<16>": ("pas_sublist", (16,), 4, 16, None, 30),
}


def _sub_check(form, cases):
    """cases: (me, rng, cache base or None, cached draws, V, n, k, on, OUT0)"""
    name, pre, groups, lanes, depth, _ = SUB[form]
    rows, want = [], []
    for me, rng, base, vals, V, n, k, on, OUT0 in cases:
        rows.append(P.rc_row(me=me, rng=rng, dcb=base, dc=vals or (), p=[n, k, on], r0=V, r2=OUT0))
        D = P.Draws(me, SEED, depth or 64, base, vals) if depth else P.Draws(me, SEED, 64)
        want.append(P.sublist_at(D, rng, V, n, k, pad(OUT0, lanes), on, lanes))
    out = P.rc_run(name, P.cfg(seed=SEED), rows, *pre, groups=groups)
    for row, (s, arr), w in zip(rows, out, want):
        assert (s[0], P.rng_of(s), arr[:lanes]) == w, (form, row[:5], row[P.RC_P:P.RC_P + 3])


def _tie_windows(nmax):
    """(node, base, n) with both tied counters in [base, base + n), n <= nmax"""
    out = []
    for t in TIES["triples"]:
        c, d = t["c"], t["d"]
        if d + 1 > nmax:
            continue
        out.append((t["node"], c, d + 1))                              # the pair at the window's ends
        lead = (nmax - d - 1) // 2
        if lead:
            out.append((t["node"], c - lead, nmax))                    # ... and inside a full one
    return out


@pytest.mark.parametrize("form", list(SUB))
def test_sublist_on_philox_ties(form):
    """real counters whose top 32 key bits tie: every k in 1..n puts the tied
    pair above, across and below the cut"""
    r = random.Random(len(form))
    nmax = SUB[form][5] if form != "wv" else 30
    wins = _tie_windows(nmax)
    assert len(wins) >= (3 if nmax == 8 else 12)
    cases = []
    for node, base, n in wins:
        V = ids_distinct(r, n, 1 << 27)
        for k in range(1, n + 1):
            for on in (0, 1, 3):
                cases.append((node, base, None, None, V, n, k, on, [r.getrandbits(27) for _ in range(SUB[form][3])]))
    r.shuffle(cases)
    _sub_check(form, cases)


def test_pw_sublist_on_philox_ties_and_past_64():
    """the pluggable wave's sublist has no tie branch: the same windows as a
    plain check, and lists in both registers"""
    r = random.Random(128)
    rows, want = [], []
    wins = _tie_windows(30) + [(5, 1000, 64), (6, (1 << 32) - 20, 65), (7, 77, 100), (8, 1 << 40, 128)]
    for node, base, n in wins:
        V = ids_distinct(r, n, 1 << 27)
        for k in sorted({1, 2, n // 2, n - 1, n, 64}):
            if k > 64:
                k = 64
            rows.append(P.rc_row(me=node, rng=base, p=[n, k], r0=V[:64], r1=V[64:]))
            keys = [P.draw58(base + i, node, SEED) for i in range(n)]
            got = P.sublist(V, n, k, keys)
            want.append((len(got), base + n, pad(got)))
    out = P.rc_run("pw_sublist", P.cfg(seed=SEED), rows)
    for row, (s, arr), w in zip(rows, out, want):
        assert (s[0], P.rng_of(s), arr) == w, (row[:3], row[P.RC_P:P.RC_P + 2])


def _injected_draws(r, n, kind, at):
    """n draws with distinct top-32 key bits, but the entries `at`: equal keys
    (draws that differ in their low 5 bits only), equal top 32 bits only, or
    the all-ones key of the lanes past the count"""
    his = r.sample(range(1, 1 << 32), n + 1)
    his.sort()
    tied_hi = his.pop(r.choice([0, 0, len(his) // 2, len(his) - 1]))   # often the smallest: across the cut
    r.shuffle(his)
    draws = [(h << 26) | r.getrandbits(26) for h in his[:n]]
    low = r.getrandbits(21)
    for i in at:
        if kind == "key":
            draws[i] = (((tied_hi << 21) | low) << 5) | r.getrandbits(5)
        elif kind == "hi":
            draws[i] = (tied_hi << 26) | r.getrandbits(26)
        elif kind == "ones":
            draws[i] = T58 - 1 - (r.getrandbits(5) if i != at[0] else 0)
    return draws


@pytest.mark.parametrize("form", ["wv", "lite<30,32>", "lite<8,32>", "lite<8,16>", "Pas<32>"])
def test_sublist_injected_ties(form):
    r = random.Random(500 + len(form))
    _, _, _, lanes, depth, nmax = SUB[form]
    nmax = min(nmax, 30) if form != "wv" else 64
    cases = []

    def add(n, k, on, draws, V=None):
        V = V if V is not None else ids_distinct(r, n, 1 << 27)
        base = r.getrandbits(40)
        off = r.randrange(0, depth - n + 1)                            # the cache covers [rng, rng + n)
        vals = [r.getrandbits(58) for _ in range(off)] + draws
        vals += [r.getrandbits(58) for _ in range(depth - len(vals))]
        OUT0 = [r.getrandbits(27) for _ in range(lanes)]
        cases.append((r.randrange(1 << 20), base + off, base, vals, V, n, k, on, OUT0))

    sizes = sorted({2, 3, 5, 8, nmax} | ({9, 29, 30} if nmax >= 30 else set()) | ({63, 64} if nmax == 64 else set()))
    for n in [s for s in sizes if s <= nmax]:
        ks = sorted({0, 1, 2, 3, n // 3, n // 3 + 1, n - 1, n, n + 2})  # n = 3 m, n = 3 m - 1: the wave_min path's edge
        for k in ks:
            for on in (0, 1, 3):
                if on + min(n, k) > (64 if form == "wv" else 99):
                    continue
                for kind in ("key", "hi", "ones"):
                    for cnt in (2, 3):
                        if cnt > n:
                            continue
                        at = sorted(r.sample(range(n), cnt))
                        draws = _injected_draws(r, n, kind, at)
                        V = ids_distinct(r, n, 1 << 27)
                        add(n, k, on, draws, V)
                        add(n, k, on, draws, list(reversed(V)))        # the element order the other way
                same = (r.getrandbits(53) << 5)
                add(n, k, on, [same | r.getrandbits(5) for _ in range(n)])             # all keys equal
                add(n, k, on, [T58 - 1] * n)                                           # ... and all-ones
    for n in (0, 1):
        for k in (0, 1, 4):
            for on in (0, 1, 3):
                add(n, k, on, [r.getrandbits(58) for _ in range(n)])
    # n = 3 m and 3 m - 1 with the tie among the m smallest
    for n, k in ((30, 10), (29, 10), (9, 3), (8, 3), (6, 2), (5, 2), (3, 1), (2, 1)):
        if n > nmax:
            continue
        for kind in ("key", "hi"):
            for _ in range(4):
                at = sorted(r.sample(range(n), 2))
                draws = _injected_draws(r, n, kind, at)
                for i in at:                                           # the two smallest top words tie
                    draws[i] = (1 << 26) | (r.getrandbits(5) if kind == "key" else r.getrandbits(26))
                add(n, k, 1, draws)
    r.shuffle(cases)
    _sub_check(form, cases)


# ---------------------------------------------------------- merge_exchange --
MERGE = {"wv": ("wv_merge", (), 1, 64), "lite32": ("lite_merge", (32,), 2, 32), "lite16": ("lite_merge", (16,), 4, 16)}


def _merge_cases(r, width, bucket, top, sorted_):
    """(me, rng, draws, A, P, EX, maxp) over the view sizes, the candidates'
    kinds and which cached draw the ?uniform_range test rejects"""
    out = []
    for maxp in (1, 7, 8, 29, 30):
        for fill in sorted({0, max(maxp - 3, 0), maxp - 1, maxp}):
            for rep in range(6):
                ids = ids_distinct(r, 60, top)
                me, A, Pv = ids[0], ids[1:1 + r.randrange(0, 7)], P.make_view(ids[8:8 + fill], bucket)
                new = ids[40:]
                nex = r.choice([1, 2, 5, 8, 8])
                EX = [r.choice(new) for _ in range(nex)]               # repeats among them
                if rep % 3 == 1 and nex >= 3:                          # members, Active, Myself
                    EX[0] = me
                    EX[1] = r.choice(A) if A else me
                    EX[2] = r.choice(Pv) if Pv else me
                if rep % 3 == 2:
                    EX = [r.choice(Pv + A + [me]) for _ in range(nex)] if rep == 5 else EX[:nex - 1] + [me]
                if sorted_:
                    EX = P.usort(EX)
                cand = [e for e in P.usort(EX) if e != me and e not in A]
                # the evictions of a run without a rejected draw
                draws = [r.choice([r.randrange(maxp), r.randrange(maxp, T58 - 64)]) if r.random() < 0.2
                         else r.randrange(64, T58 - 64) for _ in range(width)]
                rng = r.getrandbits(40)
                _, rng1, _ = P.merge_exchange(P.Draws(me, SEED, width, rng, draws), rng, me, A, Pv, EX, maxp, bucket)
                used = rng1 - rng
                spots = [None]
                if T58 % maxp:
                    if used:
                        spots += sorted({0, used // 2, used - 1})
                    if used < len(cand):
                        spots.append(r.randrange(used, len(cand)))     # a lane no eviction reads
                for sp in spots:
                    d = list(draws)
                    if sp is not None:
                        d[sp] = T58 - 1 - r.randrange(T58 % maxp)
                        if rep == 4 and sp + 1 < width:
                            d[sp + 1] = T58 - 1                        # two in a row
                    out.append((me, rng, d, A, Pv, EX, maxp))
    return out


@pytest.mark.parametrize("tabled", [False, True], ids=["default-hash", "table"])
@pytest.mark.parametrize("form", ["wv", "lite32-sorted", "lite32-usort", "lite16-sorted", "lite16-usort"])
def test_merge_exchange(form, tabled):
    name, pre, groups, width = MERGE[form.split("-")[0]]
    sorted_ = form.endswith("sorted")
    r = random.Random(len(form) * 3 + tabled)
    tab = np.array([r.getrandbits(8) for _ in range(4096)], np.uint8) if tabled else None
    if tabled:
        tab[:512] = 0x42                                   # many equal buckets
    b = P.bucket_of(tab)
    cases = _merge_cases(r, width, b, 4096 if tabled else 1 << 27, sorted_)
    by_maxp = {}
    for cse in cases:
        by_maxp.setdefault(cse[6], []).append(cse)
    # (a rejected draw among a merge's candidates sends the group down the sequential path)
    assert sum(1 for c in cases if T58 % c[6] and any(d >= T58 - T58 % c[6] for d in c[2][:8])) > 20
    for maxp, group in sorted(by_maxp.items()):
        r.shuffle(group)
        rows, want = [], []
        for me, rng, draws, A, Pv, EX, _ in group:
            rows.append(P.rc_row(me=me, rng=rng, dcb=rng, dc=draws, p=[len(A), len(Pv), len(EX), int(sorted_)],
                                 r0=Pv, r1=A, r2=EX))
            w = P.merge_exchange(P.Draws(me, SEED, width, rng, draws), rng, me, A, Pv, EX, maxp, b)
            want.append((len(w[0]), w[1], w[2], pad(w[0], 32)))
        out = P.rc_run(name, P.cfg(seed=SEED, max_passive=maxp, table=tab), rows, *pre, groups=groups)
        for row, (s, arr), w in zip(rows, out, want):
            assert (s[0], P.rng_of(s), s[3], arr[:32]) == w, (form, maxp, row[:3], row[P.RC_P:P.RC_P + 4])


# ------------------------------------------- psim_strategy.hip: L2 and sets --
def test_l2_insert_lookup():
    r = random.Random(2)
    rows, want = [], []
    for n in (0, 63, 64, 65, 126, 127):
        for pos in sorted({p for p in (0, 62, 63, 64, 65, n) if p <= n}):
            V, e = ids_distinct(r, n, 1 << 32), r.randrange(1, 1 << 32)
            rows.append([0, n, pos, e] + pad(V, 128))
            want.append((n + 1, 0, pad(P.list_ins(V, pos, e), 128)))
        V = ids_distinct(r, n, 1 << 32)
        for i in sorted({i for i in (0, 1, 62, 63, 64, 65, n - 1) if 0 <= i < n}):
            rows.append([2, n, i, 0] + pad(V, 128)); want.append((n, V[i], pad(V, 128)))
            rows.append([1, n, 0, V[i]] + pad(V, 128)); want.append((n, 1, pad(V, 128)))
        for e in (0, r.randrange(1, 1 << 32)):                         # 0 fills the entries past the count
            rows.append([1, n, 0, e] + pad(V, 128)); want.append((n, int(e in V), pad(V, 128)))
    out = P.run_rows("l2", P.cfg(), rows, P.L2_OUT)
    for row, o, w in zip(rows, out, want):
        assert (int(o[0]), int(o[1]), [int(x) for x in o[2:]]) == w, row[:4]


def test_add_del_set2_against_otp_sets():
    rows, wants = [], []
    tabs = []
    for t in range(3):
        r = random.Random(1000 + t)
        tab = np.array([r.getrandbits(8) for _ in range(4096)], np.uint8)
        ids = ids_distinct(r, 200, 4096)
        s, ops, live, want = P.otp_set(tab), [], [], []
        def do(e, delete):
            (s.del_element if delete else s.add_element)(e)
            ops.append(e | (1 << 31) if delete else e)
            want.append((len(s.to_list()), s.n, pad(s.to_list(), 128)))
        for e in ids[:128]:                                            # 16 slots up to 26
            do(e, False); live.append(e)
        spare = ids[128:]
        while len(live) > 40:                                          # ... and back to 16
            x = r.random()
            if x < 0.1 and len(live) < 128:
                e = spare.pop(); do(e, False); live.append(e)
            elif x < 0.2:
                do(spare[0], True)                                     # not a member
            else:
                do(live.pop(r.randrange(len(live))), True)
        assert max(w[1] for w in want) >= 26 and want[-1][1] == 16 and len(ops) <= P.S2_MAXOPS
        tabs.append(tab); wants.append(want)
        rows.append([len(ops)] + pad(ops, P.S2_MAXOPS))
    for tab, row, want in zip(tabs, rows, wants):
        out = P.run_rows("set2", P.cfg(table=tab), [row], P.S2_MAXOPS * P.S2_SOUT)[0].reshape(P.S2_MAXOPS, P.S2_SOUT)
        for s, w in enumerate(want):
            assert (int(out[s][0]), int(out[s][1]), [int(x) for x in out[s][2:]]) == w, (s, row[1 + s])


def test_set_slot_every_byte():
    tab = np.arange(256, dtype=np.uint8)                               # id = its hash byte
    rows = [[e, ns] for ns in range(16, 33) for e in range(256)]
    out = P.run_rows("set_slot", P.cfg(table=tab), rows, 1)
    assert [int(o[0]) for o in out] == [P.set_slot(tab, e, ns) for e, ns in rows]
