"""Test-only loader for tests/prims/libpsim_prims_test.so (one kernel a device
primitive, over the product's own text) and the plain models the GPU tests
compare it with.  The models work on Python ints and lists and are meant to be
obviously right, not fast; numpy only carries the cases to the launchers."""
import ctypes as C
import os

import numpy as np

import _oracle
from partisan_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "prims", "libpsim_prims_test.so")
MAKE_HINT = "build it with `make -C partisan_amd/csrc prims` (or __graft_entry__.build())"

NONE = _abi.PSIM_NONE
TWO58 = 1 << 58
EDOM = -22                      # a launcher's domain check refused a case

# the layouts of tests/prims/prims_host.h
RC_P, RC_DCL, RC_DCH, RC_R0, RC_R1, RC_R2, RC_IN, RC_OUT, RC_ARR = 5, 16, 80, 144, 208, 272, 336, 72, 8
PS_ROW, PS_STEPS, PS_NSTEP, PS_IN, PS_SOUT = 1, 33, 64, 33 + 128, 34
L32_V, L32_IN, L32_OUT = 4, 68, 66
L64_V, L64_IN, L64_OUT = 5, 133, 130
L2_V, L2_IN, L2_OUT = 4, 132, 130
S2_MAXOPS, S2_IN, S2_SOUT = 400, 401, 130


class PrimCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("max_passive", C.c_uint32), ("max_active", C.c_uint32),
                ("k_active", C.c_uint32), ("k_passive", C.c_uint32), ("btab", C.c_void_p),
                ("btab_len", C.c_uint64)]


_lib = None


def load():
    """The module, or an error that names the make target: never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: %s" % (LIB_PATH, MAKE_HINT))
        lib = C.CDLL(LIB_PATH)
        try:
            abi = lib.psim_prims_abi()
        except AttributeError:
            raise RuntimeError("%s exports no psim_prims_abi: %s" % (LIB_PATH, MAKE_HINT))
        if abi != _abi.PSIM_ABI_VERSION:
            raise RuntimeError("%s was built for ABI %d, the tree is ABI %d: %s"
                               % (LIB_PATH, abi, _abi.PSIM_ABI_VERSION, MAKE_HINT))
        lib.psim_prims_last_error.restype = C.c_char_p
        _lib = lib
    return _lib


def cfg(seed=23, max_passive=30, max_active=6, k_active=3, k_passive=4, table=None):
    """(PrimCfg, table): the fields a test kernel sees through kargs()"""
    c = PrimCfg(seed, max_passive, max_active, k_active, k_passive, None, 0)
    if table is not None:
        table = np.ascontiguousarray(table, np.uint8)
        c.btab, c.btab_len = table.ctypes.data, table.size
    c._keep = table
    return c


class DomainError(Exception):
    pass


_hip_error = None


def call(name, c, *args):
    """One launcher call; a HIP error or a refused case raises.  After a HIP
    error nothing more is launched from this process: a fault is to be read
    from the code, not run again."""
    global _hip_error
    if _hip_error is not None:
        raise RuntimeError("not launching psim_prims_%s: %s earlier in this process" % (name, _hip_error))
    rc = getattr(load(), "psim_prims_" + name)(C.byref(c), *args)
    if rc == EDOM:
        raise DomainError("%s: %s" % (name, load().psim_prims_last_error().decode()))
    if rc != 0:
        _hip_error = "psim_prims_%s returned HIP error %d" % (name, rc)
        raise RuntimeError(_hip_error)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def run_rows(name, c, rows, out_words, *pre, groups=1, post=()):
    """rows (cases x words, uint32) through launcher `name`; `groups` cases
    share a wave, so the rows are padded with copies of the last one"""
    rows = np.ascontiguousarray(rows, np.uint32)
    n = len(rows)
    pad = -n % groups
    if pad:
        rows = np.concatenate([rows, np.repeat(rows[-1:], pad, 0)])
    out = np.zeros((len(rows), out_words), np.uint32)
    call(name, c, *[C.c_uint32(p) for p in pre], _ptr(rows), C.c_uint32(len(rows)),
         *[C.c_uint32(p) for p in post], _ptr(out))
    return out[:n]


# ------------------------------------------------------------------ Philox --
def philox(c0, c1, c2, c3, k0, k1):
    out = (C.c_uint32 * 4)()
    _oracle.load().orc_philox(c0, c1, c2, c3, k0, k1, out)
    return list(out)


def draw58(ctr, node, seed):
    o = philox(ctr & 0xFFFFFFFF, ctr >> 32, node, 0, seed & 0xFFFFFFFF, seed >> 32)
    return ((o[1] << 32) | o[0]) >> 6


class Draws:
    """A node's draws behind a `width`-deep cache.  The cache may start with
    injected values at `base`; a draw outside it refills the whole cache from
    Philox at that draw's counter."""

    def __init__(self, node, seed, width, base=None, vals=None):
        self.node, self.seed, self.width = node, seed, width
        self.base, self.vals = base, list(vals) if vals is not None else None
        if self.vals is not None:
            assert base is not None and len(self.vals) == width

    def cover(self, base, n):
        if self.base is None or base < self.base or base + n > self.base + self.width:
            self.base = base
            self.vals = [draw58(base + i, self.node, self.seed) for i in range(self.width)]

    def at(self, ctr):
        return self.vals[ctr - self.base]

    def draw(self, ctr):
        self.cover(ctr, 1)
        return self.at(ctr)


# ------------------------------------------------------------------ models --
def uniform(draws, n):
    """OTP rand.erl ?uniform_range on 58-bit draws: (value, draws consumed)"""
    used = 0
    for v in draws:
        used += 1
        if v < n:
            return v + 1, used
        i = v % n
        if v - i <= TWO58 - n:
            return i + 1, used
    raise AssertionError("out of draws")


def uniform_at(D, rng, n):
    """rand:uniform(n) at counter rng: (value, the counter after)"""
    def stream():
        c = rng
        while True:
            yield D.draw(c)
            c += 1
    v, used = uniform(stream(), n)
    return v, rng + used


def select_random(D, rng, V, n, omit):
    elig = [e for e in V[:n] if e not in omit]
    if not elig:
        return NONE, rng
    k, rng = uniform_at(D, rng, len(elig))
    return elig[k - 1], rng


def sublist(V, n, k, keys):
    """the first min(n, k) of V[:n] sorted by (draw >> 5, element)"""
    order = sorted(range(n), key=lambda i: (keys[i] >> 5, V[i]))
    return [V[i] for i in order[:min(n, k)]]


def sublist_at(D, rng, V, n, k, OUT, on, lanes):
    """... of the draws at rng.., appended to OUT at lanes on.. of a
    `lanes`-wide register: (on + m, rng + n, OUT)"""
    D.cover(rng, n)
    got = sublist(V, n, k, [D.at(rng + i) for i in range(n)])
    out = list(OUT)
    for i, e in enumerate(got):
        if on + i < lanes:
            out[on + i] = e
    return on + len(got), rng + n, out


def usort(vals):
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return sorted(out)


def list_ins(V, pos, e):
    return V[:pos] + [e] + V[pos:]


def list_del(V, k):
    return V[:k] + V[k + 1:]


def bucket_of(table):
    """the 16-slot bucket of an id: the table's, or the default stand-in hash"""
    if table is None:
        lib = _oracle.load()
        return lambda e: int(lib.orc_bucket16(e))
    return lambda e: int(table[e]) & 15


def view_add(V, e, bucket):
    """sets:add_element in to_list order: after every entry of a bucket <= e's"""
    b = bucket(e)
    return list_ins(V, sum(1 for x in V if bucket(x) <= b), e)


def make_view(ids, bucket):
    V = []
    for e in ids:
        V = view_add(V, e, bucket)
    return V


def pas_step(P, e, evk, bucket):
    """one add_to_passive step: (P, changed); a member is a no-op, evk is the
    index evicted first or None"""
    if e in P:
        return P, 0
    if evk is not None:
        P = list_del(P, evk)
    return view_add(P, e, bucket), 1


def merge_exchange(D, rng, me, A, P, EX, maxp, bucket):
    """add_to_passive for each of usort(Exchange) -- Active -- [Myself]; a full
    view first evicts index uniform(|Passive|) - 1: (P, rng, dirty)"""
    cand = [e for e in usort(EX) if e != me and e not in A]
    dirty = 0
    if cand:
        D.cover(rng, len(cand))
    for e in cand:
        if e in P:
            continue
        if len(P) >= maxp:
            k, rng = uniform_at(D, rng, len(P))
            P = list_del(P, k - 1)
        P = view_add(P, e, bucket)
        dirty = 1
    return P, rng, dirty


def otp_set(table):
    from test_sets_v1 import OtpSetsV1
    return OtpSetsV1(table)


def set_slot(table, e, ns):
    """get_slot/2 of a sets v1 table with ns active slots, 0-based"""
    s = otp_set(table)
    s.maxn = 16
    while s.maxn < ns:
        s.maxn *= 2
    s.n, s.bso = ns, s.maxn // 2
    return s.get_slot(e) - 1


# ------------------------------------------------------- the RC case rows --
def rc_row(me=0, rng=0, dcb=None, dc=(), p=(), r0=(), r1=(), r2=()):
    """one case of a kernel that runs on a node's draw counter"""
    row = [0] * RC_IN
    dcb = (1 << 64) - 1 if dcb is None else dcb
    row[0:5] = [me, rng & 0xFFFFFFFF, rng >> 32, dcb & 0xFFFFFFFF, dcb >> 32]
    for i, v in enumerate(p):
        row[RC_P + i] = v
    for i, v in enumerate(dc):
        row[RC_DCL + i], row[RC_DCH + i] = v & 0xFFFFFFFF, v >> 32
    for at, r in ((RC_R0, r0), (RC_R1, r1), (RC_R2, r2)):
        for i, v in enumerate(r):
            row[at + i] = v
    return row


def rc_run(name, c, rows, *pre, groups=1):
    """-> per case (scalars, array) as Python ints; out[1:3] is the counter"""
    out = run_rows(name, c, rows, RC_OUT, *pre, groups=groups)
    return [([int(x) for x in o[:RC_ARR]], [int(x) for x in o[RC_ARR:]]) for o in out]


def rng_of(scalars):
    return scalars[1] | (scalars[2] << 32)
