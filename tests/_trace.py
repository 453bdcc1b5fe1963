"""The reference of the message trace (psim_trace_watch / psim_trace_read): a
numpy filter over Oracle.inbox().  Expected values never come from the engine.

After the oracle has stepped round r, Oracle.inbox() is the set of records
sent in r -- the inbox round r + 1 will read -- which is what an armed engine
handle captures for round r.  The oracle packs seq before the type word: words
2 and 3 are swapped here, into the wire codec's layout (dst, src, type | ttl <<
8 | nex << 16, seq, a0..a3, ex[0..8))."""
import numpy as np

from _oracle import Oracle
from partisan_amd import _abi

ALL_TYPES = (1 << _abi.NTYPES) - 1
PL_STATE, PL_GOSSIP = 1, 2                      # psim_pl_msg_type: payload words are arena references


def mask_of(types):
    m = 0
    for t in types:
        m |= 1 << int(t)
    return m


def canonical(inbox):
    """An Oracle.inbox() array in the wire layout, in (dst, src, seq) order"""
    r = np.ascontiguousarray(inbox, np.uint32).reshape(-1, 16).copy()
    r[:, [2, 3]] = r[:, [3, 2]]
    return r[np.lexsort((r[:, 3], r[:, 1], r[:, 0]))]


def select(recs, n_nodes, nodes=None, to=True, frm=True, type_mask=ALL_TYPES, owned=None):
    """The records of one round (wire layout) a watch keeps: the type's bit in
    type_mask, and dst watched with `to` or src watched with `frm`.
    nodes=None: every node.  owned=(lo, hi): a rank handle, dst in [lo, hi)."""
    table = np.array([(type_mask >> k) & 1 for k in range(256)], bool)
    keep = table[recs[:, 2] & 0xFF]
    w = np.ones(n_nodes, bool) if nodes is None else np.zeros(n_nodes, bool)
    if nodes is not None:
        w[np.asarray(nodes, np.int64)] = True
    d = np.zeros(len(recs), bool)
    if to:
        d |= w[recs[:, 0]]
    if frm:
        d |= w[recs[:, 1]]
    if owned is not None:
        d &= (recs[:, 0] >= owned[0]) & (recs[:, 0] < owned[1])
    return recs[keep & d]


class Reference:
    """A watch's buffer over the rounds fed to it: add(round, records of that
    round in canonical order) applies the filter and the capacity rule -- the
    first `capacity` matches since the last read are kept, the later ones
    counted in lost -- and read() returns (recs, rounds, lost) and empties it."""

    def __init__(self, n_nodes, nodes=None, to=True, frm=True, type_mask=ALL_TYPES, capacity=1 << 20, owned=None):
        self.n, self.kw = n_nodes, dict(nodes=nodes, to=to, frm=frm, type_mask=type_mask, owned=owned)
        self.capacity = capacity
        self._clear()

    def _clear(self):
        self.recs, self.rounds, self.kept, self.lost = [], [], 0, 0

    def add(self, rnd, recs):
        m = select(recs, self.n, **self.kw)
        room = self.capacity - self.kept
        k = min(room, len(m))
        self.recs.append(m[:k])
        self.rounds.append(np.full(k, rnd, np.uint32))
        self.kept += k
        self.lost += len(m) - k

    def feed(self, tape, first=0, last=None):
        """the rounds r of a tape with first <= r (< last)"""
        for r, recs in tape:
            if r >= first and (last is None or r < last):
                self.add(r, recs)
        return self

    def read(self):
        recs = np.concatenate(self.recs) if self.recs else np.zeros((0, 16), np.uint32)
        rounds = np.concatenate(self.rounds) if self.rounds else np.zeros(0, np.uint32)
        out = recs.reshape(-1, 16), rounds, self.lost
        self._clear()
        return out


class TapedOracle(Oracle):
    """An oracle that steps one round at a time whatever step() is asked and
    keeps every round's records: tape = [(round, canonical records)]"""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.tape = []

    def step(self, n_rounds=1):
        out = []
        for _ in range(n_rounds):
            r = self.round
            out.append(super().step(1))
            self.tape.append((r, canonical(self.inbox())))
        return np.concatenate(out) if out else super().step(0)

    def counts(self):
        return np.array([len(recs) for _, recs in self.tape])


def assert_same(got, want, opaque_payload=False):
    """(recs, rounds, lost) of the engine against the reference's: every word
    and the round, exactly.  opaque_payload (the full strategy): STATE and
    GOSSIP records on words 0-3 only."""
    (g, gr, gl), (w, wr, wl) = got, want
    assert len(g) == len(w), f"{len(g)} records against {len(w)}"
    assert gl == wl, f"lost {gl} against {wl}"
    assert np.array_equal(gr, wr), "rounds differ"
    g, w = g.copy(), w.copy()
    if opaque_payload:
        t = w[:, 2] & 0xFF
        rows = (t == PL_STATE) | (t == PL_GOSSIP)
        g[rows, 4:] = 0
        w[rows, 4:] = 0
    if not np.array_equal(g, w):
        k = int(np.nonzero((g != w).any(1))[0][0])
        raise AssertionError(f"record {k} (round {int(gr[k])}): {g[k].tolist()} against {w[k].tolist()}")
