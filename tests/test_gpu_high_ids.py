"""The engine against the oracle at ids up to 2^27 - 2 (tests/_high_ids.py).

No other parity test uses an id at or above 2^20, and ids share 32-bit words
with other bits in the route keys (dst | max_emit << 27), the lite kernel's
tags (bucket << 27 | id), the connection entries, the Plumtree identities
and the records.  A host-exchange handle allocates node rows for its own ids
only, so a scenario of at most 1024 nodes runs in an id window anywhere in a
space of 2^27 - 1 ids: at its top (the last id has bits 0..26 all set), and
with 2^26 and 2^24 in the window's middle.  The oracle side is a range oracle
(orc_create_range), which tests/test_high_ids.py shows to be the oracle.

  one party   the engine owns the whole window: each scenario, each window
  boundary    top window, the engine the lower half beside a range oracle on
              the upper, and the other way round: every round's outbound list
              word for word the all-oracle exchange's (k_host_export,
              k_host_import, psim_record_check see the ids)
  also        snapshot and restore mid-run, a random bucket table (2^24: the
              table is id_space bytes), random schedules in their host form,
              the outbound records through the wire codec."""
import functools

import numpy as np
import pytest

import _high_ids as H
import _random_schedule as R
import _scenarios as S
from _hybrid import ENGINE, ORACLE
from partisan_amd import wire

pytestmark = pytest.mark.gpu

NAMES = list(H.SCENARIOS)
WINDOWS = ("top", "2^26", "2^24")


def _closed(name, out):
    """what a run leaves to compare, its handles closed"""
    sim = out[0]
    try:
        return {"stats": out[1], "extra": out[2:], "final": H.final(name, sim)}
    finally:
        sim.close()


@functools.lru_cache(maxsize=None)
def _oracle(name, window, buckets=None):
    """the reference: one range oracle over the window"""
    space, base = H.windows(H.size_of(name))[window]
    make = H.at_ids(H.one_party(ORACLE), base, space)
    return _closed(name, H.run(name, make if buckets is None else S.with_buckets(make, buckets),
                               **H.gpu_kw(name, window)))


# Overflow is 0 in every run but X-BOT's whole ones (2^26 and 2^24: 110
# rounds): there the oracle itself overflows disconnect-id maps past their 64
# entries (PSIM_OVF_IDMAP), where the same run at ids 0..1023 does not -- X-BOT
# places nodes by a hash of their id, so another window is another topology.
# The oracle's totals are pinned here; the engine must overflow the same
# tables in the same rounds (compare_stats: overflow, overflow_by).
ORACLE_OVERFLOW = {("xbot_churn", "2^26"): 65, ("xbot_churn", "2^24"): 4}


def _overflow(name, window, stats):
    assert int(stats["overflow"].sum()) == ORACLE_OVERFLOW.get((name, window), 0)


def _same(name, got, ref, window):
    S.compare_stats(got["stats"], ref["stats"])
    _overflow(name, window, got["stats"])
    assert got["extra"] == ref["extra"]
    H.compare_final(got["final"], ref["final"])


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", NAMES)
def test_one_party(name, window):
    space, base = H.windows(H.size_of(name))[window]
    got = _closed(name, H.run(name, H.at_ids(H.one_party(ENGINE), base, space), **H.gpu_kw(name, window)))
    _same(name, got, _oracle(name, window), window)


def test_bucket_table_2_24():
    """S.with_buckets through the proxy: the n buckets placed in a table of
    id_space bytes"""
    name, window = "churn_partition", "2^24"
    space, base = H.windows(H.size_of(name))[window]
    make = S.with_buckets(H.at_ids(H.one_party(ENGINE), base, space), 12)
    _same(name, _closed(name, H.run(name, make)), _oracle(name, window, 12), window)


# ---------------------------------------------------------------- across the boundary
SIDES = {"engine_low": (ENGINE, ORACLE), "engine_high": (ORACLE, ENGINE)}


@functools.lru_cache(maxsize=None)
def _all_oracle(name, side):
    """the expected exchange: the same two ranges, both played by range
    oracles -- its per-round trace; the run itself equals one range"""
    space, base = H.windows(H.size_of(name))["top"]
    out = H.run(name, H.at_ids(H.split(SIDES[side], engine=False), base, space), **H.gpu_kw(name, "top"))
    trace = out[0].trace
    assert out[0].n_out > 0 and out[0].n_in > 0
    _same(name, _closed(name, out), _oracle(name, "top"), "top")
    return trace


def _boundary(name, side, **kw):
    space, base = H.windows(H.size_of(name))["top"]
    out = H.run(name, H.at_ids(H.split(SIDES[side], expect=_all_oracle(name, side), **kw), base, space),
                **H.gpu_kw(name, "top"))
    hy = out[0]
    try:
        ref = _oracle(name, "top")
        S.compare_stats(out[1], ref["stats"])
        _overflow(name, "top", out[1])
        assert hy.n_out > 0 and hy.n_in > 0
        e = hy.engine
        assert e.hi - e.lo == H.size_of(name) // 2 and (e.hi == H.TOP) == (side == "engine_high")
        rows = ref["final"]["strategy_nodes" if H.pluggable(name) else "nodes"][e.lo - base:e.hi - base]
        S.compare_nodes(e.strategy_nodes() if H.pluggable(name) else e.nodes(), rows)
        if not hy.resumed:                   # (a fresh handle counts from its restore)
            assert e.exchange_stats() == (hy.n_out + hy.n_in, 64 * (hy.n_out + hy.n_in))
        return hy.resumed
    finally:
        hy.close()


@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("name", H.BOUNDARY)
def test_boundary_top(name, side):
    _boundary(name, side)


def test_snapshot_restore_top():
    """after round 45, in the churn, the engine's state moves into a fresh
    handle of the same range (psim_snapshot / psim_restore)"""
    assert _boundary("churn_partition", "engine_high", resume_at=45)


@functools.lru_cache(maxsize=None)
def _xbot_outbound():
    kept = []
    _boundary("xbot_churn", "engine_low", on_outbound=lambda r, box: kept.append(box.copy()))
    return np.concatenate(kept)


def test_outbound_records_round_trip_the_wire_top():
    """as tests/test_gpu_host_exchange.py's: encode then decode (dst passed in)
    gives the record back, seq zeroed; ids up to 2^27 - 2 in every id field"""
    nm = wire.names(prefix="n", host="127.0.0.1", ip_base=(10 << 24), port=9090)
    out = _xbot_outbound()
    assert out[:, 0].max() == H.TOP - 1 and out[:, 1].min() >= H.TOP - 1024
    k = 0
    for r in out:
        if (r[2] & 0xFF) == 11 and r[6] == 0xFFFFFFFF:
            continue
        got, _ = wire.decode(wire.encode(r, nm), nm, int(r[0]))
        want = r.copy()
        want[3] = 0
        assert np.array_equal(got, want), (r, got)
        k += 1
    assert k > 1000, k


# ---------------------------------------------------------------- random schedules
HOST_ENTRIES = [(k, s) for k in ("hv", "xbot", "scamp_v1", "scamp_v2") for s in R.CORPUS_SEEDS[k][:2]]
OPTS = R.Opts(drop=("histograms",), single_rounds=True)


@pytest.mark.parametrize("kind,seed", HOST_ENTRIES, ids=[f"{k}-{s}" for k, s in HOST_ENTRIES])
def test_random_schedule_top(kind, seed):
    sch = R.generate(kind, seed, host=True, rounds=H.RANDOM_TOP_ROUNDS)
    base = H.TOP - sch.n
    ref = R.execute(H.at_ids(H.one_party(ORACLE), base, H.TOP), sch, OPTS)
    got = R.execute(H.at_ids(H.one_party(ENGINE), base, H.TOP), sch, OPTS)
    R.compare(got, ref)
    assert int(got.stats["overflow"].sum()) == int(ref.stats["overflow"].sum())
