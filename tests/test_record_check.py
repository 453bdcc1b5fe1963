"""psim_record_check (include/partisan_gpu_sim.h): the host-side check every
record passes before psim_round_absorb copies it to the device -- its type
must be one the manager's handlers receive, and dst, src, the exchange ids
and every word the handler reads as a node id must lie below cfg.n_nodes.
The id table is pinned against the wire codec by a route that shares none of
its code: the node names found in the bytes of the record's frame.  Pure host
code of the product library: no GPU needed."""
import ctypes as C
import re

import numpy as np

import _scenarios as S
from _oracle import Oracle
from partisan_amd import _lib, wire
from partisan_amd.sim import default_config

NM = wire.names(prefix="n", host="127.0.0.1", ip_base=(10 << 24), port=9090)
NAME = re.compile(rb"n(\d+)@127\.0\.0\.1")
NONE = 0xFFFFFFFF
OK, EINVAL, ERANGE = 0, -1, -5


def _records(sim, rounds):
    """Every record of `rounds` more rounds, in the codec's word order (the
    oracle packs seq before the type word), as tests/test_wire.py gathers
    them; an IHAVE of a retired id has no frame and is skipped there too."""
    out = []
    for _ in range(rounds):
        sim.step(1)
        for m in sim.inbox():
            r = np.zeros(16, np.uint32)
            r[0], r[1], r[2], r[3] = m[0], m[1], m[3], m[2]
            r[4:8], r[8:] = m[4:8], m[8:]
            if (r[2] & 0xFF) == 11 and r[6] == NONE:
                continue
            out.append(r)
    return out


def _pin(recs, cfg):
    """OK at n_nodes = m + 1 and ERANGE at n_nodes = m, m the largest id the
    record or its frame names."""
    cfg = type(cfg).from_buffer_copy(cfg)
    for r in recs:
        ids = [int(r[0]), int(r[1])] + [int(x) for x in NAME.findall(wire.encode(r, NM))]
        m = max(ids)
        cfg.n_nodes = m + 1
        assert wire.check(r, cfg) == OK, (r, m)
        cfg.n_nodes = m
        assert wire.check(r, cfg) == ERANGE, (r, m)


def test_ids_match_the_frames_hyparview():
    sim, _ = S.churn_partition(Oracle, n=512, rounds=60)
    sim.broadcast(3, 77)
    recs = _records(sim, 8)
    assert len(recs) > 1000
    assert {int(r[2]) & 0xFF for r in recs} >= {1, 2, 3, 7, 8, 9, 10, 11}
    _pin(recs, sim.cfg)


def test_ids_match_the_frames_xbot():
    sim, _ = S.churn_partition(Oracle, n=512, rounds=60, manager=2, xbot_period=5)
    recs = _records(sim, 12)
    assert len(recs) > 500
    assert any((int(r[2]) & 0xFF) >= 16 for r in recs)
    _pin(recs, sim.cfg)


def _rec(dst, src, t, nex=0, a=(0, 0, 0, 0), ex=()):
    r = np.zeros(16, np.uint32)
    r[0], r[1], r[2] = dst, src, t | (nex << 16)
    r[4:8] = a
    r[8:8 + len(ex)] = ex
    return r


def test_unknown_type_and_long_exchange():
    cfg = default_config(n_nodes=64)
    assert wire.check(_rec(1, 2, 7, nex=3, ex=(3, 4, 5)), cfg) == OK
    assert wire.check(_rec(1, 2, 23), cfg) == EINVAL
    assert wire.check(_rec(1, 2, 7, nex=9), cfg) == EINVAL
    # X-BOT's types belong to X-BOT handles
    assert wire.check(_rec(1, 2, 16, a=(3, 4, 5, NONE)), cfg) == EINVAL
    assert wire.check(_rec(1, 2, 16, a=(3, 4, 5, NONE)), default_config(n_nodes=64, manager=2)) == OK
    assert wire.check(_rec(1, 2, 16, a=(3, 4, 5, 64)), default_config(n_nodes=64, manager=2)) == ERANGE
    # an exchange id, and a Plumtree identity with and without the map bit
    assert wire.check(_rec(1, 2, 7, nex=2, ex=(3, 64)), cfg) == ERANGE
    assert wire.check(_rec(1, 2, 10, a=(0, 0, 63 | 0x80000000, 0)), cfg) == OK
    assert wire.check(_rec(1, 2, 10, a=(0, 0, 64 | 0x80000000, 0)), cfg) == ERANGE
    assert wire.check(_rec(1, 2, 10, a=(0, 0, NONE, 0)), cfg) == ERANGE
    assert wire.check(_rec(1, 2, 11, a=(5, 2, NONE, 0)), cfg) == OK


def test_scamp_records():
    n = 256
    sim, _ = S.pl_doubling(Oracle, n=n, seed=3, rounds=30, strategy=2)
    recs = _records(sim, 12)
    assert len(recs) > 200
    for r in recs:
        assert wire.check(r, sim.cfg) == OK, r
    assert wire.check(_rec(1, 2, 3, a=(n - 1, 0, 0, NONE)), sim.cfg) == OK      # PSIM_PL_FWD_SUB
    assert wire.check(_rec(1, 2, 3, a=(n, 0, 0, NONE)), sim.cfg) == ERANGE
    assert wire.check(_rec(1, 2, 2, a=(0, 0, 0, NONE)), sim.cfg) == EINVAL      # (GOSSIP: the full strategy's)


def test_host_comm_id_arguments():
    lib = _lib.load()
    f = lib.psim_host_comm_id
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32]
    n = lib.psim_comm_id_size()
    buf = C.create_string_buffer(n)
    assert f(buf, n, 0, 16) == OK
    assert buf.raw[:8] != bytes(8)
    assert f(None, n, 0, 16) == EINVAL
    assert f(buf, n - 1, 0, 16) == EINVAL
    assert f(buf, n, 16, 16) == EINVAL
    assert f(buf, n, 17, 16) == EINVAL
    a = C.create_string_buffer(n)
    assert f(a, n, 3, 9) == OK and a.raw != buf.raw
