"""psim_snapshot / psim_restore on every kind of handle: a run that is
snapshotted in the middle, closed, and carried on by a second handle that
restored the snapshot (S.resuming) must equal the oracle's uninterrupted run
of the same scenario bit for bit -- every round's stats and the final state.
A section of the snapshot that is missing, misplaced or restored into the
wrong buffer, or state of the target handle that survives the restore, shows
as a divergence in the rounds after it.

The cases put the restore where the sections have content: under a partition
(the partition bytes), after churn (id-map extension rows, the connection
table), on SCAMP v1 / v2 and full-membership handles (sview, sinv, fbits, the
payload arena with its remove rows), under X-BOT, with all root slots taken
and retired message ids (the message-slot table), with quiet nodes and
outstanding extension rows, on sharded handles and on loopback ranks -- into
a fresh handle and into one that has already run rounds of its own."""
import functools

import pytest

import _scenarios as S
from _oracle import Oracle

pytestmark = pytest.mark.gpu


def _gpu(cfg):
    from partisan_amd import Simulator
    cfg.device = 0
    return Simulator(cfg)


def _sharded(cfg):
    cfg.n_shards = 3
    return _gpu(cfg)


def _loopback2(cfg):
    from _loopback import LoopbackRanks
    return LoopbackRanks(cfg, 2)


# name -> (run(make) -> (sim, stats, ...), compare(gpu sim, oracle sim))
def _nodes(g, o):
    S.compare_nodes(g.nodes(), o.nodes())


def _full(n):
    return lambda g, o: S.compare_strategy(g, o, full_bits=[0, 1, n // 2, n - 1])


SCENARIOS = {
    "churn_partition_2048": (lambda mk: S.churn_partition(mk, n=2048), _nodes),
    "churn_partition_1024": (lambda mk: S.churn_partition(mk, n=1024), _nodes),
    "xbot_churn": (lambda mk: S.xbot_churn(mk, n=1024, rounds=120), _nodes),
    "scamp_v1": (lambda mk: S.pl_doubling(mk, 1024, 11, 100, strategy=1, crash_at=40, part_at=60),
                 S.compare_strategy),
    "scamp_v2": (lambda mk: S.pl_doubling(mk, 1024, 11, 100, strategy=2, crash_at=40, part_at=60),
                 S.compare_strategy),
    # full membership: the remove rows of leave/1 live in the payload arena
    "full_leave_1024": (lambda mk: S.pl_leave_remote(mk, 1024, 8, 90, strategy=0, fanout=5, k=4), _full(1024)),
    "full_leave_32": (lambda mk: S.pl_leave_remote(mk, 32, 8, 90, strategy=0, fanout=0, k=4), _full(32)),
    # six live roots over four root slots, message ids past the slot table
    "multi_root": (lambda mk: S.multi_root(mk, n=512, roots=6, rounds=120), _nodes),
    "heal_after_quiet": (lambda mk: S.heal_after_quiet(mk), _nodes),
    "omission": (lambda mk: S.pl_omission(mk, 1024, 23, 100, 2), S.compare_strategy),
}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle's uninterrupted run (once per scenario, left unchanged)"""
    out = SCENARIOS[name][0](Oracle)
    return out[0], out[1]


def _check(name, make, at, target="fresh"):
    holder = []

    def mk(cfg):
        holder.append(S.resuming(make, at, target)(cfg))
        return holder[0]
    out = SCENARIOS[name][0](mk)
    gs, gst = out[0], out[1]
    assert gs is holder[0] and gs.resumed, "the run never reached the restore"
    os_, ost = _oracle(name)
    S.compare_stats(gst, ost)
    SCENARIOS[name][1](gs, os_)
    gs.close()


@pytest.mark.parametrize("target", ["fresh", "used"])
@pytest.mark.parametrize("make", [_gpu, _sharded], ids=["unsharded", "shards3"])
def test_restore_under_partition(make, target):
    """round 95 of churn_partition: the partition of rounds 90-99 in force,
    the churn's id-map extension rows and connection tables in use"""
    _check("churn_partition_2048", make, 95, target)


def test_restore_xbot():
    _check("xbot_churn", _gpu, 95)


@pytest.mark.parametrize("name", ["scamp_v1", "scamp_v2"])
def test_restore_scamp(name):
    """round 65: after the crashes and rejoins, inside the partition of rounds 60-69"""
    _check(name, _gpu, 65)


@pytest.mark.parametrize("name", ["full_leave_1024", "full_leave_32"])
def test_restore_full_with_remove_rows(name):
    """round 50: the leave/1 calls of round 40 left remove rows in the payload arena"""
    _check(name, _gpu, 50)


def test_restore_multi_root():
    _check("multi_root", _gpu, 75)


def test_restore_with_quiet_nodes():
    """round 66 of heal_after_quiet, inside the quiet step(7): quiet nodes and
    outstanding extension rows at the restore, the heal two rounds later"""
    _check("heal_after_quiet", _gpu, 66)


def test_restore_loopback_ranks_used():
    """two loopback ranks restored, rank by rank, into a world that has
    exchanged rounds of its own (capacities and batch length from them)"""
    _check("churn_partition_1024", _loopback2, 95, "used")


def test_snapshot_refused_under_faults_then_restore_after_heal():
    """pl_omission: the omission faults (rounds 40-74) are host state, so a
    snapshot at round 50 is refused (PSIM_ESTATE) and changes nothing; after
    resolve_all_faults (round 75) a restore at round 80 continues in parity"""
    from partisan_amd import Simulator
    from partisan_amd.sim import SimError
    refused = []

    class Probing(Simulator):
        def step(self, n_rounds=1):
            if self.round == 50:
                with pytest.raises(SimError):
                    self.snapshot()
                refused.append(50)
            return super().step(n_rounds)

    def make(cfg):
        cfg.device = 0
        return Probing(cfg)
    _check("omission", make, 80)
    assert refused == [50]
