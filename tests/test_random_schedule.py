"""The corpus of seeded random schedules (tests/_random_schedule.py) is worth
running: conditions on the inputs, checked with the oracle alone.  Where one
fails, other seeds are chosen or the generator is tuned until the oracle meets
it -- never the engine.  tests/test_gpu_random_schedule.py runs the same
corpus on the GPU against these oracle traces.

Run with -s for the per-kind coverage table and the oracle time per entry
(recorded in profiles/random_schedules/oracle_times.txt)."""
import functools
import json
import os

import numpy as np
import pytest

import _random_schedule as R
from partisan_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "random_schedules.json")

# the message types a kind can send (include/partisan_gpu_sim.h)
HV_TYPES = set(range(14))
TYPES = {
    "hv": HV_TYPES,
    "xbot": HV_TYPES | set(range(16, 22)),
    "scamp_v1": {0, 1, 3, 4, 6},          # hello, state, forward_subscription, ping, remove_subscription
    "scamp_v2": {0, 1, 3, 4, 5, 7},       # ... keep_subscription, bootstrap_remove_subscription
    "full": {0, 1, 2},                    # hello, state, gossip
}
# (no type turned out unreachable: every set above is emitted and delivered)
IDS = [f"{k}-{s}" for k, s in R.CORPUS]


@functools.lru_cache(maxsize=None)
def _schedule(kind, seed):
    return R.generate(kind, seed)


@functools.lru_cache(maxsize=None)
def _trace(kind, seed):
    """the oracle's trace of a corpus entry (once; left unchanged)"""
    return R.execute(R.oracle_make, _schedule(kind, seed))


def _of(kind):
    return [(k, s) for k, s in R.CORPUS if k == kind]


def test_corpus_shape():
    assert len(set(R.CORPUS)) == len(R.CORPUS)
    for kind in R.KINDS:
        assert 8 <= len(_of(kind)) <= 12
    for kind, seed in R.CORPUS:
        sch = _schedule(kind, seed)
        assert sch.rounds() == R.ROUNDS
        assert sch.n in R.SIZES or (kind == "full" and sch.n == R.FULL_FLOOD_N)
        # the full strategy's flood: fanout 0 at 17 nodes only
        assert kind != "full" or sch.n <= 257 and (sch.config["fanout"] > 0 or sch.n == R.FULL_FLOOD_N)


def test_pinned():
    """a numpy or generator change cannot silently swap the corpus: the
    schedules' hashes and the oracle's summed digests are the recorded ones
    (tests/golden/gen_random_schedules.py rewrites the file)"""
    with open(GOLDEN) as f:
        pinned = json.load(f)
    assert sorted(pinned) == sorted(IDS)
    for kind, seed in R.CORPUS:
        p = pinned[f"{kind}-{seed}"]
        assert _schedule(kind, seed).sha256() == p["sha256"], f"{kind}-{seed}: another schedule than the pinned one"
        assert _trace(kind, seed).digest() == p["digest"], f"{kind}-{seed}: the oracle's digest sum moved"


@pytest.mark.parametrize("kind", R.KINDS)
def test_message_types(kind):
    em, de = np.zeros(_abi.STATS_DTYPE["emitted"].shape, np.uint64), np.zeros(_abi.STATS_DTYPE["emitted"].shape, np.uint64)
    for k, s in _of(kind):
        st = _trace(k, s).stats
        em += st["emitted"].sum(0)
        de += st["delivered"].sum(0)
    print(f"\n{kind}: emitted {dict((int(t), int(em[t])) for t in np.nonzero(em)[0])}")
    print(f"{kind}: delivered {dict((int(t), int(de[t])) for t in np.nonzero(de)[0])}")
    assert set(np.nonzero(em)[0].tolist()) == TYPES[kind]
    assert set(np.nonzero(de)[0].tolist()) == TYPES[kind]


@pytest.mark.parametrize("kind", R.KINDS)
def test_event_calls(kind):
    made, ok, total, refused = {}, {}, 0, 0
    for k, s in _of(kind):
        for _, name, rc in _trace(k, s).rcs:
            made[name] = made.get(name, 0) + 1
            ok[name] = ok.get(name, 0) + (rc == 0)
            total += 1
            refused += rc != 0
    print(f"\n{kind}: calls made {made}\n{kind}: accepted {ok}\n{kind}: refused {refused} of {total}")
    for name in R.CALLS[kind]:
        assert made.get(name, 0) >= 1, f"{name} is never called"
        assert ok.get(name, 0) >= 1, f"{name} is never accepted"
    assert set(made) <= set(R.CALLS[kind])
    assert 1 <= refused < 0.10 * total


def _started(sch):
    ids = set()
    for s in sch.steps:
        if s[0] == "call" and s[1] in ("join", "revive"):
            ids |= set(s[2][0])
    return ids


@pytest.mark.parametrize("kind,seed", R.CORPUS, ids=IDS)
def test_schedule_is_interesting(kind, seed):
    sch, tr = _schedule(kind, seed), _trace(kind, seed)
    st = tr.stats
    assert len(st) == R.ROUNDS and np.array_equal(st["round"], np.arange(R.ROUNDS))
    # liveness (refused starts count as started: the bound only gets harder)
    assert int(st["nodes_up"][-1]) * 4 >= len(_started(sch))
    # a step of five or more rounds with messages in flight in every round of it
    r, big = 0, 0
    for s in sch.steps:
        if s[0] == "step":
            if s[1] >= 5 and st["emitted"][r:r + s[1]].sum(1).min() > 0:
                big += 1
            r += s[1]
    assert big >= 1
    # a probe over a strict sub-range
    windows = [s for s in sch.steps if s[0] == "probe" and s[1] in ("nodes", "strategy_nodes", "delivery")]
    assert any(0 < s[3] < sch.n for s in windows)
    assert any(s[0] == "snapshot_restore" for s in sch.steps)
    assert np.array_equal(st["overflow"], st["overflow_by"].sum(1))


@pytest.mark.parametrize("kind", R.KINDS)
def test_overflow(kind):
    """most schedules count no overflow; at most two a kind may, so that
    "counted alike" is exercised too"""
    counting = []
    for k, s in _of(kind):
        st = _trace(k, s).stats
        assert np.array_equal(st["overflow"], st["overflow_by"].sum(1))
        if st["overflow"].sum():
            counting.append((s, st["overflow_by"].sum(0).tolist()))
    print(f"\n{kind}: schedules that count overflows (seed, by kind): {counting}")
    assert len(counting) <= 2


def test_digests_distinct():
    sums = [_trace(k, s).digest() for k, s in R.CORPUS]
    assert len(set(sums)) == len(sums)


@pytest.mark.parametrize("kind", R.KINDS)
def test_deterministic_and_json(kind):
    """the same schedule twice gives equal traces, and a schedule survives
    json.dumps / loads and executes to the same trace"""
    k, s = _of(kind)[1]
    sch = _schedule(k, s)
    assert R.generate(k, s) == sch
    R.compare(R.execute(R.oracle_make, sch), _trace(k, s))
    back = R.Schedule.from_json(json.loads(json.dumps(sch.to_json())))
    assert back == sch and back.steps == sch.steps and back.config == sch.config
    R.compare(R.execute(R.oracle_make, back), _trace(k, s))


def test_compare_is_sensitive():
    """one word flipped in a copied trace makes compare fail and name it"""
    k, s = "hv", R.CORPUS_SEEDS["hv"][0]
    good = _trace(k, s)
    R.compare(good.copy(), good)
    # one word of one node's passive row
    bad = good.copy()
    node = int(np.nonzero(bad.final["nodes"]["pas_n"])[0][3])
    bad.final["nodes"]["pas"][node][0] ^= 1
    with pytest.raises(AssertionError, match=rf"seed {s}: final state, nodes: node field pas differs at nodes \[{node}\]"):
        R.compare(bad, good)
    # one round's digest
    bad = good.copy()
    bad.stats["digest"][37] ^= 1 << 40
    with pytest.raises(AssertionError, match=rf"seed {s}: stats field digest differs first at round 37"):
        R.compare(bad, good)
    # one probe result
    bad = good.copy()
    at = next(j for j, p in enumerate(bad.probes) if p[1] == "nodes")
    i, what, first, count, rnd, res = bad.probes[at]
    res["rng_ctr"][count // 2] += 1
    with pytest.raises(AssertionError, match=rf"seed {s}: probe nodes \[{first}, {first + count}\) at step {i}, after round "
                                             rf"{rnd - 1}: node field rng_ctr differs at nodes \[{count // 2}\]"):
        R.compare(bad, good)
    # one event call's return code
    bad = good.copy()
    i, name, rc = bad.rcs[5]
    bad.rcs[5] = (i, name, rc - 1)
    with pytest.raises(AssertionError, match=rf"seed {s}: step {i}, call {name}: return code"):
        R.compare(bad, good)


SHARDED = [(k, s) for kind in R.KINDS if kind != "full" for k, s in _of(kind)[:2]]


@pytest.mark.parametrize("kind,seed", SHARDED, ids=[f"{k}-{s}" for k, s in SHARDED])
def test_oracle_shards(kind, seed):
    """four oracle shards exchanging records by hand (tests/_hybrid.py,
    engine=False) equal the unsharded oracle, on the host-exchange form of the
    entry (no leave_node, no histogram probe: both need a collective)"""
    sch = R.generate(kind, seed, host=True)
    assert not any(s[0] == "call" and s[1] == "leave_node" for s in sch.steps)
    make, opts = R.path("oracle-sharded")
    assert opts.restore is None and "histograms" in opts.drop
    a = R.execute(make, sch, opts)
    b = R.execute(R.oracle_make, sch)
    R.compare(a, b)
    assert len(a.probes) > 0


def test_oracle_time():
    rows = []
    for kind, seed in R.CORPUS:
        tr = _trace(kind, seed)
        sch = tr.schedule
        rows.append(f"{kind}-{seed}: n {sch.n}, {len(sch.calls())} event calls, {len(tr.probes)} probes, "
                    f"{int(tr.stats['emitted'].sum())} messages, {tr.seconds:.3f} s")
        assert tr.seconds < 1.0, rows[-1]
    print("\n" + "\n".join(rows))
    print(f"total: {sum(len(_schedule(k, s).calls()) for k, s in R.CORPUS)} event calls, "
          f"{R.ROUNDS * len(R.CORPUS)} rounds, {sum(_trace(k, s).seconds for k, s in R.CORPUS):.2f} s")


def test_shrink_tool():
    """the reducer on a CPU machine (backends oracle and oracle-sharded) with a
    planted difference: a comparer that rejects any schedule with a revive in
    it.  The reducer must end with that one call."""
    sch = R.generate("hv", 2, host=True)
    assert sch.n == 65 and len(sch.calls()) > 20

    def planted(a, b):
        R.compare(a, b)                                  # (the two oracles agree)
        assert not any(name == "revive" for _, name, _ in a.rcs), "planted: a revive"

    def fails(s):
        return R.differ(s, ("oracle-sharded", "oracle"), compare_fn=planted)

    small, used = R.shrink(sch, fails, max_steps=150)
    assert used <= 150
    assert [s[1] for s in small.calls()] == ["revive"], small.steps
    assert small.rounds() < sch.rounds() and len(small.steps) < 6
    assert "planted" in fails(small)
    # the tool's own entry point, on agreeing backends
    assert R.main(["--kind", "scamp_v2", "--seed", "2", "--backends", "oracle-sharded,oracle"]) == 0
