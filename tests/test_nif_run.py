"""The Erlang NIF shim (erlang/c_src/partisan_gpu_sim_nif.c), executed: the
shim is compiled into tests/nif_run's driver program over a stand-in erl_nif
runtime, with the CPU oracle behind the psim_* calls, and driven from here
(tests/_nif_run.py).  The expected side is always the oracle called directly
through ctypes and projected to what the NIF surface shows; it never comes
through the shim.  Every comparison is exact.

What the stand-in cannot show: scheduler behaviour, real term sizes, a real
erl_nif.h's types."""
import functools
import os
import re
import threading

import numpy as np
import pytest

import _nif_run as N
import _random_schedule as R
from _oracle import Oracle
from partisan_amd.sim import SimError, default_config

pytestmark = pytest.mark.skipif(not N.have_gcc(), reason="no C compiler (gcc) in this image: the shim cannot be built")

B1 = "<<01000000>>"
# valid arguments after the handle, for a handle of 8 nodes
VALID = {
    "join_nif": [B1, "<<00000000>>"], "crash_nif": [B1], "revive_nif": [B1], "leave_nif": [B1],
    "leave_node_nif": [B1, "<<02000000>>"], "broadcast_nif": ["0", "1"], "step": ["1"], "round_emit": [],
    "outbound": [], "round_absorb": ["<<>>"], "active_nif": ["0"], "members_nif": ["0", "8"], "delivery_nif": ["0"],
    "histograms": [], "strategy_histograms": [], "graph_metrics_nif": ["<<>>", "0"],
    "set_partition_nif": ["<<" + "00" * 8 + ">>"], "clear_partition_nif": [],
    "set_bucket_table_nif": ["<<" + "03" * 8 + ">>"], "set_phash_table_nif": ["<<" + "07000000" * 8 + ">>"],
    "omission_nif": ["0", B1, "<<02000000>>", "1"], "faulted_nif": [B1, "1"], "clear_faults_nif": [],
    "node_nif": ["0"], "msg_slots_nif": [], "snapshot": [], "restore": ["<<00>>"],
}
BUSY = ("error", "busy")
OOM = ("error", "out of memory")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return N.build(tmp_path_factory.mktemp("nif_run"))


def _table_from_source():
    c = open(N.SHIM).read()
    return [(n, int(a), f) for n, a, f in re.findall(r'\{"(\w+)",\s*(\d+),\s*nif_\w+,\s*(\w+)\}', c)]


def _create(beam, name, **cfg):
    ans = beam.call(f"{name} = create {N.erl(cfg)}")
    assert isinstance(ans, tuple) and ans[0] == "ok", ans
    return "$" + name


def _boot(beam, h, n=8):
    """ids 0..n-1 join in a chain; ten rounds"""
    assert beam.call(f"join_nif {h} {N.pack([0])} {N.pack([N.NONE])}") == "ok"
    assert beam.call(f"step {h} 1")[0] == "ok"
    assert beam.call(f"join_nif {h} {N.pack(range(1, n))} {N.pack(range(0, n - 1))}") == "ok"
    return beam.call(f"step {h} 10")


def _after(beam, h, n=8):
    """what a handle shows now and over its next rounds"""
    out = [beam.call(f"step {h} 6")]
    out += beam.calls([f"node_nif {h} {i}" for i in range(n)] + [f"members_nif {h} {i} {n}" for i in range(n)])
    return out


# ---------------------------------------------------------------- the table
def test_table_is_callable_at_its_arity(exe):
    with N.Beam(exe) as b:
        table = b.call("!table")
        flags = {"0": 0, "ERL_NIF_DIRTY_JOB_CPU_BOUND": 1, "ERL_NIF_DIRTY_JOB_IO_BOUND": 2}
        assert table == [(n, a, flags[f]) for n, a, f in _table_from_source()] and len(table) == 28
        assert sorted(n for n, _, _ in table) == sorted(list(VALID) + ["create"]) and len(VALID) == 27
        for name, arity, _ in table:
            assert len(VALID.get(name, [])) + 1 == arity
            assert b.call(" ".join([name] + ["foo"] * arity)) == "badarg", name
            assert b.call(" ".join([name] + ["foo"] * (arity + 1))) == ("undef", arity + 1)
        b.finish_clean()


def test_wrong_handle_is_badarg(exe):
    with N.Beam(exe) as b:
        assert b.call("!other o") == "ok"
        h = _create(b, "h", n_nodes=8, manager=1, strategy=1)
        for name, args in VALID.items():
            for wrong in ("foo", "7", "<<00>>", "$o", "{ok," + h + "}", "#{}"):
                assert b.call(" ".join([name, wrong] + args)) == "badarg", (name, wrong)
        assert b.live() == (0, 0, 2, 1)
        b.finish_clean()


# ---------------------------------------------------------------- create/1
BASES = {"hv": ("hv", 6), "xbot": ("xbot", 2), "v1": ("scamp_v1", 2), "full": ("full", 4)}
# key -> (the corpus schedule it is changed in, its other value)
KEY_CASES = {
    "seed": ("hv", 99), "max_active_size": ("hv", 4), "min_active_size": ("hv", 1), "max_passive_size": ("hv", 8),
    "arwl": ("hv", 2), "prwl": ("hv", 2), "k_active": ("hv", 1), "k_passive": ("hv", 1), "shuffle_period": ("hv", 4),
    "promotion_period": ("hv", 5), "random_promotion": ("hv", 0), "persist_epoch": ("hv", 1), "plumtree": ("hv", 0),
    "lazy_tick_period": ("hv", 1), "manager": ("hv", 2), "strategy": ("v1", 2), "periodic_interval": ("v1", 4),
    "scamp_c": ("v1", 1), "fanout": ("full", 5), "xbot_period": ("xbot", 9),
}
# keys whose effect no schedule of the corpus can carry, and the test that shows the shim reads them
ELSEWHERE = {"n_nodes": "test_create_n_nodes", "strict": "test_error_atoms"}


@functools.lru_cache(maxsize=None)
def _schedule(kind, seed):
    return R.generate(kind, seed)


@functools.lru_cache(maxsize=None)
def _want(kind, seed, key=None, value=None):
    """the oracle's projected trace of a corpus schedule, one config key changed"""
    sch = _schedule(kind, seed)
    if key is not None:
        sch = R.Schedule(sch.kind, sch.seed, dict(sch.config, **{key: value}), sch.steps)
    return sch, N.project(R.execute(R.oracle_make, sch))


def _through_the_shim(exe, sch, opts=None, timeout=60.0):
    with N.Beam(exe, timeout=timeout) as b:
        got = R.execute(N.nif_make(b), sch, opts)
        b.finish_clean()
    return got


def test_every_protocol_field_has_a_case():
    """derived from the ABI's config structure: a new field fails here until
    the shim reads it and a case shows that it does"""
    assert N.CONFIG_KEYS[0] == "n_nodes" and N.CONFIG_KEYS[1] == "seed" and N.CONFIG_KEYS[-1] == "xbot_period"
    assert sorted(N.CONFIG_KEYS) == sorted(list(KEY_CASES) + list(ELSEWHERE))
    src = open(N.SHIM).read()
    for k in N.CONFIG_KEYS:
        assert f'"{k}"' in src, f"create/1 never reads {k}"
    for name in ELSEWHERE.values():
        assert name in globals()


@pytest.mark.parametrize("key", list(KEY_CASES))
def test_create_reads_the_key(exe, key):
    """a run whose only difference is the key: the oracle's differs from the
    default run, and the shim's equals the oracle's"""
    base, value = KEY_CASES[key]
    kind, seed = BASES[base]
    _, default = _want(kind, seed)
    sch, want = _want(kind, seed, key, value)
    assert _schedule(kind, seed).config.get(key, getattr(default_config(), key)) != value
    with pytest.raises(AssertionError):
        N.same(want, default)             # (the key is live on the oracle in this schedule)
    N.same(_through_the_shim(exe, sch), want)


def test_create_n_nodes(exe):
    with N.Beam(exe) as b:
        h = _create(b, "h", n_nodes=40)
        assert b.call(f"node_nif {h} 39")[0] == "ok"
        assert b.call(f"node_nif {h} 40") == ("error", "node id out of range")
        assert b.call(f"set_partition_nif {h} <<{'00' * 40}>>") == "ok"
        b.finish_clean()


def test_create_refuses_what_is_not_a_config(exe):
    with N.Beam(exe) as b:
        for bad in ("foo", "7", "[]", "{n_nodes,8}", "<<>>"):
            assert b.call(f"create {bad}") == "badarg", bad
        for k in N.CONFIG_KEYS + ("host_lo", "host_hi"):
            for v in ("foo", "<<01>>", "[1]", "#{}"):
                assert b.call("create " + N.erl(dict({"n_nodes": 8}, **{k: v}))) == "badarg", (k, v)
            if k != "seed":
                assert b.call("create " + N.erl(dict({"n_nodes": 8}, **{k: 4294967296}))) == "badarg", k
        assert b.call("create #{n_nodes => 8, seed => 18446744073709551615}")[0] == "ok"
        assert b.live() == (0, 0, 0, 0)
        b.finish_clean()


def test_create_failures_leave_nothing(exe):
    with N.Beam(exe) as b:
        assert b.call("create #{n_nodes => 0}") == ("error", "invalid argument")
        assert b.live() == (0, 0, 0, 0)          # the mutex destroyed, nothing left allocated
        assert b.call("create #{n_nodes => 8, host_lo => 2, host_hi => 6}") == ("error", "unsupported")
        assert b.live() == (0, 0, 0, 0)
        b.finish_clean()


# ---------------------------------------------------------------- argument checks
def _bad_calls(h):
    three = "<<010000>>"
    return [
        f"join_nif {h} {three} {three}", f"join_nif {h} {B1} <<>>", f"join_nif {h} <<>> {B1}", f"join_nif {h} 1 {B1}",
        f"crash_nif {h} {three}", f"revive_nif {h} {three}", f"leave_nif {h} {three}", f"crash_nif {h} [1]",
        f"leave_node_nif {h} {three} {three}", f"leave_node_nif {h} {B1} <<0100000002000000>>",
        f"omission_nif {h} 0 {three} {three} 1", f"omission_nif {h} 0 {B1} <<>> 1", f"omission_nif {h} foo {B1} {B1} 1",
        f"omission_nif {h} 0 {B1} {B1} foo", f"faulted_nif {h} {three} 1", f"faulted_nif {h} {B1} foo",
        f"set_partition_nif {h} <<{'00' * 7}>>", f"set_partition_nif {h} <<{'00' * 9}>>",
        f"set_bucket_table_nif {h} <<{'00' * 7}>>", f"set_bucket_table_nif {h} <<{'00' * 9}>>",
        f"set_phash_table_nif {h} <<{'00' * 28}>>", f"set_phash_table_nif {h} <<{'00' * 33}>>",
        f"set_phash_table_nif {h} <<{'00' * 8}>>",
        f"step {h} 0", f"step {h} 100001", f"step {h} foo",
        f"graph_metrics_nif {h} {N.pack(range(65))} 0", f"graph_metrics_nif {h} {three} 0",
        f"graph_metrics_nif {h} <<>> foo", f"round_absorb {h} <<{'00' * 63}>>", f"round_absorb {h} foo",
        f"broadcast_nif {h} foo 1", f"broadcast_nif {h} 0 foo", f"node_nif {h} foo", f"active_nif {h} <<>>",
        f"members_nif {h} 0 7", f"members_nif {h} 0 9", f"members_nif {h} foo 8", f"delivery_nif {h} foo",
        f"restore {h} 5",
    ]


def case_argument_checks(b, strategy=1):
    """each bad call is badarg, leaves the mutex free (the driver checks that
    after every call) and the handle as a run without it"""
    cfg = dict(n_nodes=8, seed=4, manager=1, strategy=strategy)
    plain, tried = _create(b, "plain", **cfg), _create(b, "tried", **cfg)
    assert _boot(b, plain) == _boot(b, tried)
    before = b.live()
    for line in _bad_calls(tried):
        assert b.call(line) == "badarg", line
        assert b.live() == before, line
    assert _after(b, plain) == _after(b, tried)


def test_argument_checks(exe):
    for strategy in (0, 1):
        with N.Beam(exe) as b:
            case_argument_checks(b, strategy)
            b.finish_clean()


# ---------------------------------------------------------------- error atoms
def _ops(sim, ops):
    """[(method, args...)] on a driver; each answer 0 or the error"""
    out = []
    for name, *args in ops:
        try:
            res = getattr(sim, name)(*args)
            out.append(len(res) if name == "step" else 0)
        except SimError as e:
            out.append(e.rc)
    return out


CAPACITY_OPS = [("join", [0], [N.NONE]), ("step", 1), ("join", list(range(1, 8)), [0] * 7), ("step", 10)] + \
    [x for r in range(6) for x in (("broadcast", r, r + 1), ("step", 2))]


def test_error_atoms(exe):
    """every PSIM_E* code a handle returns without a GPU arrives as {error,
    Atom} with psim_strerror's text"""
    seen = set()
    with N.Beam(exe) as b:
        assert b.call("create #{n_nodes => 0}") == ("error", N.STRERROR[-1])
        hv = _create(b, "hv", n_nodes=8)
        _boot(b, hv)
        for line, code in ((f"join_nif {hv} {N.pack([1, 1])} {N.pack([0, 0])}", -1),
                           (f"set_bucket_table_nif {hv} <<{'01' * 8}>>", -4), (f"members_nif {hv} 0 8", -4),
                           (f"node_nif {hv} 8", -5), (f"crash_nif {hv} {N.pack([8])}", -5),
                           (f"broadcast_nif {hv} 0 65536", -5), (f"leave_nif {hv} {B1}", -7),
                           (f"faulted_nif {hv} {B1} 1", -7), (f"snapshot {hv}", -7), (f"restore {hv} <<00>>", -7),
                           (f"strategy_histograms {hv}", -7), (f"graph_metrics_nif {hv} <<>> 0", -7),
                           (f"set_partition_nif {hv} <<{'ff' * 8}>>", -1)):
            ans = b.call(line)
            assert ans == ("error", N.STRERROR[code]), (line, ans)
            seen.add(code)
        # ECAPACITY under strict: a fifth live Plumtree root at a node
        for strict in (0, 1):
            cfg = default_config(n_nodes=8, seed=3, strict=strict)
            o = Oracle(type(cfg).from_buffer_copy(cfg))
            want = _ops(o, CAPACITY_OPS)
            o.close()
            assert (-8 in want) == bool(strict)
            got = _ops(N.NifSim(b, cfg), CAPACITY_OPS)
            assert got == [N._rc(x) if x <= 0 else x for x in want], (got, want)
            seen |= {x for x in want if x < 0}
        b.finish_clean()
    assert seen == {-1, -4, -5, -7, -8}


def test_strerror_texts_fit_an_atom():
    """err() makes an atom of psim_strerror's text: at most 255 bytes each,
    and the restatements (the oracle stand-in, the tests' table) are the library's"""
    hip = open(os.path.join(N.LIB_DIR, "psim_engine.hip")).read()
    body = hip[hip.index("const char* psim_strerror"):]
    body = body[:body.index("\n}")]
    lib = dict(re.findall(r'case (PSIM_\w+): return "([^"]*)"', body))
    lib_default = re.search(r'default: return "([^"]*)"', body).group(1)
    codes = {"PSIM_OK": 0}
    for name, v in re.findall(r"#define (PSIM_E\w+) (-\d+)", open(os.path.join(N.ROOT, "include", "partisan_gpu_sim.h")).read()):
        codes[name] = int(v)
    assert sorted(lib) == sorted(codes) and len(codes) == 9
    assert {codes[k]: v for k, v in lib.items()} == N.STRERROR
    stand_in = open(os.path.join(N.NIF_RUN, "psim_on_oracle.c")).read()
    assert dict(re.findall(r'case (PSIM_\w+): return "([^"]*)"', stand_in)) == lib
    assert re.search(r'default: return "([^"]*)"', stand_in).group(1) == lib_default
    for text in list(lib.values()) + [lib_default]:
        assert 0 < len(text.encode()) <= 255


# ---------------------------------------------------------------- busy
def case_busy_injected(b):
    """trylock busy: {error, busy}, nothing leaked, nothing changed"""
    table = b.call("!table")
    normal = [n for n, a, f in table if f == 0 and n != "create"]
    assert len(normal) == 18          # every NIF of the table but create/1 and the nine dirty ones
    cfg = dict(n_nodes=8, seed=4, manager=1, strategy=1)
    plain, tried = _create(b, "plain", **cfg), _create(b, "tried", **cfg)
    assert _boot(b, plain) == _boot(b, tried)
    before = b.live()
    for name in normal:
        line = " ".join([name, tried] + VALID[name])
        assert b.call("!busy") == "ok"
        assert b.call(line) == BUSY, line
        assert b.live() == before, f"{name} leaks on its busy path"
    assert _after(b, plain) == _after(b, tried)


def test_busy_injected(exe):
    with N.Beam(exe) as b:
        case_busy_injected(b)
        b.finish_clean()


def test_busy_with_a_step_on_a_second_thread(exe):
    with N.Beam(exe) as b:
        N.busy_two_threads(b, Oracle)
        b.finish_clean()


# ---------------------------------------------------------------- allocation failures
def case_allocation_failures(b):
    """each injected failure: an error term, no crash, no held mutex (the
    driver checks), no leak, and the handle goes on as a run without it"""
    for what in ("alloc_resource", "mutex_create"):
        assert b.call(f"!fail {what} 1") == "ok"
        assert b.call("create #{n_nodes => 8}") == OOM, what
        assert b.live() == (0, 0, 0, 0), what
    for strategy in (0, 1):
        cfg = dict(n_nodes=8, seed=4, manager=1, strategy=strategy)
        plain, tried = _create(b, f"plain{strategy}", **cfg), _create(b, f"tried{strategy}", **cfg)
        assert _boot(b, plain) == _boot(b, tried)
        before = b.live()
        lines = [f"step {tried} 3", f"round_absorb {tried} <<>>"]
        lines += [" ".join([n, tried] + VALID[n]) for n in ("join_nif", "crash_nif", "revive_nif", "leave_nif",
                                                             "leave_node_nif", "omission_nif", "faulted_nif",
                                                             "set_phash_table_nif")]
        if strategy == 0:
            lines.append(f"members_nif {tried} 0 8")
        for line in lines:
            assert b.call("!fail alloc 1") == "ok"
            assert b.call(line) == OOM, line
            assert b.live() == before, line
        assert _after(b, plain) == _after(b, tried)
    # outbound's binary, with a round open; the round closes as it would have
    for k, h in enumerate((_create(b, "o1", n_nodes=8, seed=4), _create(b, "o2", n_nodes=8, seed=4))):
        _boot(b, h)
        assert b.call(f"round_emit {h}") == "ok"
        if k:
            assert b.call("!fail alloc_binary 1") == "ok"
            assert b.call(f"outbound {h}") == OOM
            assert b.live()[:2] == (0, 0)
    got = []
    for h in ("$o1", "$o2"):
        box = b.call(f"outbound {h}")
        assert box[0] == "ok" and len(box[1]) % 64 == 0 and len(box[1]) > 0
        got.append((box, b.call(f"round_absorb {h} {N.hexbin(box[1])}"), _after(b, h)))
    assert got[0] == got[1]
    # (the oracle stand-in answers snapshot/1 `unsupported` before any binary is made:
    # its failure point is reached on the GPU, tests/test_gpu_nif_run.py)
    assert b.call("!fail alloc_binary 1") == "ok"
    assert b.call("snapshot $o1") == ("error", "unsupported")
    assert b.call("!fail alloc_binary 0") == "ok"


def test_allocation_failures(exe):
    with N.Beam(exe) as b:
        case_allocation_failures(b)
        b.finish_clean()


def test_round_halves_equal_step(exe):
    """round_emit / outbound / round_absorb on a whole-range handle are one step/2 round"""
    with N.Beam(exe) as b:
        a, c = _create(b, "a", n_nodes=8, seed=4), _create(b, "c", n_nodes=8, seed=4)
        assert _boot(b, a) == _boot(b, c)
        assert b.call(f"outbound {a}") == ("error", "invalid state")
        assert b.call(f"round_absorb {a} <<>>") == ("error", "invalid state")
        for _ in range(5):
            assert b.call(f"round_emit {a}") == "ok"
            assert b.call(f"round_emit {a}") == ("error", "invalid state")
            box = b.call(f"outbound {a}")[1]
            row = b.call(f"round_absorb {a} {N.hexbin(box)}")
            assert row == ("ok", b.call(f"step {c} 1")[1][0])
        assert _after(b, a) == _after(b, c)
        b.finish_clean()


# ---------------------------------------------------------------- alignment
def alignment_script(aligned):
    """every binary-taking NIF, on a SCAMP v1, a full and a HyParView handle"""
    lines = [f"!align {aligned}"]
    for k, cfg in enumerate((dict(manager=1, strategy=1), dict(manager=1, strategy=0), dict(manager=0))):
        h = f"$h{k}"
        lines += [f"h{k} = create {N.erl(dict(cfg, n_nodes=8, seed=4))}",
                  f"set_bucket_table_nif {h} <<{'0f0e0d0c0b0a0908'}>>",
                  f"set_phash_table_nif {h} {N.hexbin(np.arange(8, dtype=np.uint32)[::-1].tobytes())}",
                  f"join_nif {h} {N.pack([0])} {N.pack([N.NONE])}", f"step {h} 1",
                  f"join_nif {h} {N.pack(range(1, 8))} {N.pack(range(0, 7))}", f"step {h} 10",
                  f"crash_nif {h} {N.pack([3, 4])}", f"leave_nif {h} {N.pack([5])}", f"step {h} 2",
                  f"revive_nif {h} {N.pack([3])}", f"leave_node_nif {h} {N.pack([1])} {N.pack([2])}",
                  f"omission_nif {h} 0 {N.pack([0, 1])} {N.pack([1, 0])} 1",
                  f"omission_nif {h} 1 {N.pack([6])} {N.pack([7])} 1", f"faulted_nif {h} {N.pack([7])} 1",
                  f"set_partition_nif {h} <<0000000001010101>>", f"step {h} 4",
                  f"graph_metrics_nif {h} {N.pack([0, 1])} 0", f"restore {h} <<0001020304>>",
                  f"round_emit {h}", f"box{k} = outbound {h}", f"round_absorb {h} $box{k}", f"step {h} 3"]
        lines += [f"node_nif {h} {i}" for i in range(8)] + [f"members_nif {h} {i} 8" for i in range(8)]
    return lines


def test_alignment(exe):
    """odd-address and aligned binaries give the same results"""
    runs = []
    for aligned in (0, 1):
        rc, out, err = N.run_script(exe, alignment_script(aligned))
        assert rc == 0 and err == "" and out[-1] == "{exit,clean}", (rc, err, out[-3:])
        runs.append(out)
    assert runs[0] == runs[1]
    assert sum(x.startswith("{ok,") for x in runs[0]) > 50 and runs[0].count("ok") > 30


# ---------------------------------------------------------------- equivalence
SMALL = [(k, s) for k, s in R.CORPUS if _schedule(k, s).n <= 257]


def test_the_small_corpus_covers_every_kind():
    assert {k for k, _ in SMALL} == set(R.KINDS) and len(SMALL) >= 25


@pytest.mark.parametrize("kind,seed", SMALL, ids=[f"{k}-{s}" for k, s in SMALL])
def test_equivalence(exe, kind, seed):
    """execute + project: the shim's trace equals the oracle's"""
    sch, want = _want(kind, seed)
    N.same(_through_the_shim(exe, sch), want)


class _Turn:
    """two drivers of one child, strictly alternating call by call"""

    def __init__(self, beam):
        self.beam, self.cv, self.turn, self.alive, self.switches = beam, threading.Condition(), 0, [True, True], 0

    def side(self, k):
        outer = self

        class Side:
            def name(self, stem="v"):
                return outer.beam.name(stem)

            def calls(self, lines):
                with outer.cv:
                    outer.cv.wait_for(lambda: outer.turn == k or not outer.alive[1 - k])
                    try:
                        return outer.beam.calls(lines)
                    finally:
                        if outer.alive[1 - k]:
                            outer.turn = 1 - k
                            outer.switches += 1
                        outer.cv.notify_all()

            def call(self, line):
                return self.calls([line])[0]

            def raw(self, lines):
                return outer.beam.raw(lines)

        return Side()

    def done(self, k):
        with self.cv:
            self.alive[k] = False
            self.cv.notify_all()


def test_two_handles_interleaved(exe):
    """two handles alive at once in one program equal their separate runs"""
    pair = (("hv", 2), ("scamp_v1", 2))
    with N.Beam(exe) as b:
        turn, got, errs = _Turn(b), [None, None], []

        def work(k):
            try:
                got[k] = R.execute(N.nif_make(turn.side(k)), _schedule(*pair[k]))
            except BaseException as e:          # noqa: B902 (handed to the test's thread)
                errs.append(e)
            finally:
                turn.done(k)

        ts = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errs:
            raise errs[0]
        assert turn.switches > 300
        b.finish_clean()
    for k in (0, 1):
        N.same(got[k], _want(*pair[k])[1])


# ---------------------------------------------------------------- the sanitized build
# (LeakSanitizer stops the world through ptrace, which a confined user may not be allowed; what the
# shim could leak is counted by the stand-in runtime's own accounting at exit)
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU machine (/dev/kfd): the sanitized program runs on CPU-only machines")
def test_sanitized_program_runs_clean(tmp_path):
    """The same program under -fsanitize=address,undefined, the oracle's
    source compiled in (no shared library, nothing preloaded): the argument,
    busy, allocation-failure and alignment scripts and three schedules exit 0
    with nothing on stderr."""
    exe = N.build(tmp_path, sanitize=True)
    for case in (case_argument_checks, case_busy_injected, case_allocation_failures,
                 lambda b: N.busy_two_threads(b, Oracle, rounds=120)):
        with N.Beam(exe, env=SAN_ENV, timeout=120.0) as b:
            case(b)
            b.finish_clean()
    for aligned in (0, 1):
        rc, out, err = N.run_script(exe, alignment_script(aligned), env=SAN_ENV, timeout=120.0)
        assert rc == 0 and err == "" and out[-1] == "{exit,clean}", (rc, err[-3000:], out[-3:])
    for kind, seed in (("hv", 2), ("scamp_v1", 2), ("full", 4)):
        sch, want = _want(kind, seed)
        with N.Beam(exe, env=SAN_ENV, timeout=120.0) as b:
            got = R.execute(N.nif_make(b), sch)
            b.finish_clean()
        N.same(got, want)
