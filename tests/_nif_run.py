"""Runs the Erlang NIF shim (erlang/c_src/partisan_gpu_sim_nif.c) without
Erlang: builds tests/nif_run's driver program -- the shim over a stand-in
erl_nif runtime, with the CPU oracle or the HIP library behind it -- starts it
as a child process, sends it script lines and parses the Erlang terms it
prints.

NifSim drives one handle of such a child with the method surface that
tests/_random_schedule.execute expects, packing every argument as
erlang/src/partisan_gpu_sim.erl does.  project(trace) reduces a Trace of the
oracle called directly to what the NIF surface can show, so that the two can
be compared with same().  Test infrastructure only."""
import os
import re
import subprocess
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from partisan_amd import _abi  # noqa: E402
from partisan_amd.sim import SimError  # noqa: E402

NIF_RUN = os.path.join(HERE, "nif_run")
# (PSIM_NIF_SHIM: another source in the shim's place, for trying a deliberate break on a scratch copy)
SHIM = os.environ.get("PSIM_NIF_SHIM") or os.path.join(ROOT, "erlang", "c_src", "partisan_gpu_sim_nif.c")
ORACLE_SRC = os.path.join(ROOT, "oracle", "psim_oracle.c")
LIB_DIR = os.path.join(ROOT, "partisan_amd", "csrc")
NONE = 0xFFFFFFFF

# psim_strerror's texts (include/partisan_gpu_sim.h's codes): the atoms of {error, Atom}
STRERROR = {
    0: "ok", -1: "invalid argument", -2: "out of memory", -3: "HIP runtime error", -4: "invalid state",
    -5: "node id out of range", -6: "communication error", -7: "unsupported", -8: "a fixed table overflowed (strict)",
}
# psim_config's fields that are no part of the protocol: create/1 has no key for them
EXECUTION_FIELDS = ("abi_version", "device", "n_shards", "shard_rank", "shard_world", "comm_id", "max_msgs_per_round",
                    "reserved1")
CONFIG_KEYS = tuple(name for name, _ in _abi.PsimConfig._fields_ if name not in EXECUTION_FIELDS)
NIF_STATS_DTYPE = np.dtype([("round", np.uint64), ("emitted", np.uint64), ("delivered", np.uint64),
                            ("first_deliveries", np.uint64)])


# ---------------------------------------------------------------- the build
def have_gcc():
    try:
        return subprocess.run(["gcc", "--version"], capture_output=True).returncode == 0
    except OSError:
        return False


def build(out_dir, backend="oracle", sanitize=False, shim=SHIM):
    """The driver program in out_dir.  backend "oracle": the oracle's source
    is compiled into the executable; "gpu": linked against the HIP library.
    Returns the program's path."""
    exe = os.path.join(str(out_dir), "beam_" + backend + ("_san" if sanitize else ""))
    cmd = ["gcc", "-std=gnu11", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror",
           "-I", os.path.join(HERE, "nif_lint"), "-I", NIF_RUN, "-I", os.path.join(ROOT, "include")]
    cmd += ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    cmd += ["-o", exe, os.path.join(NIF_RUN, "beam_main.c"), os.path.join(NIF_RUN, "fake_erts.c"), shim]
    if backend == "oracle":
        cmd += [os.path.join(NIF_RUN, "psim_on_oracle.c"), ORACLE_SRC]
    else:
        assert backend == "gpu" and not sanitize
        cmd += ["-L", LIB_DIR, "-lpartisan_gpu_sim", "-Wl,-rpath," + LIB_DIR, "-Wl,--allow-shlib-undefined"]
    cmd += ["-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# ---------------------------------------------------------------- the terms
_TOKEN = re.compile(r"\s*(?:(\d+)|([a-z][A-Za-z0-9_@]*)|'((?:[^'\\]|\\.)*)'|<<([0-9a-f]*)>>|(#\{|=>|[{}\[\],]))")


def parse_term(text):
    """Erlang term text -> int, str (atom), bytes, tuple, list, dict"""
    pos = 0

    def tok():
        nonlocal pos
        m = _TOKEN.match(text, pos)
        if not m:
            raise ValueError(f"not a term at {pos}: {text[pos:pos + 40]!r}")
        pos = m.end()
        return m

    def seq(close):
        out = []
        m = tok()
        if m.group(5) == close:
            return out
        while True:
            out.append(term(m))
            m = tok()
            if m.group(5) == close:
                return out
            assert m.group(5) == ",", text[pos - 5:pos + 20]
            m = tok()

    def term(m):
        if m.group(1) is not None:
            return int(m.group(1))
        if m.group(2) is not None:
            return m.group(2)
        if m.group(3) is not None:
            return re.sub(r"\\(.)", r"\1", m.group(3))
        if m.group(4) is not None:
            return bytes.fromhex(m.group(4))
        p = m.group(5)
        if p == "{":
            return tuple(seq("}"))
        if p == "[":
            return seq("]")
        assert p == "#{", p
        out = {}
        m = tok()
        if m.group(5) == "}":
            return out
        while True:
            k = term(m)
            assert tok().group(5) == "=>"
            assert k not in out
            out[k] = term(tok())
            m = tok()
            if m.group(5) == "}":
                return out
            assert m.group(5) == ","
            m = tok()

    t = term(tok())
    assert text[pos:].strip() == "", text[pos:pos + 40]
    return t


def hexbin(data):
    return "<<" + bytes(data).hex() + ">>"


def pack(ids):
    """partisan_gpu_sim:pack/1: little-endian u32"""
    return hexbin(np.ascontiguousarray(ids, np.uint32).astype("<u4").tobytes())


def erl(v):
    """a Python value as script text"""
    if isinstance(v, dict):
        return "#{" + ", ".join(f"{k} => {erl(x)}" for k, x in v.items()) + "}"
    if isinstance(v, (bytes, bytearray)):
        return hexbin(v)
    if isinstance(v, (list, tuple)):
        inner = ", ".join(erl(x) for x in v)
        return "{" + inner + "}" if isinstance(v, tuple) else "[" + inner + "]"
    if isinstance(v, str):
        return v
    return str(int(v))


# ---------------------------------------------------------------- the child
class Beam:
    """One run of the driver program.  Every child carries its own timeout: a
    watchdog kills it, and the pending read then ends."""

    BATCH = 32      # lines written before their answers are read (well under a pipe's buffer)

    def __init__(self, exe, timeout=60.0, env=None):
        e = dict(os.environ)
        e.update(env or {})
        self.proc = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                     env=e)
        self.timed_out = False
        self._dog = threading.Timer(timeout, self._kill)
        self._dog.daemon = True
        self._dog.start()
        self._names = 0
        self.stderr = b""
        self.returncode = None

    def _kill(self):
        self.timed_out = True
        self.proc.kill()

    def name(self, stem="v"):
        self._names += 1
        return f"{stem}{self._names}"

    def raw(self, lines):
        out = []
        for at in range(0, len(lines), self.BATCH):
            part = lines[at:at + self.BATCH]
            assert all("\n" not in x for x in part)
            try:
                self.proc.stdin.write(("\n".join(part) + "\n").encode())
                self.proc.stdin.flush()
            except (BrokenPipeError, OSError):
                self._dead(part[0])
            for x in part:
                ans = self.proc.stdout.readline()
                if not ans.endswith(b"\n"):
                    self._dead(x)
                out.append(ans[:-1].decode())
        return out

    def _dead(self, line):
        self.finish()
        raise AssertionError(f"the driver program ended (status {self.returncode}, timed out: {self.timed_out}) "
                             f"at: {line[:200]}\n{self.stderr.decode(errors='replace')[-4000:]}")

    def calls(self, lines):
        return [parse_term(x) for x in self.raw(lines)]

    def call(self, line):
        return self.calls([line])[0]

    def live(self):
        """(enif_alloc blocks, owned binaries, resources, mutexes) alive now"""
        t = self.call("!live")
        assert t[0] == "live"
        return tuple(t[1:])

    def finish(self):
        """End of script.  Returns (exit status, the last stdout lines, stderr)."""
        if self.returncode is None:
            try:
                out, err = self.proc.communicate()
            except ValueError:
                out, err = b"", b""
            self._dog.cancel()
            self.returncode, self.stderr, self.tail = self.proc.returncode, err, out.decode().splitlines()
        return self.returncode, self.tail, self.stderr

    def finish_clean(self):
        """every term dropped, nothing left alive, nothing on stderr (but the HIP
        library's own notes, `psim: ...`, such as an outbox that grew)"""
        rc, tail, err = self.finish()
        assert not self.timed_out, "the driver program ran into its timeout"
        stray = [x for x in err.decode(errors="replace").splitlines() if not x.startswith("psim: ")]
        assert rc == 0 and tail[-1:] == ["{exit,clean}"] and not stray, (rc, tail[-3:], stray[-40:])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.returncode is None:
            self.proc.kill()
            self.finish()


def run_script(exe, lines, timeout=60.0, env=None):
    """A whole script at once (no interaction).  Returns (status, answers, stderr)."""
    p = subprocess.run([exe], input=("\n".join(lines) + "\n").encode(), capture_output=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout.decode().splitlines(), p.stderr.decode(errors="replace")


# ---------------------------------------------------------------- the driver
def config_map(cfg, **extra):
    """every protocol key of create/1 from a psim_config"""
    m = {k: int(getattr(cfg, k)) for k in CONFIG_KEYS}
    m.update(extra)
    return m


class NifError(SimError):
    pass


def _raise(ans, what):
    e = NifError(f"{what}: {ans}")
    e.rc = ans[1] if isinstance(ans, tuple) and len(ans) == 2 and ans[0] == "error" else ans
    raise e


class NifSim:
    """A handle of a Beam child, driven through the NIFs alone."""

    def __init__(self, beam, cfg, **extra):
        self.beam, self.cfg, self.n = beam, cfg, int(cfg.n_nodes)
        self.h = "$" + beam.name("h")
        ans = beam.call(f"{self.h[1:]} = create {erl(config_map(cfg, **extra))}")
        if not (isinstance(ans, tuple) and ans[0] == "ok"):
            _raise(ans, "create")
        self.full = cfg.manager == _abi.MANAGER_PLUGGABLE and cfg.strategy == _abi.STRATEGY_FULL
        self.stepped = 0

    def close(self):
        pass            # (the child drops every term when its script ends, and checks that the handle went)

    def _ok(self, line, what):
        ans = self.beam.call(line)
        if ans != "ok":
            _raise(ans, what)

    def _get(self, lines, what):
        out = []
        for ans in self.beam.calls(lines):
            if not (isinstance(ans, tuple) and len(ans) == 2 and ans[0] == "ok"):
                _raise(ans, what)
            out.append(ans[1])
        return out

    # ---- events, packed as partisan_gpu_sim.erl packs them
    def join(self, nodes, contacts): self._ok(f"join_nif {self.h} {pack(nodes)} {pack(contacts)}", "join")
    def crash(self, nodes): self._ok(f"crash_nif {self.h} {pack(nodes)}", "crash")
    def revive(self, nodes): self._ok(f"revive_nif {self.h} {pack(nodes)}", "revive")
    def leave(self, nodes): self._ok(f"leave_nif {self.h} {pack(nodes)}", "leave")
    def leave_node(self, a, t): self._ok(f"leave_node_nif {self.h} {pack(a)} {pack(t)}", "leave_node")
    def broadcast(self, root, msg_id): self._ok(f"broadcast_nif {self.h} {int(root)} {int(msg_id)}", "broadcast")
    def clear_partition(self): self._ok(f"clear_partition_nif {self.h}", "clear_partition")
    def resolve_all_faults(self): self._ok(f"clear_faults_nif {self.h}", "clear_faults")

    def set_partition(self, group):
        self._ok(f"set_partition_nif {self.h} {hexbin(np.ascontiguousarray(group, np.uint8).tobytes())}", "set_partition")

    def set_bucket_table(self, buckets):
        self._ok(f"set_bucket_table_nif {self.h} {hexbin(np.ascontiguousarray(buckets, np.uint8).tobytes())}",
                 "set_bucket_table")

    def set_phash_table(self, phash):
        # <<H:32/native>>
        self._ok(f"set_phash_table_nif {self.h} {hexbin(np.ascontiguousarray(phash, np.uint32).tobytes())}",
                 "set_phash_table")

    def _omission(self, kind, s, d, on):
        self._ok(f"omission_nif {self.h} {kind} {pack(np.atleast_1d(s))} {pack(np.atleast_1d(d))} {on}", "omission")

    def begin_send_omission(self, s, d): self._omission(0, s, d, 1)
    def end_send_omission(self, s, d): self._omission(0, s, d, 0)
    def begin_receive_omission(self, s, d): self._omission(1, s, d, 1)
    def end_receive_omission(self, s, d): self._omission(1, s, d, 0)
    def begin_omission(self, nodes): self._ok(f"faulted_nif {self.h} {pack(np.atleast_1d(nodes))} 1", "faulted")
    def end_omission(self, nodes): self._ok(f"faulted_nif {self.h} {pack(np.atleast_1d(nodes))} 0", "faulted")

    # ---- rounds
    def step(self, n_rounds=1):
        rows = self._get([f"step {self.h} {int(n_rounds)}"], "step")[0]
        self.stepped += len(rows)
        return np.array([tuple(r) for r in rows], NIF_STATS_DTYPE)

    def emit(self): self._ok(f"round_emit {self.h}", "round_emit")

    def outbound(self):
        b = self._get([f"outbound {self.h}"], "outbound")[0]
        return np.frombuffer(b, np.uint32).reshape(-1, 16).copy()

    def absorb(self, recs):
        r = np.ascontiguousarray(recs, np.uint32).reshape(-1, 16)
        row = self._get([f"round_absorb {self.h} {hexbin(r.tobytes())}"], "round_absorb")[0]
        self.stepped += 1
        return np.array([tuple(row)], NIF_STATS_DTYPE)

    # ---- inspection: what node/2, active/2, members/3, delivery/2 show
    @property
    def round(self):
        """node/2's round where the handle answers node/2, else the rounds stepped"""
        ans = self.beam.call(f"node_nif {self.h} 0")
        if isinstance(ans, tuple) and ans[0] == "ok":
            return ans[1]["round"]
        return self.stepped

    def nodes(self, first=0, count=None):
        count = self.n - first if count is None else count
        ids = range(first, first + count)
        rows = self._get([f"node_nif {self.h} {i}" for i in ids], "node")
        act = self._get([f"active_nif {self.h} {i}" for i in ids], "active")
        out = []
        for m, a in zip(rows, act):
            assert sorted(m) == ["active", "epoch", "have", "passive", "round", "up"], sorted(m)
            out.append((m["up"], m["epoch"], tuple(m["active"]), tuple(m["passive"]), m["have"], m["round"], tuple(a)))
        return out

    def strategy_nodes(self, first=0, count=None):
        count = self.n - first if count is None else count
        mem = self._get([f"members_nif {self.h} {i} {self.n}" for i in range(first, first + count)], "members")
        return [(len(m),) if self.full else tuple(m) for m in mem]

    def member_bits(self, node):
        return list(self._get([f"members_nif {self.h} {int(node)} {self.n}"], "members")[0])

    def delivery(self, first=0, count=None):
        count = self.n - first if count is None else count
        rows = self._get([f"delivery_nif {self.h} {i}" for i in range(first, first + count)], "delivery")
        assert all(r[0] in ("true", "false") for r in rows)
        return (np.array([r[0] == "true" for r in rows], np.uint8), np.array([r[1] for r in rows], np.uint32),
                np.array([r[2] for r in rows], np.uint32))

    def msg_slots(self):
        ids, roots = np.full(_abi.MSG_SLOTS, NONE, np.uint32), np.zeros(_abi.MSG_SLOTS, np.uint32)
        last = -1
        for slot, msg, root in self._get([f"msg_slots_nif {self.h}"], "msg_slots")[0]:
            assert last < slot < _abi.MSG_SLOTS
            last = slot
            ids[slot], roots[slot] = msg, root
        return ids, roots

    def histograms(self):
        m = self._get([f"histograms {self.h}"], "histograms")[0]
        return {k: np.array(v, np.uint64) if isinstance(v, list) else int(v) for k, v in m.items()}

    def strategy_histograms(self):
        m = self._get([f"strategy_histograms {self.h}"], "strategy_histograms")[0]
        return {k: np.array(v, np.uint64) if isinstance(v, list) else int(v) for k, v in m.items()}

    def graph_metrics(self, sources, max_levels=0):
        m = self._get([f"graph_metrics_nif {self.h} {pack(sources)} {int(max_levels)}"], "graph_metrics")[0]
        return {k: np.array(v, np.uint64) if isinstance(v, list) else int(v) for k, v in m.items()}

    # ---- snapshot: the binary stays in the child, under a name
    def snapshot(self):
        name = self.beam.name("snap")
        ans = self.beam.raw([f"{name} = snapshot {self.h}"])[0]
        if not ans.startswith("{ok,<<"):
            _raise(parse_term(ans), "snapshot")
        return "$" + name

    def restore(self, snap):
        self._ok(f"restore {self.h} {snap if isinstance(snap, str) else hexbin(snap)}", "restore")
        return self


def nif_make(beam, sims=None):
    def make(cfg):
        sim = NifSim(beam, cfg)
        if sims is not None:
            sims.append(sim)
        return sim
    return make


def restore_in_child(sim, fresh):
    """snapshot/1 into restore/2 of a second handle of the same program"""
    snap = sim.snapshot()
    other = fresh()
    other.restore(snap)
    other.stepped = sim.stepped
    return other


# ---------------------------------------------------------------- the projection
def _rc(rc):
    return 0 if rc == 0 else STRERROR[rc]


def _node_rows(rows, rnd):
    out = []
    for v in rows:
        act = tuple(int(x) for x in v["act"][: v["act_n"]])
        out.append(("true" if v["up"] else "false", int(v["epoch"]), act,
                    tuple(int(x) for x in v["pas"][: v["pas_n"]]), int(v["have"]), int(rnd), act))
    return out


def _bits(words):
    return [int(i) for i in np.nonzero(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8),
                                                     bitorder="little"))[0]]


def _project(what, res, rnd, full):
    if what == "nodes":
        return _node_rows(res, rnd)
    if what == "strategy_nodes":
        return [(int(v["members"]),) if full else tuple(int(x) for x in v["view"][: v["view_n"]]) for v in res]
    if what.startswith("member_bits"):
        return _bits(res)
    if what == "msg_slots":
        ids, roots = res
        return ids.copy(), np.where(ids == NONE, 0, roots & ~np.uint32(_abi.PSIM_MAP_BIT)).astype(np.uint32)
    return res           # delivery, histograms, round: as the NIFs show them


def project(trace):
    """An oracle Trace reduced to what the NIF surface can show: per round
    (round, sum of emitted, sum of delivered, first_deliveries); return codes
    as psim_strerror's atoms; node/2's six fields and active/2; members/3;
    delivery/2; the histograms/1 map; msg_slots/1 without PSIM_MAP_BIT."""
    from _random_schedule import Trace
    full = trace.schedule.kind == "full"
    t = Trace(trace.schedule)
    st = trace.stats
    t.stats = np.zeros(len(st), NIF_STATS_DTYPE)
    t.stats["round"], t.stats["first_deliveries"] = st["round"], st["first_deliveries"]
    t.stats["emitted"], t.stats["delivered"] = st["emitted"].sum(1), st["delivered"].sum(1)
    t.rcs = [(i, name, _rc(rc)) for i, name, rc in trace.rcs]
    t.probes = [(i, what, first, count, rnd, _project(what, res, rnd, full))
                for i, what, first, count, rnd, res in trace.probes]
    last = int(st["round"][-1]) + 1 if len(st) else 0
    t.final = {k: _project(k, v, last, full) for k, v in trace.final.items()}
    return t


def _eq(where, a, b):
    if isinstance(a, dict) or isinstance(b, dict):
        assert isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b), f"{where}: keys {sorted(a)} against {sorted(b)}"
        for k in a:
            _eq(f"{where}.{k}", a[k], b[k])
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert a.shape == b.shape, f"{where}: shape {a.shape} against {b.shape}"
        if a.dtype.names:
            assert a.dtype.names == b.dtype.names, where
            for f in a.dtype.names:
                _eq(f"{where}.{f}", a[f], b[f])
        else:
            assert np.array_equal(a, b), f"{where}: differs at {np.nonzero(a != b)[0][:8].tolist()}: " \
                f"{a[a != b][:4].tolist()} against {b[a != b][:4].tolist()}"
    elif isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), f"{where}: {len(a)} entries against {len(b)}"
        for k, (x, y) in enumerate(zip(a, b)):
            _eq(f"{where}[{k}]", x, y)
    else:
        assert type(a) is type(b) or (isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer))), \
            f"{where}: {a!r} against {b!r}"
        assert a == b, f"{where}: {a!r} against {b!r}"


def same(a, b, skip_probes=()):
    """Trace a (through the shim) against b = project(the oracle's trace):
    exact in every round, return code, probe and final field."""
    tag = f"schedule {a.schedule.kind} seed {a.schedule.seed}"
    _eq(f"{tag}: stats", a.stats, b.stats)
    _eq(f"{tag}: return codes", a.rcs, b.rcs)
    pa = [p for p in a.probes if p[1] not in skip_probes]
    pb = [p for p in b.probes if p[1] not in skip_probes]
    assert len(pa) == len(pb), f"{tag}: {len(pa)} probes against {len(pb)}"
    for x, y in zip(pa, pb):
        assert x[:5] == y[:5], f"{tag}: probe {x[:5]} against {y[:5]}"
        _eq(f"{tag}: probe {x[1]} [{x[2]}, {x[2] + x[3]}) at step {x[0]}", x[5], y[5])
    assert sorted(a.final) == sorted(b.final), (sorted(a.final), sorted(b.final))
    for k in a.final:
        _eq(f"{tag}: final {k}", a.final[k], b.final[k])


# ---------------------------------------------------------------- busy, with a real second thread
BUSY_CFG = dict(n_nodes=257, seed=3, shuffle_period=1, promotion_period=1)
BUSY_ROUNDS = 500          # about a second of the oracle alone at these periods (2 ms a round)


def busy_two_threads(b, make_oracle, rounds=BUSY_ROUNDS, node=5):
    """a second thread inside step; the main thread polls node_nif: every
    answer is {error, busy} or the oracle's row at a round boundary"""
    from partisan_amd.sim import default_config
    cfg = default_config(**BUSY_CFG)
    sim = NifSim(b, cfg)
    o = make_oracle(type(cfg).from_buffer_copy(cfg))
    rows = {}
    for s in (sim, o):
        s.join([0], [NONE])
        s.step(1)
        s.join(list(range(1, 257)), list(range(0, 256)))
        s.step(20)
    r0 = int(o.round)
    rows[r0] = _node_rows(o.nodes(node, 1), r0)[0][:6]
    o.step(rounds)
    rows[r0 + rounds] = _node_rows(o.nodes(node, 1), r0 + rounds)[0][:6]
    o.close()
    assert b.raw([f"spawn s step {sim.h} {rounds}"]) == ["spawned"]
    n_busy = n_rows = 0
    for _ in range(2000000):
        ans = b.call(f"node_nif {sim.h} {node}")
        if ans == ("error", "busy"):
            n_busy += 1
            continue
        m = ans[1]
        assert ans[0] == "ok" and m["round"] in rows, ans
        assert (m["up"], m["epoch"], tuple(m["active"]), tuple(m["passive"]), m["have"], m["round"]) == rows[m["round"]]
        n_rows += 1
        if m["round"] == r0 + rounds:
            break
    else:
        raise AssertionError("the step never ended")
    done = b.call("await s")
    assert done[0] == "ok" and len(done[1]) == rounds and done[1][-1][0] == r0 + rounds - 1
    print(f"busy answers {n_busy}, rows {n_rows}")
    assert n_busy > 0 and n_rows > 0, f"inconclusive: {n_busy} busy answers, {n_rows} rows"

