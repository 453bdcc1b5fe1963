"""The corpus of seeded random schedules (tests/_random_schedule.py; what it
reaches: tests/test_random_schedule.py) on the GPU against the oracle, bit for
bit: every round's stats, the return code of every event call (refusals
included), every probe over its window, and the final state.

test_entry            every entry on one local shard.  ("snapshot_restore",)
                      is honoured: snapshot, a second handle with the same
                      config and tables, restore into it, close the first, go
                      on with the second.  The oracle ignores the step.
test_entry_paths      three entries a kind over 3 and 7 virtual shards (7
                      divides none of the sizes: uneven last shards), three
                      loopback ranks and a one-rank RCCL communicator.
                      Full-membership handles have one shard and no ranks
                      (psim_create refuses more): theirs run on the RCCL
                      communicator alone.  That path ignores the restore step
                      (one communicator a process); the others honour it.
test_entry_host_exchange  two entries a kind except `full`, in their host form
                      (generated with host=True: no leave_node, no histogram
                      probe), the engine as ranks 1 and 2 of 4 beside oracle
                      shards: every ("step", k) is k emit/absorb rounds, each
                      round's exchange must equal the all-oracle exchange's.
test_knobs            one child process a knob set (the knobs are read once
                      per process): tests/_random_schedule_run.py.
test_regressions      every fixture of tests/golden/random_regressions/ (the
                      shrunk schedule of a disagreement found and fixed) on
                      every path.

Oracle traces are computed once per entry and left unchanged."""
import functools
import glob
import os
import subprocess
import sys

import pytest

import _random_schedule as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [f"{k}-{s}" for k, s in R.CORPUS]


@functools.lru_cache(maxsize=None)
def _oracle(kind, seed, host=False):
    sch = R.generate(kind, seed, host=host)
    return sch, R.execute(R.oracle_make, sch)


def _run(path, sch, ref):
    make, opts = R.path(path, sch.kind)
    tr = R.execute(make, sch, opts)
    R.compare(tr, ref)
    return tr


@pytest.mark.parametrize("kind,seed", R.CORPUS, ids=IDS)
def test_entry(kind, seed):
    sch, ref = _oracle(kind, seed)
    tr = _run("local", sch, ref)
    assert tr.restored == sum(1 for s in sch.steps if s[0] == "snapshot_restore") >= 1


PATH_ENTRIES = [(p, k, s) for k in R.KINDS for s in R.CORPUS_SEEDS[k][2:5] for p in R.paths_of(k)]


@pytest.mark.parametrize("path,kind,seed", PATH_ENTRIES, ids=[f"{p}-{k}-{s}" for p, k, s in PATH_ENTRIES])
def test_entry_paths(path, kind, seed):
    sch, ref = _oracle(kind, seed)
    tr = _run(path, sch, ref)
    assert len(tr.probes) == len(ref.probes)         # (no probe kind had to be dropped on these paths)
    assert path == "rccl1" or tr.restored >= 1


HOST_ENTRIES = [(k, s) for k in R.KINDS if k != "full" for s in R.CORPUS_SEEDS[k][:2]]


@functools.lru_cache(maxsize=None)
def _all_oracle_exchange(kind, seed):
    """the expected exchange: the engine's ranks played by oracle shards; that
    run itself equals the unsharded oracle's"""
    sch, ref = _oracle(kind, seed, True)
    holder = []
    tr = R.execute(R.hybrid_make(engine=False, holder=holder), sch, R.path("oracle-sharded")[1])
    R.compare(tr, ref)
    assert holder[0].n_out > 0 and holder[0].n_in > 0
    return holder[0].trace


@pytest.mark.parametrize("kind,seed", HOST_ENTRIES, ids=[f"{k}-{s}" for k, s in HOST_ENTRIES])
def test_entry_host_exchange(kind, seed):
    sch, ref = _oracle(kind, seed, True)
    assert not any(s[0] == "call" and s[1] == "leave_node" or s[0] == "probe" and s[1] == "histograms" for s in sch.steps)
    holder = []
    opts = R.path("host-exchange")[1]
    tr = R.execute(R.hybrid_make(expect=_all_oracle_exchange(kind, seed), holder=holder), sch, opts)
    R.compare(tr, ref)
    assert holder[0].resumed and tr.restored >= 1


# test_gpu_knobs.py's sets; PSIM_PTL_EARLY 1 and 2 (test_gpu_ptl_early.py);
# PSIM_PREP_FUSED off and on (test_gpu_prep_fused.py); the lite kernel's half
# selection -- the quarter one is the default, the first set --
# (test_gpu_lite_quarter.py) and k_hv_phase's (test_gpu_phase_fused.py)
KNOBS = {
    "default": {},
    "wshift12": {"PSIM_ROUTE_WSHIFT": "12"},
    "route_reg0": {"PSIM_ROUTE_REG": "0", "PSIM_ROUTE_BLOCKS": "7"},
    "lite_wave": {"PSIM_LITE_WAVE": "1"},
    "grids": {"PSIM_LITE_GRID": "x1", "PSIM_PTL_GRID": "x2", "PSIM_PT_GRID": "x2", "PSIM_CONSUME_GRID": "x2"},
    "concurrent": {"PSIM_CONCURRENT_PHASE": "1"},
    "ptl_grid": {"PSIM_PTL_GRID": "x1"},
    "route_fused0": {"PSIM_ROUTE_FUSED": "0"},
    "no_rank_batch_loopback3": {"PSIM_NO_RANK_BATCH": "1", "PSIM_KNOB_PATH": "loopback3"},
    "no_rank_batch_rccl1": {"PSIM_NO_RANK_BATCH": "1", "PSIM_KNOB_PATH": "rccl1"},
    "rccl1": {"PSIM_KNOB_PATH": "rccl1"},
    "loopback3": {"PSIM_KNOB_PATH": "loopback3"},
    "early1": {"PSIM_PTL_EARLY": "1"},
    "early2": {"PSIM_PTL_EARLY": "2"},
    "prep_fused0": {"PSIM_PREP_FUSED": "0"},
    "prep_fused1": {"PSIM_PREP_FUSED": "1"},
    "lite_half": {"PSIM_LITE_HALF": "1"},
    "phase_fused0": {"PSIM_PHASE_FUSED": "0"},
    "phase_fused2": {"PSIM_PHASE_FUSED": "2"},
    "phase_fused3": {"PSIM_PHASE_FUSED": "3"},
}
OURS = sorted({k for v in KNOBS.values() for k in v})


@pytest.mark.parametrize("knobs", list(KNOBS))
def test_knobs(knobs):
    env = {k: v for k, v in os.environ.items() if k not in OURS}
    env.update(KNOBS[knobs])
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_random_schedule_run.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout


def test_regressions():
    """every fixture on every path its kind has (none yet: the corpus and the
    search beyond it found no disagreement)"""
    for name in sorted(glob.glob(os.path.join(HERE, "golden", "random_regressions", "*.json"))):
        with open(name) as f:
            sch = R.Schedule.from_json(f.read())
        ref = R.execute(R.oracle_make, sch)
        for path in ("local",) + R.paths_of(sch.kind):
            _run(path, sch, ref)
