"""bench.py's plain run, --dump-outputs and --full.

CPU: dump_outputs() over the oracle (float64 files, exact values, a sample
fixed by the node range alone) and the --dry-run launcher's dump.  GPU: one
small plain run twice (same arrays both times, exactly --steps stats rows,
none of --full's parts in the line) and one small --full run (they are
there)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)

FULL_ONLY = ("cpu_baseline", "check", "overlay", "device_mem_used_gb")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _check_dump(arrs, steps):
    assert arrs and all(a.dtype == np.float64 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert all(a.shape[0] == steps for k, a in arrs.items() if k.startswith("stats_"))
    assert np.array_equal(arrs["stats_round"], arrs["stats_round"][0] + np.arange(steps))
    k = len(arrs["nodes_id"])
    assert k and all(a.shape[0] == k for name, a in arrs.items() if name.startswith("nodes_"))


def test_dump_outputs_over_the_oracle(tmp_path):
    import bench
    from _oracle import Oracle
    from partisan_amd import workloads as W
    from partisan_amd.sim import default_config

    n, steps = 8192, 6
    o = Oracle(default_config(n_nodes=n, seed=3))
    boot = W.doubling_join(n, 3)
    o.run_schedule(boot, boot[-1][0] + 5)
    o.broadcast(0, 1)
    st = o.step(steps)
    bench.dump_outputs(str(tmp_path), st, o.nodes, 0, n)
    arrs = _load(str(tmp_path))
    _check_dump(arrs, steps)
    ids = arrs["nodes_id"].astype(np.int64)
    assert len(ids) == bench.DUMP_BLOCKS * bench.DUMP_BLOCK_NODES and len(set(ids)) == len(ids)
    assert ids.min() >= 0 and ids.max() < n
    rows = o.nodes()[ids]
    for f in rows.dtype.names:                       # every value exact, 64-bit patterns through their halves
        if f in bench.DUMP_WIDE:
            got = (arrs[f"nodes_{f}_hi"].astype(np.uint64) << np.uint64(32)) | arrs[f"nodes_{f}_lo"].astype(np.uint64)
        else:
            got = arrs[f"nodes_{f}"].astype(rows[f].dtype)
        assert np.array_equal(got, rows[f]), f
    dig = (arrs["stats_digest_hi"].astype(np.uint64) << np.uint64(32)) | arrs["stats_digest_lo"].astype(np.uint64)
    assert np.array_equal(dig, st["digest"])
    assert np.array_equal(arrs["stats_emitted"].astype(np.uint64), st["emitted"])
    # a range smaller than the sample: every node of it once, from its first
    small = tmp_path / "small"
    bench.dump_outputs(str(small), st, o.nodes, 100, 40)
    assert sorted(np.load(small / "nodes_id.npy").astype(int)) == list(range(100, 140))


def _bench(args, timeout=240):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dry_run_dumps_its_state(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        out = _bench(["--dry-run", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and "cpu_baseline" not in out
    x, y = np.load(a / "host_state.npy"), np.load(b / "host_state.npy")
    assert x.dtype == np.float64 and np.array_equal(x, y)


SMALL = ["--gpus", "1", "--nodes", "16384", "--steps", "7", "--warmup", "3"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_repeats(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    outs = [_bench(SMALL + ["--dump-outputs", str(d)]) for d in (a, b)]
    for out in outs:
        assert all(k in out for k in HEADLINE) and not any(k in out for k in FULL_ONLY)
        assert out["steps"] == 7 and out["warmup"] == 3 and out["n_gpus"] == 1
        assert out["unit"] == "node-rounds/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
        assert out["value"] == pytest.approx(16384 * 1e3 / out["ms_per_step"], rel=1e-9)
        assert out["conservation"]["ok"] and out["overflow"] == 0
    x, y = _load(str(a)), _load(str(b))
    _check_dump(x, 7)
    assert x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)
    assert x["stats_emitted"].sum() > 0 and x["nodes_up"].all()


@pytest.mark.gpu
def test_full_run_adds_the_rest():
    # (the CPU baseline is host work of minutes: bench.py --full without the flag runs it)
    out = _bench(SMALL + ["--full", "--no-cpu-baseline"])
    assert all(k in out for k in HEADLINE + FULL_ONLY[1:]) and "cpu_baseline" not in out
    assert out["steps"] == 7 and out["check"]["shards"] == 2 and out["overlay"]["rounds_drained"] >= 40
