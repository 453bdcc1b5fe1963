"""Config B's workload (bench.py --workload B: 100,000 nodes, the
full-membership strategy, fanout 5, periodic_interval 1) on 4 virtual shards
and on 4 loopback ranks of one GPU: what the payload exchange costs.

Per path, three handles one after the other (plain, timers, plain again: the
repeat shows what the order of the runs in one process does to the figure):
  plain    bootstrap + settle, warm-up, then WINDOWS timed windows of STEPS
           rounds (host clock around psim_step, which ends in a device
           synchronise): ms per round; the exchange counters over the windows:
           cross-shard records and bytes per round, rows shipped per round
           (bytes - 32 B a record, over the row bytes), the dedup ratio
           (cross-shard records per row)
  timers   the same with PSIM_PHASE_TIMERS=1 (event pairs around each phase
           put bubbles between kernels, so the plain handle gives the round
           time): psim_kernel_times of pay_pack (k_pay_pack alone), sort (the
           owner partition with mark / rank / rewrite) and exchange, and the
           copy kernel's achieved bytes/s = rows x row bytes x 2 (read and
           written) over its time

One JSON line per path on stdout.  Usage:
  python profiles/full_sharded/measure.py [--nodes N] [--steps K] [--windows W]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_TBS = 8.0          # MI355X HBM3E, spec; a float4 copy measures 6.29 TB/s


def make(path, cfg):
    if path.startswith("shards"):
        from partisan_amd import Simulator
        c = type(cfg).from_buffer_copy(cfg)
        c.device, c.n_shards = 0, int(path[6:])
        return Simulator(c)
    from _full_sharded import FullLoopbackRanks
    return FullLoopbackRanks(cfg, int(path[8:]))


def handles(sim):
    return sim.ranks if hasattr(sim, "ranks") else [sim]


def xstats(sim):
    r = b = 0
    for h in handles(sim):
        x = h.exchange_stats()
        r, b = r + x[0], b + x[1]
    return r, b


def run(path, args, timers):
    from partisan_amd import workloads as W
    from partisan_amd.sim import default_config
    if timers:
        os.environ["PSIM_PHASE_TIMERS"] = "1"
    else:
        os.environ.pop("PSIM_PHASE_TIMERS", None)
    n = args.nodes
    cfg = default_config(n_nodes=n, seed=args.seed, manager=1, strategy=0, fanout=5, periodic_interval=1)
    sim = make(path, cfg)
    try:
        boot = W.doubling_join(n, args.seed)
        sim.run_schedule(boot, boot[-1][0] + 1 + args.settle)
        sim.step(args.warmup)
        out = {"ms_per_round": [], "overflow": 0}
        r0, b0 = xstats(sim)
        kt = {}
        for _ in range(args.windows):
            t0 = time.perf_counter()
            st = sim.step(args.steps)
            out["ms_per_round"].append((time.perf_counter() - t0) / args.steps * 1e3)
            out["overflow"] += int(st["overflow"].sum())
            for h in handles(sim):
                for k, (ms, cnt) in h.kernel_times().items():
                    a = kt.setdefault(k, [0.0, 0])
                    a[0] += ms
                    a[1] += cnt
        r1, b1 = xstats(sim)
        rounds = args.windows * args.steps
        fw = ((n + 31) // 32 + 3) & ~3
        recs, nbytes = r1 - r0, b1 - b0
        assert (nbytes - 32 * recs) % (4 * fw) == 0
        rows = (nbytes - 32 * recs) // (4 * fw)
        out.update(records_per_round=recs / rounds, bytes_per_record=nbytes / max(1, recs),
                   rows_per_round=rows / rounds, records_per_row=recs / max(1, rows), row_bytes=4 * fw,
                   members_min=int(sim.strategy_nodes(0, min(n, 4096))["members"].min()))
        if timers:
            # (summed over the shards or ranks, which share the device: per round)
            out["kernel_ms_per_round"] = {k: v[0] / rounds for k, v in kt.items() if v[1]}
            out["kernel_launches_per_round"] = {k: v[1] / rounds for k, v in kt.items() if v[1]}
            pack_s = kt.get("pay_pack", [0.0, 0])[0] / 1e3
            if pack_s > 0:
                out["pack_TBs"] = rows * 4 * fw * 2 / pack_s / 1e12
                out["pack_frac_of_hbm_peak"] = out["pack_TBs"] / HBM_PEAK_TBS
        return out
    finally:
        sim.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=100000)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--settle", type=int, default=60)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--paths", default="shards4,loopback4")
    args = p.parse_args()
    for path in args.paths.split(","):
        rec = {"path": path, "nodes": args.nodes, "steps": args.steps, "windows": args.windows,
               "plain": run(path, args, False), "timers": run(path, args, True),
               "plain_again": run(path, args, False)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
