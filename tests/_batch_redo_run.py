"""Child process of tests/test_gpu_batch_redo.py: one scenario on the GPU under
whatever PSIM_* knobs the environment sets (PSIM_TEST_DESC_CAP is read once
per process), against the oracle's results the parent computed once and
saved: argv = scenario, reference .npz.  Exit 0 = every round's stats and the
final node state identical.  The last line printed is JSON: "prep" = per round
stepped on its own (local path), the quiet lazy ticks k_node_prep counted
without running the node (kernel_counts), "overflow" = the run's overflows.

CASES is shared with the parent: scenario -> run(make) -> (sim, stats)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _scenarios as S  # noqa: E402

CASES = {
    # the heal of a partition that left quiet nodes, first of a multi-round step
    "heal_after_quiet": lambda make: S.heal_after_quiet(make, n=512),
    # outstanding tables past one register over a partition, single-round steps
    "out_tail": lambda make: S.out_tail(make, n=512)[:2],
    # a broadcast, a crash wave, a partition and its heal, each first of a multi-round step
    "multistep": lambda make: S.multistep(make, n=4096),
    # joins, crashes and rejoins, a partition: every event kind of the HyParView scenarios
    "churn_partition": lambda make: S.churn_partition(make, n=2048),
    "xbot_churn": lambda make: S.xbot_churn(make, n=1024, rounds=100),
}


def main():
    from partisan_amd import Simulator

    path = os.environ.get("PSIM_KNOB_PATH", "local")
    prep = {}

    class Counted(Simulator):
        def step(self, n_rounds=1):
            r = self.round
            st = super().step(n_rounds)
            if n_rounds == 1:
                prep[r] = int(self.kernel_counts()["k_node_prep"][0])
            return st

    def gpu(cfg):
        cfg.device = 0
        return Counted(cfg)

    if path.startswith("loopback"):
        from _loopback import LoopbackRanks
        make = lambda cfg: LoopbackRanks(cfg, int(path[len("loopback"):]))  # noqa: E731
    else:
        make = gpu

    import numpy as np
    name, ref = sys.argv[1], np.load(sys.argv[2])
    gs, gst = CASES[name](make)
    S.compare_stats(gst, ref["stats"])
    S.compare_nodes(gs.nodes(), ref["nodes"])
    gs.close()
    print("scenario", name, {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "identical")
    print(json.dumps({"prep": prep, "overflow": int(gst["overflow"].sum())}))


if __name__ == "__main__":
    main()
