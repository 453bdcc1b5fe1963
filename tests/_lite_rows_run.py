"""Child process of tests/test_gpu_lite_rows.py: one scenario group on the GPU
under whatever PSIM_* knobs the environment sets (they are read once per
process), against the oracle's results the parent computed once and saved:
argv = group, reference .npz.  Exit 0 = every round's stats and the final node
state identical for every scenario of the group.  The last line printed is
JSON: per scenario, for every round stepped on its own, [round, the lite
kernel's nodes, its deliveries] (kernel_counts; empty on the rank path, whose
counts are one shard's)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _scenarios as S  # noqa: E402
from _lite_rows_cases import GROUPS  # noqa: E402
from partisan_amd import Simulator  # noqa: E402

path = os.environ.get("PSIM_KNOB_PATH", "local")
rows = []


class Counted(Simulator):
    def step(self, n_rounds=1):
        r = self.round
        st = super().step(n_rounds)
        if n_rounds == 1:
            k = self.kernel_counts()
            rows.append([int(r), int(k["k_lite_half"][0]), int(k["k_lite_half"][1])])
        return st


def gpu(cfg, n_shards=1):
    cfg.device, cfg.n_shards = 0, n_shards
    return Counted(cfg)


if path.startswith("loopback"):
    from _loopback import LoopbackRanks
    make = lambda cfg, n_shards=1: LoopbackRanks(cfg, int(path[len("loopback"):]))  # noqa: E731
else:
    make = gpu

group, ref = sys.argv[1], np.load(sys.argv[2])
counts = {}
for name, run in GROUPS[group]:
    del rows[:]
    gs, gst = run(make)
    S.compare_stats(gst, ref[name + ".stats"])
    S.compare_nodes(gs.nodes(), ref[name + ".nodes"])
    gs.close()
    counts[name] = list(rows)
print("group", group, {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "identical")
print(json.dumps(counts))
