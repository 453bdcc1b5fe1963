"""Child process of tests/test_gpu_phase_fused.py: one scenario group on the
GPU under whatever PSIM_* knobs the environment sets (they are read once per
process), against the oracle's results the parent computed once and saved:
argv = group, reference .npz.  Exit 0 = every round's stats and the final node
state identical for every scenario of the group.  The last line printed is
JSON: over the rounds stepped one at a time, how many ran no crash and had
nodes in k_shuf, the lite kernel and k_consume at once ("reach"), and how
many were crash rounds ("crash")."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _scenarios as S  # noqa: E402
from _phase_fused_cases import GROUPS  # noqa: E402
from partisan_amd import Simulator  # noqa: E402

path = os.environ.get("PSIM_KNOB_PATH", "local")
reach = {"reach": 0, "crash": 0}


class Counted(Simulator):
    """counts, after every single-round step, what the round's HyParView
    kernels ran (a crash round is one that delivered EXITs: phase_consume
    runs those serially)"""

    def step(self, n_rounds=1):
        st = super().step(n_rounds)
        if n_rounds == 1:
            k = self.kernel_counts()
            # (k_shuf's nodes are counted by k_relay, which listed them: its
            # own row has the SHUFFLEs they emitted)
            all3 = k["k_shuf"][2] > 0 and k["k_lite_half"][0] > 0 and k["k_consume"][0] > 0
            crash = int(st["exits"][0]) > 0
            reach["crash"] += crash
            reach["reach"] += all3 and not crash
        return st


def gpu(cfg):
    cfg.device = 0
    return Counted(cfg)


if path.startswith("loopback"):
    from _loopback import LoopbackRanks
    make = lambda cfg: LoopbackRanks(cfg, int(path[len("loopback"):]))  # noqa: E731
else:
    make = gpu

group, ref = sys.argv[1], np.load(sys.argv[2])
for name, run in GROUPS[group]:
    gs, gst = run(make)
    S.compare_stats(gst, ref[name + ".stats"])
    S.compare_nodes(gs.nodes(), ref[name + ".nodes"])
    gs.close()
print("group", group, {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "identical")
print(json.dumps(reach))
