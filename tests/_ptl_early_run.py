"""Child process of tests/test_gpu_ptl_early.py: one scenario group on the GPU
under whatever PSIM_* knobs the environment sets (they are read once per
process), against the oracle's results the parent computed once and saved:
argv = group, reference .npz.  Exit 0 = every round's stats and the final node
state identical for every scenario of the group.  The last line printed is
JSON, counted after every single-round step from psim_debug_kernel_counts with
cap 32 (a kernel "delivered" when its records-delivered count is above zero):
"overlap": non-crash rounds in which the early part of k_ptl's list, the late
part (the k_ptl entry less the early one) and the lite kernel all delivered;
"crash": crash rounds; "pt_early": rounds in which k_pt and the early part
both delivered."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _scenarios as S  # noqa: E402
from _ptl_early_cases import GROUPS  # noqa: E402
from partisan_amd import Simulator  # noqa: E402

path = os.environ.get("PSIM_KNOB_PATH", "local")
reach = {"overlap": 0, "crash": 0, "pt_early": 0}
# entries of psim_debug_kernel_counts, 4 words each: [1] = records delivered
LITE, PTL, PT, EARLY = 2, 4, 5, 7


class Counted(Simulator):
    def step(self, n_rounds=1):
        st = super().step(n_rounds)
        if n_rounds == 1:
            out = (C.c_uint64 * 32)()
            k = self._extra["debug_kernel_counts"](self._h, out, 32)
            assert k == 8, k
            dl = [int(out[4 * i + 1]) for i in range(8)]
            assert dl[PTL] >= dl[EARLY]
            crash = int(st["exits"][0]) > 0
            reach["crash"] += crash
            reach["overlap"] += (not crash) and dl[EARLY] > 0 and dl[PTL] - dl[EARLY] > 0 and dl[LITE] > 0
            reach["pt_early"] += dl[PT] > 0 and dl[EARLY] > 0
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
