"""Child process of tests/test_gpu_lite_quarter.py: one scenario of
tests/_lite_quarter_cases.py (an F case name, NAME+buckets for the bucket
table, or D) on the GPU under whatever PSIM_LITE_* knob the environment sets
(the knobs are read once per process), against the oracle.  Exit 0 = every
round's stats and the final node state identical, and the lite kernel ran
nodes in the last round."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _lite_quarter_cases as Q  # noqa: E402
import _scenarios as S  # noqa: E402
from _oracle import Oracle  # noqa: E402
from partisan_amd import Simulator  # noqa: E402


def gpu(cfg):
    cfg.device = 0
    return Simulator(cfg)


name = sys.argv[1]
if name == "D":
    gs, gst = Q.run_d(gpu)
    os_, ost = Q.run_d(Oracle)
elif name.endswith("+buckets"):
    gs, gst = Q.run_f(S.with_buckets(gpu), name[:-len("+buckets")])
    os_, ost = Q.run_f(S.with_buckets(Oracle), name[:-len("+buckets")])
else:
    gs, gst = Q.run_f(gpu, name)
    os_, ost = Q.run_f(Oracle, name)
S.compare_stats(gst, ost)
S.compare_nodes(gs.nodes(), os_.nodes())
ran = gs.kernel_counts()["k_lite_half"][0]
assert ran > 0, ran
print("case", name, {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "identical over", len(gst),
      "rounds; lite nodes in the last round:", ran)
