"""Child process of tests/test_gpu_rare_branches.py: one scenario of the
registry's RARE table (argv[1]) on the GPU under whatever PSIM_* knobs the
environment sets, against the oracle.  Exit 0 = every round's stats and the
final node state identical."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _parity_registry as P  # noqa: E402
import _scenarios as S  # noqa: E402
from _oracle import Oracle  # noqa: E402
from partisan_amd import Simulator  # noqa: E402

name = sys.argv[1]
gs, gst = P.RARE[name](Simulator)[:2]
os_, ost = P.RARE[name](Oracle)[:2]
S.compare_stats(gst, ost)
if P.RARE_KIND[name] == "pl":
    S.compare_strategy(gs, os_)
else:
    S.compare_nodes(gs.nodes(), os_.nodes())
print(name, {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "identical over", len(gst), "rounds")
