"""One psim_get_latency_metrics call in a fresh process (test infrastructure of
tests/test_gpu_latency.py): argv[1] = JSON [scenario, sources, cap, root]; the
environment selects the push kernel and the weight path.  Prints the struct as
one JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_latency import RUNS, _gpu  # noqa: E402


def main():
    key, sources, cap, root = json.loads(sys.argv[1])
    g = RUNS[key][0](_gpu)[0]
    m = g.latency_metrics(sources, tree_root=root, max_sweeps=cap)
    g.close()
    print(json.dumps({k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in m.items()}))


if __name__ == "__main__":
    main()
