"""One relay_reach() call on a fresh GPU handle, for a test that sets
PSIM_RELAY_SLOTS / PSIM_RELAY_LANES in the child's environment (both are read
by the library at the call): scenario A of tests/test_gpu_relay.py, the cases
given as JSON in argv[1], max_levels in argv[2]; prints the struct as JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import _scenarios as S
from partisan_amd import Simulator


def main():
    cases, cap = json.loads(sys.argv[1]), int(sys.argv[2])
    g = S.doubling(Simulator, n=203, seed=3, rounds=30)[0]
    m = g.relay_reach([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], max_levels=cap)
    g.close()
    print(json.dumps({k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in m.items()}))


if __name__ == "__main__":
    main()
