"""relay_reach() on injected graphs in a fresh process, for the test that sets
PSIM_RELAY_SLOTS / PSIM_RELAY_LANES in the child's environment (the library
reads both at the call): the bridge graph's 64 cases and two floods of the
9-clique of tests/_graph_families.py; prints both structs as JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np

import _graph_families as F
import _overlay_inject as I
from partisan_amd import Simulator
from partisan_amd.sim import default_config


def run(rows, cases):
    n = len(rows)
    sim = Simulator(default_config(n_nodes=n, seed=1))
    ids = np.arange(n, dtype=np.uint32)
    sim.join(ids, np.concatenate([np.array([0xFFFFFFFF], np.uint32), ids[:-1]]))
    sim.step(1)
    I.inject(sim, F.relay_inject_rows(rows))
    m = sim.relay_reach([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    sim.close()
    return {k: v.tolist() if isinstance(v, np.ndarray) else v for k, v in m.items()}


def main():
    rows = F.bridge_relay_rows()
    out = dict(bridge=run(rows, F.bridge_relay_cases(rows)))
    out["clique"] = run(F.relay_rows(F.clique_and_outsider(9)), [(0, 9, 16), (1, 9, 5)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
