"""The oracle fails the step with PSIM_ENOMEM when a round buffer cannot grow
(it used to write through realloc's NULL).  The full strategy with fanout 0
at 65 nodes floods (tens of millions of gossips within 60 rounds): under an
address-space limit 48 MiB above what the process already maps, the outbox
stops growing in round 11, after about a second.  The limit has to be a
process's own: the run is a child's."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

CHILD = r"""
import resource, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import _scenarios as S
from _oracle import Oracle, load
from partisan_amd.sim import SimError
load()
with open("/proc/self/statm") as f:
    mapped = int(f.read().split()[0]) * resource.getpagesize()
limit = mapped + (48 << 20)
resource.setrlimit(resource.RLIMIT_AS, (limit, limit))
kept = {}
def make(cfg):
    kept["sim"] = Oracle(cfg)
    return kept["sim"]
try:
    S.pl_doubling(make, 65, 11, 60, strategy=0)
    print("ran to the end")
except SimError as e:
    sim = kept["sim"]
    print("failed:", e.rc, "round", sim.round)
    try:
        sim.step(1)
        print("then stepped")
    except SimError as e2:
        print("then:", e2.rc)
"""


def test_step_fails_with_enomem():
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    print(out)
    assert out[0].startswith("failed: -2 round"), out          # PSIM_ENOMEM, no crash
    assert out[1] == "then: -4", out                            # the handle is unusable: PSIM_ESTATE
