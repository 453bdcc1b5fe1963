"""Child process of tests/test_gpu_random_schedule.py::test_knobs: a fixed part
of the random-schedule corpus (four hv entries, two xbot, one of each pluggable
kind) on the GPU under whatever PSIM_* knobs the environment sets, against the
oracle: every round's stats, every event call's return code, every probe and
the final state.  Exit 0 and a line with "identical" = no difference.

PSIM_KNOB_PATH (as tests/_knob_run.py): "local" (one shard), "loopbackN" (N
loopback ranks), "rccl1" (a one-rank RCCL communicator).  A full-membership
handle has no ranks (psim_create refuses them): on "loopbackN" that entry is
left out, and the line says so."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import _random_schedule as R  # noqa: E402

ENTRIES = [("hv", 1), ("hv", 4), ("hv", 7), ("hv", 9), ("xbot", 2), ("xbot", 4),
           ("scamp_v1", 3), ("scamp_v2", 4), ("full", 3)]


def main():
    path = os.environ.get("PSIM_KNOB_PATH", "local")
    rounds = calls = 0
    left_out = []
    for kind, seed in ENTRIES:
        assert (kind, seed) in R.CORPUS
        if kind == "full" and path.startswith("loopback"):
            left_out.append(f"{kind}-{seed}")
            continue
        sch = R.generate(kind, seed)
        make, opts = R.path(path, kind)
        R.compare(R.execute(make, sch, opts), R.execute(R.oracle_make, sch))
        rounds += sch.rounds()
        calls += len(sch.calls())
    print("knobs", {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "identical over", rounds, "rounds and",
          calls, "event calls; left out:", left_out)


if __name__ == "__main__":
    main()
