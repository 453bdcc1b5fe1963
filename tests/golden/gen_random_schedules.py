"""Regenerates tests/golden/random_schedules.json: for every (kind, seed) of the
random-schedule corpus (tests/_random_schedule.py CORPUS) the SHA-256 of the
schedule's canonical JSON and the oracle's `digest` stat summed over its
rounds (mod 2^64).  tests/test_random_schedule.py::test_pinned compares both,
so a numpy or generator change cannot silently swap the corpus.

SELF-GENERATED: the digests come from oracle/psim_oracle.c, not from running
the reference.
Usage: python tests/golden/gen_random_schedules.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import _random_schedule as R  # noqa: E402


def main():
    out = {}
    for kind, seed in R.CORPUS:
        sch = R.generate(kind, seed)
        tr = R.execute(R.oracle_make, sch)
        out[f"{kind}-{seed}"] = {"sha256": sch.sha256(), "digest": tr.digest(), "n": sch.n,
                                 "event_calls": len(sch.calls())}
    with open(os.path.join(HERE, "random_schedules.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} entries")


if __name__ == "__main__":
    main()
