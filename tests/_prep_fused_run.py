"""Child process of tests/test_gpu_prep_fused.py: a list of (scenario, size)
cases on the GPU under whatever PSIM_* knobs the environment sets
(PSIM_PREP_FUSED and the others are read once per process), against the
oracle's results the parent computed once and saved: argv = the cases as
"scenario:n,scenario:n,...", the reference .npz.  Exit 0 = every round's stats
(the digest among them), the final node rows and the overlay histograms
identical for every case.

The scenarios step one round at a time (run_schedule); batches form only in
calls of several rounds.  So the handle here is `Lagged`: a step is not run but
owed, and the rounds owed run as one psim_step call when the next event (or a
read of the state) comes -- the same rounds with the same events at the same
rounds, stepped in calls as long as the stretches between events."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import _scenarios as S  # noqa: E402

CASES = {
    # a broadcast at a batch's first round: its origin must read as spent in the second
    "multistep": lambda make, n: S.multistep(make, n=n),
    # crash rounds between the stepped calls
    "churn_partition": lambda make, n: S.churn_partition(make, n=n),
    # quiet lazy ticks counted by the prepare; the wake on the event round only
    "heal_after_quiet": lambda make, n: S.heal_after_quiet(make, n=n),
    # a saturated outstanding nibble: the prepare reads the header
    "out_tail": lambda make, n: S.out_tail(make, n=n)[:2],
    # X-BOT: closing connections and due optimization rounds in the bound
    "xbot_churn": lambda make, n: S.xbot_churn(make, n=n),
    # every node joins node 0: its bucket of the fused route overflows
    "star": lambda make, n: S.star(make, n=n, rounds=20),
}


def parse(arg):
    return [(c.split(":")[0], int(c.split(":")[1])) for c in arg.split(",")]


def main():
    from partisan_amd import Simulator, _abi

    class Lagged(Simulator):
        _lag = 0

        def _flush(self):
            if self._lag:
                k, self._lag = self._lag, 0
                self.__dict__.setdefault("_stats", []).append(Simulator.step(self, k))

        def step(self, n_rounds=1):
            self._lag += n_rounds
            return np.zeros(0, _abi.STATS_DTYPE)     # (the stats come from all_stats)

        @property
        def round(self):
            return Simulator.round.fget(self) + self._lag

        def all_stats(self):
            self._flush()
            return np.concatenate(self.__dict__.get("_stats", []))

    for name in ("join", "crash", "revive", "broadcast", "set_partition", "clear_partition", "nodes", "histograms"):
        def wrap(f):
            def g(self, *a, **k):
                self._flush()
                return f(self, *a, **k)
            return g
        setattr(Lagged, name, wrap(getattr(Simulator, name)))

    def gpu(cfg):
        cfg.device = 0
        return Lagged(cfg)

    ref = np.load(sys.argv[2])
    for name, n in parse(sys.argv[1]):
        key = f"{name}:{n}"
        gs = CASES[name](gpu, n)[0]
        S.compare_stats(gs.all_stats(), ref[key + ".stats"])
        S.compare_nodes(gs.nodes(), ref[key + ".nodes"])
        hist = gs.histograms()
        for k, v in hist.items():
            assert np.array_equal(np.asarray(v), ref[key + ".hist." + k]), (key, k)
        gs.close()
        print("case", key, "identical", flush=True)
    print("cases", sys.argv[1], {k: v for k, v in os.environ.items() if k.startswith("PSIM_")}, "all identical")


if __name__ == "__main__":
    main()
