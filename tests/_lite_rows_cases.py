"""Scenario groups of tests/test_gpu_lite_rows.py, shared by the parent (the
oracle's run of each, once) and its child processes (the GPU's, per knob set):
group -> [(name, run(make) -> (sim, stats))].  `make(cfg, n_shards=1)` builds
the simulator; the oracle has no shards and ignores the count.

The lite kernel fetches the next node's rows into LDS behind the body of the
node it runs (psim_lite.h, PSIM_LITE_ROWS_LDS): one DMA per wave, whose lanes
belong to four nodes (two in k_lite_half), with groups that have no node,
groups that have left the loop, and ordinary loads in the body of a node with
a long inbox.  What each group is there for:

tiny     overlays of 3, 5, 9, 33 and 130 nodes that shuffle every round: lite
         lists of 1 to about 120 nodes, mostly no multiple of 4, so a wave has
         groups without a node, groups with one node beside a neighbour with
         two, and lists of a single node; from n = 5 up some inboxes pass 16
         records (the row kernel's second pass over the inbox, an ordinary
         load while a DMA is in flight)
edges    tests/_relay_lead_cases.py's: a join ramp, views of two, and a star
         whose inboxes pass 32 records (the half kernel's second pass)
churn_partition
         crash rounds launch k_lite_quarter on its own; sends fail across the
         partition
shards2  1024 nodes in two virtual shards: the second shard's rows are indexed
         by id - lo with lo = 512
"""
import _relay_lead_cases as R
import _scenarios as S
from partisan_amd import workloads as W
from partisan_amd.sim import default_config

TINY_SIZES = (3, 5, 9, 33, 130)
TINY_SEED, TINY_ROUNDS, TINY_BCAST = 11, 80, 40


def tiny(make, n):
    sim = make(default_config(n_nodes=n, seed=TINY_SEED, shuffle_period=1))

    def hook(r):
        if r == TINY_BCAST:
            sim.broadcast(0, 0)
    return sim, sim.run_schedule(W.doubling_join(n, TINY_SEED), TINY_ROUNDS, extra=hook)


def shards2(make):
    n, seed = 1024, 13
    sim = make(default_config(n_nodes=n, seed=seed, shuffle_period=2), n_shards=2)
    bc = S._bcast_every(sim, 10, 20)
    return sim, sim.run_schedule(W.doubling_join(n, seed), 60, extra=bc)


def _theirs(run):
    return lambda make: run(lambda cfg: make(cfg))


GROUPS = {
    "tiny": [("tiny%d" % n, lambda make, n=n: tiny(make, n)) for n in TINY_SIZES],
    "edges": [(name, _theirs(run)) for name, run in R.GROUPS["edges"]],
    "churn_partition": [(name, _theirs(run)) for name, run in R.GROUPS["churn_partition"]],
    "shards2": [("shards2", shards2)],
}
