"""Full-membership handles over virtual shards and loopback ranks (test
infrastructure): the `make` functions of tests/test_gpu_full_sharded.py, and
the loopback world with the two calls a full handle adds to _loopback's."""
import numpy as np

from _loopback import LoopbackRanks


def vshards(g):
    """make(cfg) -> a Simulator of g virtual shards on device 0"""
    def make(cfg):
        from partisan_amd import Simulator
        c = type(cfg).from_buffer_copy(cfg)
        c.device, c.n_shards = 0, g
        return Simulator(c)
    return make


class FullLoopbackRanks(LoopbackRanks):
    def member_bits(self, node):
        """the member bitset of `node`, asked of the rank that owns it"""
        return self.ranks[node // self.per].member_bits(node)

    def strategy_histograms(self):
        """a collective: one thread per rank, every rank the same answer"""
        hs = self._threads("strategy_histograms")
        for h in hs[1:]:
            assert all(np.array_equal(h[k], hs[0][k]) for k in h), "ranks disagree on the overlay statistics"
        return hs[0]


def loopback(world):
    """make(cfg) -> `world` loopback ranks driven like one simulator"""
    def make(cfg):
        return FullLoopbackRanks(cfg, world)
    return make
