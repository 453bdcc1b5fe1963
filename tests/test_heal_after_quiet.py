"""The heal_after_quiet scenario does on the oracle what its users rely on
(tests/test_gpu_batch_redo.py, tests/test_gpu_restore.py): quiet rounds under
the partition -- few messages, thousands of failed lazy sends -- then the heal
round's wake-up as the first round of a multi-round step."""
import _scenarios as S
from _oracle import Oracle


def test_heal_wakes_the_quiet_nodes():
    sim, st = S.heal_after_quiet(Oracle)
    assert len(st) == 113 and [int(r) for r in st["round"]] == list(range(113))
    em = st["emitted"].sum(1)
    assert [int(x) for x in st["send_fail"][66:68]] == [7870, 7976]
    assert [int(x) for x in em[66:70]] == [676, 623, 8593, 17461]
    assert int(st["send_fail"][68]) < 200          # the pushes across the healed partition go out
    assert int(st["overflow"].sum()) == 0
    # the second leg's events: two crash waves of n / 16, the first rejoined, the second revived
    assert [int(st["nodes_up"][r]) for r in (83, 84, 91, 99, 105)] == [512, 480, 512, 480, 512]
    assert int(st["exits"][84]) > 0 and int(st["exits"][99]) > 0
    sim.close()
