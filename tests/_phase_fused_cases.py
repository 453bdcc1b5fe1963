"""Scenario groups of tests/test_gpu_phase_fused.py, shared by the parent (the
oracle's run of each, once) and its child processes (the GPU's, per knob set):
group -> [(name, run(make) -> (sim, stats))]."""
import _lite_quarter_cases as Q
import _scenarios as S


def _f(name):
    return lambda make: Q.run_f(make, name)


GROUPS = {
    # several rounds a step call: the batch path
    "multistep": [("multistep", S.multistep)],
    # crash rounds go serial and the rounds between go fused, in one run
    "churn_partition": [("churn_partition", lambda make: S.churn_partition(make, n=2048))],
    # joins and promotions for k_consume beside due shuffles, and broadcasts
    "doubling": [("doubling", lambda make: S.doubling(make, 4096, 9, 60, bcast_period=10, bcast_first=20))],
    # k_consume's heaviest handlers
    "xbot_churn": [("xbot_churn", lambda make: S.xbot_churn(make, n=2048))],
    # the lite body: full passive views at the slot boundaries, deep inboxes
    "lite_F": [(name, _f(name)) for name in Q.F_CASES],
    "lite_D": [("D", Q.run_d)],
}
