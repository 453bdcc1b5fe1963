"""Scenario groups of tests/test_gpu_ptl_early.py, shared by the parent (the
oracle's run of each, once) and its child processes (the GPU's, per knob set):
group -> [(name, run(make) -> (sim, stats))]."""
import _scenarios as S

GROUPS = {
    # Plumtree traffic beside due shuffles, SHUFFLE terminals and joins
    "doubling": [("doubling", lambda make: S.doubling(make, 4096, 9, 60, bcast_period=10, bcast_first=20))],
    # crash rounds go serial (one k_ptl launch over both parts), the rounds between overlapped
    "churn_partition": [("churn_partition", lambda make: S.churn_partition(make, n=2048))],
    # several rounds a step call: the batch path
    "multistep": [("multistep", S.multistep)],
    # closing entries: nodes that fall to k_pt from either part
    "xbot_churn": [("xbot_churn", lambda make: S.xbot_churn(make, n=2048))],
}
