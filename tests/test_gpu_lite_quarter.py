"""k_lite_quarter (four nodes a wave, one per 16-lane row, the passive view
two entries a lane) against the oracle, bit for bit, on the scenarios of
tests/_lite_quarter_cases.py: full passive views at the slot boundaries
(sizes 1, 15, 17, 30, 16 and the default 30), the bucket-table load path of
the merge, and inboxes deeper than the 16 records a row reads at a time.
Every test also checks that the lite kernel did run nodes in a late round,
so none can pass by the nodes having gone to k_consume.  The two-nodes-a-wave
k_lite_half (PSIM_LITE_HALF=1) runs the same handlers with a 32-lane group:
the same scenarios in a child process each (the knob is read once per
process) -- they fill its one-entry-a-lane passive view to each boundary, and
D pushes the inbox past the 32 records a half reads at a time."""
import os
import subprocess
import sys

import pytest

import _lite_quarter_cases as Q
import _scenarios as S
from _oracle import Oracle
from partisan_amd import Simulator

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def gpu(cfg):
    cfg.device = 0
    return Simulator(cfg)


def check(gs, gst, os_, ost):
    S.compare_stats(gst, ost)
    S.compare_nodes(gs.nodes(), os_.nodes())
    # (the counts are the last round's)
    assert gs.kernel_counts()["k_lite_half"][0] > 0


@pytest.mark.parametrize("name", list(Q.F_CASES))
def test_full_views(name):
    gs, gst = Q.run_f(gpu, name)
    os_, ost = Q.run_f(Oracle, name)
    check(gs, gst, os_, ost)


def test_full_views_bucket_table():
    gs, gst = Q.run_f(S.with_buckets(gpu), "F30")
    os_, ost = Q.run_f(S.with_buckets(Oracle), "F30")
    check(gs, gst, os_, ost)


def test_deep_inboxes():
    gs, gst = Q.run_d(gpu)
    os_, ost = Q.run_d(Oracle)
    check(gs, gst, os_, ost)


HALF_CASES = ["F-m1", "F-m15", "F-m17", "F-m30-k1", "F16", "F30", "F30+buckets", "D"]


@pytest.mark.parametrize("name", HALF_CASES)
def test_half_kernel_scenarios(name):
    env = dict(os.environ, PSIM_LITE_HALF="1")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_lite_case_run.py"), name], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout


def test_half_kernel_keeps_parity():
    env = dict(os.environ, PSIM_LITE_HALF="1")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "_knob_run.py")], env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "identical" in r.stdout
