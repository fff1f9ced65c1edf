"""The one-wave scan sweep at every number of rows per lane, three above all (a lane dimension of 129..192): ctx.dp_batch against
O.align_interval, columns and scores, exact.  The cases are tests/dp_rows_cases.py's; one child process per route, because the
routes are switches the library reads once."""
import os
import pickle
import re
import subprocess
import sys

import pytest

from tests import dp_rows_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MAUVE_DP_ONE_WAVE", "MAUVE_DP_NOSCAN", "MAUVE_DP_NO_GROUPS", "MAUVE_DP_WIDE_MIN", "MAUVE_DP_BIG_MAX", "MAUVE_DP_NO_WIDE", "MAUVE_DP_CLUSTER",
            "MAUVE_DP_CLASS", "MAUVE_DP_TB_BUDGET")
TRACE = re.compile(r"\[trace\] dp_core: \d+ round\(s\); (\d+) intervals: (\d+) workgroup, (\d+) one-wave, (\d+) two/wave, (\d+) four/wave")

# one_wave: no workgroup kernel and no sub-wave groups, so every interval is dp3_interval's; wide: every interval with a step of several bands goes to the
# workgroup kernel, whose steps of at most one band run the same one-wave sweep on its first wave; default: whatever the launch list decides
ROUTES = {
    "one_wave": {"MAUVE_DP_ONE_WAVE": "1", "MAUVE_DP_NO_GROUPS": "1"},
    "wide": {"MAUVE_DP_WIDE_MIN": "1"},
    "default": {},
}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """the oracle's result of every case under every scheme, computed once for all routes"""
    path = str(tmp_path_factory.mktemp("dp_rows") / "dp_rows_ref.pickle")
    with open(path, "wb") as f:
        pickle.dump(W.reference(), f)
    return path


def test_the_cases_reach_the_edges():
    """what the shapes are there for (no launch): every lane dimension of the list in both roles, the three positions of the last row, lane 63"""
    lens = [[len(s) for s in iv if len(s)] for _, iv in W.intervals()]
    pairs = [l for l in lens if len(l) == 2]
    for L in W.LANE_DIMS:
        assert any(l[0] == L and l[1] < L for l in pairs) and any(l[1] == L and l[0] < L for l in pairs), L
    assert {(m - 1) % 3 for m in (130, 131, 132)} == {0, 1, 2} and {(m - 1) // 3 for m in (190, 191, 192)} == {63}
    assert {len(l) for l in lens} >= {2, 3, 5}
    assert any(len(iv[1]) == 0 and len(iv[2]) > 0 for _, iv in W.intervals())


@pytest.mark.parametrize("route", list(ROUTES))
def test_rows_per_lane_against_the_oracle(route, reference):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ROUTES[route], MAUVE_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "tests.dp_rows_cases", reference], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    n = len(W.intervals())
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK %d" % (n * len(W.SCHEMES)), route + "\n" + r.stdout[-2000:] + r.stderr[-4000:]
    launches = [tuple(int(x) for x in m.groups()) for m in TRACE.finditer(r.stderr)]
    assert len(launches) == len(W.SCHEMES)
    for total, big, med, s32, s16 in launches:
        assert total == n
        if route == "one_wave":
            assert (big, med) == (0, n)                      # a wave per interval, and every scheme here is admitted by the scans
        elif route == "wide":
            assert big >= 3                                  # the "mixed" intervals: small steps of a workgroup entry
