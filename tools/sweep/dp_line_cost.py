"""Time per line of the one-wave scan sweeps at R = 1, 2, 3, 4 rows (orientation A) / columns (B) per lane: single-interval launches of a pair,
the lane dimension fixed at 64 R, the number of lines at 24 and at 64 R - 8; the slope of the kernel time between the two is the cost of
a line (the walk and the rebuild see the same longer dimension both times).  Prints one row per (orientation, R) and the table
dp_batch.hip's dp3_line_cost wants (units of 10 ns).  MAUVE_DP_NO_GROUPS keeps the pairs with few lines out of the sub-wave classes.
The shapes keep the orientation they are meant to have under any rule that prices a line between 1 / 2 and 2 times another's."""
import os, sys
os.environ["MAUVE_DP_NO_GROUPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from mauvealigner_amd import _lib
rng = np.random.default_rng(3)
ctx = _lib.Context(0); ctx.profile(True)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 12


def t(m, n):
    a = rng.integers(0, 4, m, dtype=np.uint8); b = rng.integers(0, 4, n, dtype=np.uint8)
    ts = []
    for rep in range(REPS):
        ctx.profile_reset(); ctx.dp_batch([[a, b]]); ts.append(ctx.profile_get()["dp_step"]["ms"])
    return min(ts), float(np.median(ts))


table = {}
for R in (1, 2, 3, 4):
    x, l0, l1 = 64 * R, 24, 64 * R - 8
    for o in "AB":
        # A: m on the lanes, n + 1 lines; B: n on the lanes, m lines
        (a0, am0), (a1, am1) = (t(x, l0 - 1), t(x, l1 - 1)) if o == "A" else (t(l0, x), t(l1, x))
        ns = (a1 - a0) * 1e6 / (l1 - l0)
        table[(o, R)] = int(round(ns / 10))
        print("R %d %s: lanes hold %3d; %3d lines %.2f us (median %.2f), %3d lines %.2f us (median %.2f): %.0f ns per line" %
              (R, o, x, l0, a0 * 1e3, am0 * 1e3, l1, a1 * 1e3, am1 * 1e3, ns), flush=True)
print("dp3_line_cost:", table)
