"""Which lane dimension do the longest DP intervals of a config run at?  dp_rows.py <cfg> [k]
The k largest intervals one at a time (kernel time of each alone, as dp_top.py), and for each the progressive steps it takes: the profile
length m in front of every step (the columns of the members before it, found by aligning that prefix alone), the sequence length n, and
what dp_batch.hip's rules make of (m, n): orientation, lane dimension, rows per lane under the old rule (4 above 128) and the new
(3 for 129..192).  The two rules are restated here; the orientation shown is lines x bands, the rule without a line cost."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from mauvealigner_amd import _lib, synth
cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
k = int(sys.argv[2]) if len(sys.argv) > 2 else 12
gs = synth.make_config(cfg, 1.0)
ctx = _lib.Context(0); ctx.set_genomes(gs)
p = _lib.default_params(seed_weight=15) if cfg in ("C2", "C3") else _lib.default_params()
n_dp, cost, cap = ctx.align_begin(p)
left, right = ctx.align_dp_anchors(n_dp)
order = np.argsort(-cost, kind="stable")
ctx.profile(True)
for rep in range(2):
    ctx.profile_reset(); ctx.align_dp(np.arange(n_dp), cap); launch = ctx.profile_get()["dp_step"]["ms"]
print("%s: %d intervals, all together: kernel %.3f ms" % (cfg, n_dp, launch))
bands = lambda x: (x + 255) // 256
rows_old = lambda x: 4 if x <= 32 or x > 128 else (1 if x <= 64 else 2)
rows_new = lambda x: 3 if 128 < x <= 192 else rows_old(x)


def member(g, l, r):
    """the bases of genome g between the two anchors (signed 1-based starts; a reverse member is reverse-complemented)"""
    ll, ls, rs = int(l[0]), int(l[1 + g]), int(r[1 + g])
    if ls == 0 or rs == 0:
        return None
    if ls > 0:
        return gs[g][ls - 1 + ll:rs - 1]
    rl = int(r[0])
    return (3 - gs[g][-rs - 1 + rl:-ls - 1][::-1]).astype(np.uint8)


for t in range(min(k, n_dp)):
    iv = int(order[t])
    idx = np.array([iv])
    for rep in range(2):
        ctx.profile_reset(); ctx.align_dp(idx, cap); ms = ctx.profile_get()["dp_step"]["ms"]
    mem = [member(g, left[iv], right[iv]) for g in range(len(gs))]
    line = "interval %d (#%d): cost %d, alone %.3f ms (%.0f %% of the launch)" % (t, iv, cost[iv], ms, 100 * ms / launch)
    if any(x is None for x in mem):
        print(line + "; an anchor lacks a genome: steps not reconstructed"); continue
    lens = [len(x) for x in mem]
    steps, m, cells = [], 0, 0
    for g, s in enumerate(mem):
        n = len(s)
        if n == 0:
            continue
        if m:
            ob = m * bands(n) < (n + 1) * bands(m)
            ld = n if ob else m
            steps.append("(m %d, n %d: %s, lanes hold %d, R %s -> %s, %d lines)" % (m, n, "B" if ob else "A", ld, rows_old(ld) if ld <= 256 else "4xbands",
                                                                                 rows_new(ld) if ld <= 256 else "4xbands", m if ob else n + 1))
            cells += m * n
            cols, _ = ctx.dp_batch([[x if j <= g else x[:0] for j, x in enumerate(mem)]])
            m = len(cols[0])
        else:
            m = n
    print(line + "; lengths %s; cells %d\n    %s" % (lens, cells, " ".join(steps)), flush=True)
