"""The host-to-host step of bench.py split into its three calls, run the way bench.py's step runs them: set_genomes_packed,
align(fetch=False, out=bufs, compact=True) -- which registers the table prefetch (mauve_align_prefetch) when the binding has
it -- and _fetch_compact into the same page-locked buffers.  With the prefetch the two bulk tables travel while the pass runs:
`align` then carries what of them is still exposed and `fetch` holds the column copy alone.

    python3 tools/sweep/h2h_split.py [--config C3] [--steps 20] [--warmup 5]

Short enough to sit under a tracer (the last step is the one to look at):
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d OUT -- python3 tools/sweep/h2h_split.py --steps 3 --warmup 3
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
from mauvealigner_amd import _lib  # noqa: E402
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()

gs, _, L = bench.make_workload(a.config, 1.0, 0)
ctx = _lib.Context(0)
packed, lens = bench.pack_pinned(gs)
bufs = _lib.ResultBuffers()
p = bench.params_for(a.config)


STAGES = ("seed_ms", "chain_ms", "dp_ms", "assemble_ms", "total_ms")
stages = []


def step(tm):
    t0 = time.perf_counter()
    ctx.set_genomes_packed(packed, lens)
    t1 = time.perf_counter()
    r = ctx.align(p, fetch=False, out=bufs, compact=True)
    t2 = time.perf_counter()
    sz = _lib.AlignSizes(**{k: r[k] for k, _ in _lib.AlignSizes._fields_})
    ctx._fetch_compact(sz, bufs)
    t3 = time.perf_counter()
    st = ctx.stage_times()
    tm.append((t1 - t0, t2 - t1, t3 - t2))
    stages.append([st[k] for k in STAGES])
    return r


for _ in range(a.warmup):
    step([])
tm = []
for _ in range(a.steps):
    r = step(tm)
t = np.array(tm) * 1e3
med = np.median(t, axis=0)
print("%s: %d mums, %d anchors, %d columns; prefetch entry %s" % (a.config, r["n_mums"], r["n_anchor"], r["n_cols"],
                                                                   "present" if hasattr(ctx.L, "mauve_align_prefetch") else "absent"))
print("median of %d steps: upload %.3f ms, align %.3f ms, fetch %.3f ms, step %.3f ms" % (a.steps, med[0], med[1], med[2], np.median(t.sum(axis=1))))
print("min: upload %.3f ms, align %.3f ms, fetch %.3f ms, step %.3f ms" % (t[:, 0].min(), t[:, 1].min(), t[:, 2].min(), t.sum(axis=1).min()))
print("inside align (median): " + ", ".join("%s %.3f" % (k[:-3], v) for k, v in zip(STAGES, np.median(np.array(stages[-a.steps:]), axis=0))))
ctx.close()
