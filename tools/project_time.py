"""Cost of the projection onto a genome subset on the GPU.  Prints ONE JSON line per workload and projection list (C3 onto
(0, 1) and (0, 4), C5 onto (0, 1), at full size, after mauve_align and mauve_coord_index), two routes to "the projection is the index in
force" timed in turn, `reps` rounds alternating them in one process after a warm-up round; per route the median and the spread (min, max)
in milliseconds, host clock around calls that end in a stream synchronise:

  device  mauve_project + mauve_project_index: nothing but the interval rows and the piece offsets crosses the host link;
          project_ms / index_ms split it
  host    mauve_align_fetch of the resident alignment, the numpy restatement (tests/project_ref.py), mauve_coord_index_alignment of what
          it made: the route a caller has without this stage; fetch_ms / restate_ms / index_ms split it

Before every round of either route the index in force is rebuilt from the resident alignment (mauve_coord_index, not timed).  The two
results are compared once (equal columns and interval tables) in the warm-up round.

usage: python tools/project_time.py [--reps R] [--configs C3,C5] [--skip-c5] [--profile]
  --profile: C3 only, three rounds of the device route onto (0, 1) and (0, 4), nothing printed (the run under rocprofv3 --kernel-trace
             --stats: pj_count, pj_firsts, pj_write, the scans, the index build, and pj_source behind a fetch of src_col)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402
from tests import project_ref as PR  # noqa: E402

LISTS = {"C3": ((0, 1), (0, 4)), "C5": ((0, 1),)}


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def workload(ctx, name, reps):
    gs = synth.make_config(name)
    ctx.set_genomes(gs)
    res = ctx.align(_lib.default_params(), fetch=False)
    sz = _lib.AlignSizes()
    for k, _ in _lib.AlignSizes._fields_:
        setattr(sz, k, int(res[k]))
    for proj in LISTS[name]:
        t = {k: [] for k in ("device", "project", "index", "host", "fetch", "restate", "host_index")}
        sizes = None
        for rnd in range(reps + 1):                              # round 0 warms up: code objects, buffer growth, the host copy of the alignment
            ctx.coord_index()
            t0 = time.perf_counter()
            sizes = ctx.project(proj)
            t1 = time.perf_counter()
            ctx.project_index()
            t2 = time.perf_counter()
            ctx.coord_index()
            t3 = time.perf_counter()
            a = ctx._fetch(sz)
            t4 = time.perf_counter()
            w = PR.project(a, proj)
            t5 = time.perf_counter()
            ctx.coord_index_alignment(w["left"], w["right"], w["reverse"], w["col_off"], w["cols"])
            t6 = time.perf_counter()
            if rnd == 0:
                assert PR.same(ctx.project_fetch(), w) == [], "the two routes differ"
                continue
            for k, v in (("device", t2 - t0), ("project", t1 - t0), ("index", t2 - t1), ("host", t6 - t3), ("fetch", t4 - t3), ("restate", t5 - t4), ("host_index", t6 - t5)):
                t[k].append(v * 1e3)
        out = {"workload": name, "device": ctx.device_name(), "nseq": len(gs), "proj": list(proj), "src_iv": int(res["n_iv"]), "src_cols": int(res["n_cols"]), "reps": reps}
        out.update(sizes)
        out.update({k + "_ms": spread(v) for k, v in t.items()})
        out["ratio"] = out["host_ms"]["median"] / out["device_ms"]["median"]
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        if a.profile:
            ctx.set_genomes(synth.make_config("C3"))
            ctx.align(_lib.default_params(), fetch=False)
            for _ in range(3):
                for proj in LISTS["C3"]:
                    ctx.coord_index()
                    ctx.project(proj)
                    ctx.project_index()
                    ctx.project_fetch(want=("src_col",))       # pj_source: the source columns are made by the fetch that asks for them
            return
        for name in [c for c in a.configs.split(",") if not (a.skip_c5 and c == "C5")]:
            workload(ctx, name, a.reps)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
