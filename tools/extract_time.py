"""Cost of the column extraction on the GPU.  Prints ONE JSON line per workload (C3, C5 at full size, after mauve_align and
mauve_coord_index), the routes to the letters of the alignment timed in turn, `reps` rounds of all of them in one process after a
warm-up round; per route the median and the spread (min, max) in milliseconds:

  all     mauve_extract_select + mauve_extract_fetch of the unconditioned matrix (every column, every genome) into page-locked arrays:
          select, fill and copy-out, the call ends in a stream synchronise; select_ms / fetch_ms split it
  core    the same for the core matrix (require = all genomes)
  all_rows / core_rows   the two with the matrix alone fetched (sel_iv, sel_col, range_off = NULL: 16 bytes per selected column stay behind)
  xmfa    mauve_write_xmfa on the same context into a buffer of the right size -- the only route to the same letters without this
          stage (one call; the size query that normally precedes it costs as much again and is not counted)

ratio_* = xmfa / route are the claims DESIGN.md S15 may make.

usage: python tools/extract_time.py [--reps R] [--configs C3,C5] [--skip-c5] [--profile]
  --profile: C3 only, three rounds of the two extractions after one alignment, nothing printed (the run under rocprofv3 --kernel-trace
             --stats: ex_flags, ex_compact, ex_fill and the scans)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def workload(ctx, name, reps):
    gs = synth.make_config(name)
    N = len(gs)
    ctx.set_genomes(gs)
    sz = ctx.align(_lib.default_params(), fetch=False)
    ctx.coord_index()
    full = (1 << N) - 1
    n_cols = int(sz["n_cols"])
    narr = (C.c_char_p * N)(*[("g%d" % g).encode() for g in range(N)])
    ln = C.c_int64()
    ctx._chk(ctx.L.mauve_write_xmfa(ctx.h, narr, None, C.byref(ln)), "mauve_write_xmfa")
    buf = C.create_string_buffer(ln.value)
    bufs = {}

    def extract(key, require, lists=True):
        t0 = time.perf_counter()
        ns = ctx.extract_select(require=require)
        t1 = time.perf_counter()
        if key not in bufs:
            bufs[key] = (_lib.pinned_empty((N, ns), np.uint8), _lib.pinned_empty(ns, np.int64), _lib.pinned_empty(ns, np.int64), _lib.pinned_empty(ctx._ex_shape[2] + 1, np.int64))
        ctx.extract_fetch(out=bufs[key], lists=lists)
        t2 = time.perf_counter()
        return ns, (t1 - t0) * 1e3, (t2 - t1) * 1e3

    def xmfa():
        n = C.c_int64(ln.value)
        t0 = time.perf_counter()
        ctx._chk(ctx.L.mauve_write_xmfa(ctx.h, narr, buf, C.byref(n)), "mauve_write_xmfa")
        return (time.perf_counter() - t0) * 1e3

    t = {"all": [], "all_select": [], "all_fetch": [], "core": [], "core_select": [], "core_fetch": [], "all_rows": [], "core_rows": [], "xmfa": []}
    n_core = 0
    for rnd in range(reps + 1):                                  # round 0 warms up: code objects, buffer growth, the host copy of the genomes
        na, s1, f1 = extract("all", 0)
        n_core, s2, f2 = extract("core", full)
        _, s3, f3 = extract("all", 0, lists=False)
        _, s4, f4 = extract("core", full, lists=False)
        x = xmfa()
        if rnd:
            t["all_rows"].append(s3 + f3); t["core_rows"].append(s4 + f4)
            t["all"].append(s1 + f1); t["all_select"].append(s1); t["all_fetch"].append(f1)
            t["core"].append(s2 + f2); t["core_select"].append(s2); t["core_fetch"].append(f2)
            t["xmfa"].append(x)
        assert na == n_cols
    out = {"workload": name, "device": ctx.device_name(), "nseq": N, "n_iv": int(sz["n_iv"]), "n_cols": n_cols, "n_core": int(n_core), "xmfa_bytes": int(ln.value), "reps": reps}
    out.update({k + "_ms": spread(v) for k, v in t.items()})
    out["ratio_all"] = out["xmfa_ms"]["median"] / out["all_ms"]["median"]
    out["ratio_core"] = out["xmfa_ms"]["median"] / out["core_ms"]["median"]
    out["ratio_all_rows"] = out["xmfa_ms"]["median"] / out["all_rows_ms"]["median"]
    out["ratio_core_rows"] = out["xmfa_ms"]["median"] / out["core_rows_ms"]["median"]
    return out


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
            gs = synth.make_config("C3")
            ctx.set_genomes(gs)
            ctx.align(_lib.default_params(), fetch=False)
            ctx.coord_index()
            for _ in range(3):
                ctx.extract_columns()
                ctx.extract_columns(require=(1 << len(gs)) - 1)
            return
        for name in [c for c in a.configs.split(",") if not (a.skip_c5 and c == "C5")]:
            print(json.dumps(workload(ctx, name, a.reps)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
