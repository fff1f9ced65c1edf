"""What the extension of the repeat map costs (mauve_repeat_matches) on the GPU.  Prints ONE JSON line; per input:

  enumerate_ms  mauve_seed_match_enumerate's counting call (extract, sort, runs) on the genome, multiplicities 2 .. 32
  repeat_ms     mauve_repeat_matches on the same genome and range: the same extract and sort, then the window table, the walk of every
                family head, the compaction and the order.  Both are host clocks around calls that end in a device synchronise, alternated,
                median of `reps` after one warm-up of each; the difference is what the extension costs
  families / records / starts   the counting call's matches; the repeat map's records and their components
  hits / rounds / max_rounds    with --rounds: family heads walked, the 64-offset rounds of all walks, the most rounds of one hit (from the
                library's MAUVE_TRACE line, in a child process of its own so that the trace's synchronisations stay out of the times)

Inputs: genome 0 of config C3 (5 Mbp) at w = 15 and w = 11, and a 2 Mbp random genome with one 50 kb segment duplicated (one diagonal
with 50 k hits: every hit but the first stops at the hit before it).

usage: python tools/repeat_map_time.py [--reps R] [--rounds]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402


def inputs():
    c3 = synth.make_config("C3")[0]
    rng = np.random.default_rng(50)
    dup = rng.integers(0, 4, 2_000_000).astype(np.uint8)
    dup[1_200_000:1_250_000] = dup[300_000:350_000]
    return [("C3 genome 0, w 15", c3, _lib.get_seed(15, 0)), ("C3 genome 0, w 11", c3, _lib.get_seed(11, 0)),
            ("2 Mbp, 50 kb duplicated, w 15", dup, _lib.get_seed(15, 0))]


def counting_call(ctx, pat):
    n, ns = _lib.C.c_int64(), _lib.C.c_int64()
    ctx._chk(ctx.L.mauve_seed_match_enumerate(ctx.h, 0, _lib.C.c_uint64(pat), _lib.C.c_int64(2), _lib.C.c_int64(32), 0, _lib.C.byref(n), _lib.C.byref(ns),
                                              None, None, None), "mauve_seed_match_enumerate")
    return n.value, ns.value


def repeat_call(ctx, pat):
    n, ns = _lib.C.c_int64(), _lib.C.c_int64()
    ctx._chk(ctx.L.mauve_repeat_matches(ctx.h, 0, _lib.C.c_uint64(pat), _lib.C.c_int64(2), _lib.C.c_int64(32), _lib.C.byref(n), _lib.C.byref(ns)),
             "mauve_repeat_matches")
    return n.value, ns.value


def timed(fn, *a):
    t0 = time.perf_counter()
    r = fn(*a)
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", action="store_true")
    ap.add_argument("--trace-child", type=int, default=-1)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        if a.trace_child >= 0:                                # one repeat pass under MAUVE_TRACE: the library prints the rounds
            _, g, pat = inputs()[a.trace_child]
            ctx.set_genomes([g])
            repeat_call(ctx, pat)
            return
        out = {"device": ctx.device_name(), "inputs": []}
        for k, (name, g, pat) in enumerate(inputs()):
            ctx.set_genomes([g])
            te, tr, fam, rec = [], [], None, None
            for i in range(a.reps + 1):
                t, fam = timed(counting_call, ctx, pat)
                te.append(t)
                t, rec = timed(repeat_call, ctx, pat)
                tr.append(t)
            row = {"input": name, "windows": int(len(g) - _lib.seed_length(pat) + 1), "enumerate_ms": round(float(np.median(te[1:])), 3),
                   "repeat_ms": round(float(np.median(tr[1:])), 3), "repeat_ms_min_max": [round(min(tr[1:]), 3), round(max(tr[1:]), 3)],
                   "families": fam[0], "records": rec[0], "starts": rec[1]}
            if a.rounds:
                env = dict(os.environ)
                env["MAUVE_TRACE"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", str(k)], env=env, capture_output=True, text=True, timeout=600)
                m = re.search(r"repeat map: (\d+) windows, (\d+) hits, (\d+) records, (\d+) rounds, most rounds of one hit (\d+)", r.stderr)
                if r.returncode or not m:
                    raise RuntimeError("trace child failed: " + r.stderr[-2000:])
                row.update(hits=int(m.group(2)), rounds=int(m.group(4)), max_rounds=int(m.group(5)))
            out["inputs"].append(row)
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
