"""Cost of scoring a repeat map against a correct repeat alignment (mauve_repeat_score) on the GPU.  Prints ONE JSON line;
per input, after a warm-up round, `reps` rounds of whole calls, host clock around calls that end in a stream synchronise, as
min - median - max in milliseconds:

  truth_ms     mauve_score_truth of the planted truth: the upload of the columns, their check and the index build
  resident_ms  mauve_repeat_score of the map where mauve_repeat_matches left it (no list), tables into page-locked arrays
  list_ms      mauve_repeat_score of the fetched map handed back as a page-locked list: the same plus the list's upload, minus the reordering

and the sizes (records, components, truth columns and rows), the totals and the four figures.  Inputs: the three of S20's table -- genome 0
of config C3 at w = 15 and w = 11 with the copies of repeat_accuracy.planted_repeats written over it (40 families, elements of 500 to 5 000
bases, 2 to 8 copies, 0 to 5 % divergence), and the 2 Mbp random genome with one 50 kb segment duplicated, whose truth is that segment as a
family of two copies: the one long match spans the extents of a few thousand short ones, so every stab under it walks back over them.
For comparison the plain-Python restatement tests/repeat_score_ref.py is timed once on the 20 kb planted genome of
tests/test_repeat_score_cpu.py (where it finishes), together with the device on the same input; the results must be equal.
ratio_small_scale = Python / device there: the only ratio DESIGN.md S22 may quote, and a comparison at that scale only.

usage: python tools/repeat_score_time.py [--reps R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, repeat_accuracy, synth  # noqa: E402
from tests import repeat_score_ref  # noqa: E402


def spread(v):
    return {"min": round(float(np.min(v)), 3), "median": round(float(np.median(v)), 3), "max": round(float(np.max(v)), 3)}


def planted_over(genome, seed_key):
    """the copies of planted_repeats(len(genome), ...) written over `genome` -> (genome, truth)"""
    rng = np.random.default_rng(seed_key)
    fams = [(int(rng.integers(500, 5001)), int(rng.integers(2, 9)), float(rng.choice([0.0, 0.01, 0.03, 0.05]))) for _ in range(40)]
    p, T = repeat_accuracy.planted_repeats(len(genome), fams, seed_key)
    g = np.array(genome, np.uint8)
    for f in range(T["left"].shape[0]):
        for r in range(T["left"].shape[1]):
            if T["left"][f, r]:
                g[T["left"][f, r] - 1:T["right"][f, r]] = p[T["left"][f, r] - 1:T["right"][f, r]]
    return g, T


def inputs():
    c3, T3 = planted_over(synth.make_config("C3")[0], 22)
    rng = np.random.default_rng(50)
    dup = rng.integers(0, 4, 2_000_000).astype(np.uint8)
    dup[1_200_000:1_250_000] = dup[300_000:350_000]
    Td = dict(left=np.array([[300_001, 1_200_001]], np.int64), right=np.array([[350_000, 1_250_000]], np.int64), reverse=np.zeros((1, 2), np.int8),
              col_off=np.array([0, 50_000], np.int64), cols=np.full(50_000, 3, np.uint32))
    return [("C3 genome 0 + planted repeats, w 15", c3, T3, _lib.get_seed(15, 0)), ("C3 genome 0 + planted repeats, w 11", c3, T3, _lib.get_seed(11, 0)),
            ("2 Mbp, 50 kb duplicated, w 15", dup, Td, _lib.get_seed(15, 0))]


def pinned(a):
    q = _lib.pinned_empty(a.shape, a.dtype)
    q[...] = a
    return q


def timed(ctx, g, T, pat, reps):
    ctx.set_genomes([g])
    records = ctx.repeat_matches(0, pat)
    n, ns, N = len(records[0]), len(records[3]), T["left"].shape[1]
    lst = tuple(pinned(a) for a in records)
    out = dict(pair_records=_lib.pinned_empty((N, N, _lib.REPEAT_SCORE_WORDS), np.int64), comp_hit=_lib.pinned_empty((n,), np.uint32), pair_hit=_lib.pinned_empty((ns,), np.uint32))
    t_truth, t_res, t_list = [], [], []
    res = None
    for rnd in range(reps + 1):                                  # round 0 warms up: code objects, buffer growth
        t0 = time.perf_counter()
        ctx.score_truth(T)
        t1 = time.perf_counter()
        res = ctx.repeat_score(out=out)
        t2 = time.perf_counter()
        keep = {k: res[k].copy() for k in out}
        t3 = time.perf_counter()
        lres = ctx.repeat_score(lst, out=out)
        t4 = time.perf_counter()
        if lres["totals"] != res["totals"] or any(keep[k].tobytes() != lres[k].tobytes() for k in out):
            raise RuntimeError("the resident form and the list form disagree")
        if rnd:
            t_truth.append((t1 - t0) * 1e3); t_res.append((t2 - t1) * 1e3); t_list.append((t4 - t3) * 1e3)
    return records, res, dict(records=n, components=ns, truth_rows=N, truth_cols=int(len(T["cols"])), truth_ms=spread(t_truth), resident_ms=spread(t_res), list_ms=spread(t_list),
                              totals=res["totals"], figures=_lib.repeat_score_ppv(res["totals"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        out = {"device": ctx.device_name(), "reps": a.reps, "inputs": []}
        for name, g, T, pat in inputs():
            _, _, row = timed(ctx, g, T, pat, a.reps)
            out["inputs"].append(dict(input=name, bases=int(len(g)), **row))
        # the restatement, where it finishes
        g, T = repeat_accuracy.planted_repeats(20000, [(300, 2, 0.0), (400, 3, 0.0), (350, 4, 0.0)], 0)
        records, res, row = timed(ctx, g, T, _lib.get_seed(15, 0), a.reps)
        t0 = time.perf_counter()
        want = repeat_score_ref.score(T, records)
        py_ms = (time.perf_counter() - t0) * 1e3
        equal = want["totals"] == res["totals"] and all(np.array_equal(want[k], res[k]) for k in ("pair_records", "comp_hit", "pair_hit"))
        out["small"] = dict(input="20 kb planted, w 15", python_ms=round(py_ms, 3), equal=bool(equal), ratio_small_scale=round(py_ms / row["resident_ms"]["median"], 1), **row)
        print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
