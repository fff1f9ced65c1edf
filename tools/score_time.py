"""Cost of scoring an alignment against a correct one on the GPU.  Prints ONE JSON line: C3 at full size, T = mauve_align
with defaults, fetched; C = mauve_align with extend_lcbs = 0, indexed on the device (mauve_coord_index).  After a warm-up round, `reps`
rounds of

  truth   mauve_score_truth of T's arrays: the upload of the columns, their check against the interval ends and the index build
  score   mauve_score_alignment into page-locked records: the count and the copy-out, the call ends in a stream synchronise

with the median and the spread (min, max) in milliseconds, and the totals of the records.  For comparison the numpy restatement
tests/score_ref.py is timed once on the same pair of alignments of C3 at --numpy-scale (0.05: where numpy finishes), together with the
device on that small pair; the records of the two must be equal.  ratio_small_scale = numpy / device score there: a comparison at unequal
scale with the full-size figures, and the only ratio DESIGN.md S17 may quote.

usage: python tools/score_time.py [--reps R] [--config C3] [--numpy-scale S]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402
from tests import score_ref  # noqa: E402

KEYS = ("left", "right", "reverse", "col_off", "cols")


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def pair(ctx, gs):
    """T fetched, C left on the device and indexed -> (T arrays, sizes of C)"""
    ctx.set_genomes(gs)
    r = ctx.align(_lib.default_params())
    T = {k: np.array(r[k]) for k in KEYS}
    sz = ctx.align(_lib.default_params(extend_lcbs=0), fetch=False)
    ctx.coord_index()
    return T, sz


def timed(ctx, T, N, reps):
    out = _lib.pinned_empty((N, N, _lib.SCORE_WORDS), np.int64)
    t_truth, t_score = [], []
    for rnd in range(reps + 1):                                  # round 0 warms up: code objects, buffer growth
        t0 = time.perf_counter()
        ctx.score_truth(T)
        t1 = time.perf_counter()
        ctx.score_alignment(out=out)
        t2 = time.perf_counter()
        if rnd:
            t_truth.append((t1 - t0) * 1e3); t_score.append((t2 - t1) * 1e3)
    return out.copy(), t_truth, t_score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--numpy-scale", type=float, default=0.05)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        gs = synth.make_config(a.config)
        N = len(gs)
        T, sz = pair(ctx, gs)
        rec, t_truth, t_score = timed(ctx, T, N, a.reps)
        tot = _lib.score_totals(rec)
        out = {"workload": a.config, "device": ctx.device_name(), "nseq": N, "truth_n_iv": int(T["left"].shape[0]), "truth_n_cols": int(len(T["cols"])),
               "calc_n_iv": int(sz["n_iv"]), "calc_n_cols": int(sz["n_cols"]), "reps": a.reps, "truth_ms": spread(t_truth), "score_ms": spread(t_score),
               "totals": tot, "slots": rec[..., :6].reshape(-1, 6).sum(axis=0).tolist()}
        # the restatement, where it finishes
        gs = synth.make_config(a.config, scale=a.numpy_scale)
        T, sz = pair(ctx, gs)
        Cc = ctx.align(_lib.default_params(extend_lcbs=0))
        ctx.coord_index()
        rec, _, t_small = timed(ctx, T, N, a.reps)
        t0 = time.perf_counter()
        want = score_ref.score_records(T, Cc, N)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        out.update({"numpy_scale": a.numpy_scale, "small_truth_n_cols": int(len(T["cols"])), "small_score_ms": spread(t_small), "numpy_ms": numpy_ms,
                    "small_equal": bool(np.array_equal(rec, want)), "ratio_small_scale": numpy_ms / float(np.median(t_small))})
        print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
