"""Cost of the range map and the interval-overlap join on the GPU.  Prints ONE JSON line: on the C3 alignment at full size
(after mauve_align and mauve_coord_index), `per_genome` seeded ranges of about 1 kb per genome, `reps` rounds after a warm-up round; per
call the median and the spread (min, max) in milliseconds, host clock around calls that end in a stream synchronise:

  map          mauve_map_ranges of all ranges
  map_fetch    ... followed by mauve_map_ranges_fetch of all twelve arrays
  join         mauve_range_overlaps of every piece's nseq extents against one table of all ranges (per_genome entries per genome)
  single_map   mauve_map_ranges and mauve_map_ranges_fetch (all twelve arrays) of the ranges that lie inside one interval
  composition  what a caller had for those ranges before this stage: two mauve_seqpos_to_column batches (the two ends) and two
               mauve_column_positions batches (the extents at the two columns, the second with nearest); it gives neither n_res nor the
               extent of a row that is gapped at the first column, and it cannot take a range that crosses an interval border

The composition and the map are compared once, in the warm-up round (columns, and the extents wherever the row has a residue in the first
column).  All arrays are pageable numpy arrays, as a Python caller passes them.

usage: python tools/feature_time.py [--reps R] [--per-genome K]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--per-genome", type=int, default=5000)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        gs = synth.make_config("C3")
        N = len(gs)
        ctx.set_genomes(gs)
        res = ctx.align(_lib.default_params())
        ctx.coord_index()
        rng = np.random.default_rng(21)
        seq = np.repeat(np.arange(N, dtype=np.int32), a.per_genome)
        lo = np.concatenate([rng.integers(1, len(g) - 1200, a.per_genome) for g in gs]).astype(np.int64)
        hi = lo + rng.integers(800, 1200, len(lo))
        sizes = ctx.map_ranges(seq, lo, hi)
        m = ctx.map_ranges_fetch()
        one = np.flatnonzero((np.diff(m["piece_off"]) == 1) & (m["covered"] == hi - lo + 1))         # inside one interval
        s1, lo1, hi1 = seq[one], lo[one], hi[one]
        q_seq = np.tile(np.arange(N, dtype=np.int32), sizes["n_piece"])
        t = {k: [] for k in ("map", "map_fetch", "join", "single_map", "composition")}
        for rnd in range(a.reps + 1):                            # round 0 warms up: code objects, buffer growth
            t0 = time.perf_counter()
            ctx.map_ranges(seq, lo, hi)
            t1 = time.perf_counter()
            ctx.map_ranges(seq, lo, hi)
            m = ctx.map_ranges_fetch()
            t2 = time.perf_counter()
            n_hit, _, _ = ctx.range_overlaps((seq, lo, hi), (q_seq, m["ext_left"].reshape(-1), m["ext_right"].reshape(-1)))
            t3 = time.perf_counter()
            ctx.map_ranges(s1, lo1, hi1)
            w = ctx.map_ranges_fetch()
            t4 = time.perf_counter()
            iv_a, col_a = ctx.seqpos_to_column(s1, lo1)
            iv_b, col_b = ctx.seqpos_to_column(s1, hi1)
            first, last = np.minimum(col_a, col_b), np.maximum(col_a, col_b)
            pos_a, _ = ctx.column_positions(iv_a, first)
            ctx.column_positions(iv_a, last, nearest=True)
            t5 = time.perf_counter()
            if rnd == 0:
                assert np.array_equal(iv_a, iv_b) and np.array_equal(w["piece_iv"], iv_a) and np.array_equal(w["piece_col"], first), "the two routes differ"
                assert np.array_equal(w["piece_len"], last - first + 1), "the two routes differ"
                here = pos_a != 0                                # the row has a residue in the first column: its position is one end of the extent
                ends = np.where(pos_a < 0, w["ext_right"], w["ext_left"])
                assert np.array_equal(ends[here], pos_a[here]), "the two routes differ"
                assert int(n_hit.min()) >= 0
                continue
            for k, v in (("map", t1 - t0), ("map_fetch", t2 - t1), ("join", t3 - t2), ("single_map", t4 - t3), ("composition", t5 - t4)):
                t[k].append(v * 1e3)
        out = {"workload": "C3", "device": ctx.device_name(), "nseq": N, "n_iv": int(res["n_iv"]), "n_cols": int(res["n_cols"]), "reps": a.reps,
               "n_query": sizes["n_query"], "n_piece": sizes["n_piece"], "n_single": int(len(one)), "join_table": int(len(seq)), "join_queries": int(len(q_seq)),
               "join_hits_mean": float(n_hit.mean())}
        out.update({k + "_ms": spread(v) for k, v in t.items()})
        print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
