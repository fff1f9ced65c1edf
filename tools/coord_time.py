"""Cost of the coordinate translation on the GPU.  Prints ONE JSON line per workload (C3, C5 at full size, after mauve_align):

  index_build_ms   mauve_coord_index on the columns the alignment left in HBM (the call ends in a stream synchronise); median of `reps`
  fetch_ms         mauve_align_fetch of the alignment -- what the host route needs before it can answer anything
  ref_build_ms     the numpy restatement's own index (tests/coord_ref.py: cumulative sums of the bit columns)
  queries          per batch size (10^6, 10^7), order (random, sorted by position: the gene-table case) and kind (columns, seqpos, translate):
                     device_ms / device_qps   the batch from page-locked query and answer arrays, upload and download included,
                                              the call ends in a stream synchronise; warmed up, median of `reps`
                     ref_ms                   the numpy restatement on the same queries (one run; the answers are compared)
  host_route_ms    fetch_ms + ref_build_ms + ref_ms of the 10^6 random translate batch, beside device_route_ms = index_build_ms + device_ms

usage: python tools/coord_time.py [--reps R] [--configs C3,C5] [--skip-c5] [--sizes 1000000,10000000] [--profile]
  --profile: C3 only, three index builds and three backbone calls after one alignment, nothing printed (the run under rocprofv3:
             coord_build against bb_tile_count on the same columns)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402
from tests.coord_ref import CoordRef  # noqa: E402


def pinned_like(a):
    p = _lib.pinned_empty(a.shape, a.dtype)
    p[...] = a
    return p


def timed(fn, reps):
    fn()                                                     # warm-up: code objects, buffer growth
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), r


def workload(ctx, name, sizes, reps):
    gs = synth.make_config(name)
    N = len(gs)
    ctx.set_genomes(gs)
    sz = ctx.align(_lib.default_params(), fetch=False)
    build_ms, _ = timed(ctx.coord_index, reps)
    t0 = time.perf_counter()
    a = ctx._fetch(_lib.AlignSizes(**sz))
    fetch_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    ref_build_ms = (time.perf_counter() - t0) * 1e3
    out = {"workload": name, "device": ctx.device_name(), "nseq": N, "n_iv": int(a["n_iv"]), "n_cols": int(a["n_cols"]),
           "index_build_ms": build_ms, "fetch_ms": fetch_ms, "ref_build_ms": ref_build_ms, "queries": {}}
    rng = np.random.default_rng(14)
    lens = np.array([len(g) for g in gs], np.int64)
    for n in sizes:
        x = rng.integers(0, len(a["cols"]), n)
        seq = rng.integers(0, N, n).astype(np.int32)
        pos = rng.integers(1, lens[seq] + 1)
        for order in ("random", "sorted"):
            if order == "sorted":
                x = np.sort(x)
                o = np.lexsort((pos, seq))
                seq, pos = seq[o], pos[o]
            iv = np.searchsorted(a["col_off"], x, side="right") - 1
            col = x - a["col_off"][iv]
            piv, pcol, pseq, ppos = pinned_like(iv), pinned_like(col), pinned_like(seq), pinned_like(pos)
            o1 = (_lib.pinned_empty((n, N), np.int64), _lib.pinned_empty(n, np.uint32))
            o2 = (_lib.pinned_empty(n, np.int64), _lib.pinned_empty(n, np.int64))
            o3 = (_lib.pinned_empty((n, N), np.int64), _lib.pinned_empty(n, np.uint32), _lib.pinned_empty(n, np.int64))
            kinds = {
                "columns": (lambda: ctx.column_positions(piv, pcol, nearest=True, out=o1), lambda: R.column_positions(iv, col, nearest=True)),
                "seqpos": (lambda: ctx.seqpos_to_column(pseq, ppos, out=o2), lambda: R.seqpos_to_column(seq, pos)),
                "translate": (lambda: ctx.translate_positions(pseq, ppos, out=o3), lambda: R.translate_positions(seq, pos)),
            }
            for kind, (dev, ref) in kinds.items():
                ms, got = timed(dev, reps)
                t0 = time.perf_counter()
                want = ref()
                ref_ms = (time.perf_counter() - t0) * 1e3
                same = all(np.array_equal(u, v) for u, v in zip(got, want))
                out["queries"]["%d_%s_%s" % (n, order, kind)] = {"device_ms": ms, "device_qps": n / (ms * 1e-3), "ref_ms": ref_ms, "equal": bool(same)}
                del want
    k = "%d_random_translate" % sizes[0]
    out["device_route_ms"] = build_ms + out["queries"][k]["device_ms"]
    out["host_route_ms"] = fetch_ms + ref_build_ms + out["queries"][k]["ref_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="C3,C5")
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        if a.profile:
            ctx.set_genomes(synth.make_config("C3"))
            ctx.align(_lib.default_params(), fetch=False)
            for _ in range(3):
                ctx.backbone()
                ctx.coord_index()
            return
        sizes = [int(s) for s in a.sizes.split(",")]
        for name in [c for c in a.configs.split(",") if not (a.skip_c5 and c == "C5")]:
            print(json.dumps(workload(ctx, name, sizes, a.reps)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
