"""Cost of the alignment text on the GPU: text_time.py [--reps R] [--configs C3,C4] [--profile]
Prints ONE JSON line per workload (bench's C3 and C4 at full size, after the alignment), the two routes to the XMFA text alternating in one
process, `reps` rounds after a warm-up round; per figure the median and the spread (min, max) in milliseconds:

  a        the host route: mauve_write_xmfa twice, the length call and the fill call, as _lib's _fetch(want_xmfa=True) does
  b        the device route: mauve_coord_index + mauve_alignment_text + mauve_alignment_text_fetch into a page-locked buffer
  b_index / b_text / b_fetch   its three calls (each ends in a stream synchronise: index build, layout and generation, copy-out)
  b_noindex                    b_text + b_fetch, for a caller that holds the index already

The two texts are compared byte for byte in every round.  --profile: C3 only, three rounds of the device route after one alignment, nothing
printed (the run under rocprofv3 --kernel-trace --stats: tx_rows, tx_blocks, tx_head, tx_body and the scans)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def align(ctx, name):
    gs = synth.make_config(name, 1.0)
    ctx.set_genomes(gs)
    if name == "C4":
        return len(gs), ctx.progressive_align(_lib.default_progressive_params(), fetch=False)
    return len(gs), ctx.align(_lib.default_params(seed_weight=15), fetch=False)


def workload(ctx, name, reps):
    N, sz = align(ctx, name)
    names = ["g%d" % g for g in range(N)]
    narr = (C.c_char_p * N)(*[s.encode() for s in names])
    pin = None
    t = {k: [] for k in ("a", "a_len", "a_fill", "b", "b_index", "b_text", "b_fetch", "b_noindex")}
    nb = 0
    for rnd in range(reps + 1):                                  # round 0 warms up: code objects, buffer growth, the host copy of the genomes
        t0 = time.perf_counter()
        ln = C.c_int64()
        ctx._chk(ctx.L.mauve_write_xmfa(ctx.h, narr, None, C.byref(ln)), "mauve_write_xmfa")
        t1 = time.perf_counter()
        buf = C.create_string_buffer(ln.value)
        ctx._chk(ctx.L.mauve_write_xmfa(ctx.h, narr, buf, C.byref(ln)), "mauve_write_xmfa")
        t2 = time.perf_counter()
        host = buf.raw[:ln.value - 1]
        u0 = time.perf_counter()
        ctx.coord_index()
        u1 = time.perf_counter()
        nb, _ = ctx.alignment_text(names=names)
        u2 = time.perf_counter()
        if pin is None:
            pin = _lib.pinned_empty(nb, np.uint8)
        dev = ctx.alignment_text_fetch(out=pin)
        u3 = time.perf_counter()
        if nb != len(host) or dev.tobytes() != host:
            raise SystemExit("text_time: the device text (%d bytes) differs from mauve_write_xmfa's (%d bytes)" % (nb, len(host)))
        if rnd:
            for k, v in (("a", t2 - t0), ("a_len", t1 - t0), ("a_fill", t2 - t1), ("b", u3 - u0), ("b_index", u1 - u0), ("b_text", u2 - u1), ("b_fetch", u3 - u2),
                         ("b_noindex", u3 - u1)):
                t[k].append(v * 1e3)
    out = {"workload": name, "device": ctx.device_name(), "nseq": N, "n_iv": int(sz["n_iv"]), "n_cols": int(sz["n_cols"]), "text_bytes": int(nb), "identical": True, "reps": reps}
    out.update({k + "_ms": spread(v) for k, v in t.items()})
    out["ratio_b"] = out["a_ms"]["median"] / out["b_ms"]["median"]
    out["ratio_b_noindex"] = out["a_ms"]["median"] / out["b_noindex_ms"]["median"]
    out["fetch_GBps"] = nb / out["b_fetch_ms"]["median"] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="C3,C4")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        if a.profile:
            N, _ = align(ctx, "C3")
            ctx.coord_index()
            for _ in range(3):
                ctx.alignment_text(names=["g%d" % g for g in range(N)])
            return
        for name in a.configs.split(","):
            print(json.dumps(workload(ctx, name, a.reps)), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
