"""Cost and effect of the repeat penalty (progressiveMauve --repeat-penalty) on the GPU.  Prints ONE JSON line:

  multiplicity_ms  the multiplicity pass alone at C4 and C5 for the root pattern: a first mauve_seed_multiplicity after an upload
                   (pass + copy of genome 0's bytes) minus a second one that finds the cache (copy only); median of `reps`
  c4_step_ms       the C4 progressive step as bench.py times it (upload from page-locked memory, mauve_progressive_align at the call
                   site's defaults, compact fetch) with the penalty off, negative and zero, alternated; median of `steps` each
  accuracy         sensitivity / PPV (mauvealigner_amd.accuracy) against the generator's truth on 8 x 2 Mbp genomes of one
                   ancestor that carries planted families of diverged repeats, per mode

usage: python tools/repeat_time.py [--steps K] [--reps R] [--skip-c5] [--profile-step K]
  --profile-step K: only K penalized (negative) C4 steps after one warm-up, nothing printed (the run under rocprofv3)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, accuracy, synth  # noqa: E402

MODES = {"off": _lib.REPEAT_PENALTY_OFF, "negative": _lib.REPEAT_PENALTY_NEGATIVE, "zero": _lib.REPEAT_PENALTY_ZERO}


def root_pattern(gs):
    return _lib.get_seed(_lib.default_seed_weight(sum(len(g) for g in gs) // len(gs)), 0)


def multiplicity_ms(ctx, gs, reps):
    pat = root_pattern(gs)
    out = []
    for _ in range(reps + 1):
        ctx.set_genomes(gs)
        t0 = time.perf_counter(); ctx.seed_multiplicity(0, pat); t1 = time.perf_counter()
        ctx.seed_multiplicity(0, pat); t2 = time.perf_counter()
        out.append(((t1 - t0) - (t2 - t1)) * 1e3)
    return float(np.median(out[1:]))                     # (the first includes code-object loading and buffer growth)


def pack_pinned(gs):
    """the packed genomes in one page-locked block, as bench.py's step starts from them"""
    ws = [_lib.pack_codes(g) for g in gs]
    block = _lib.pinned_empty(sum(len(w) for w in ws), np.uint64)
    out, at = [], 0
    for w in ws:
        block[at:at + len(w)] = w
        out.append(block[at:at + len(w)])
        at += len(w)
    return out, [len(g) for g in gs]


def c4_steps(ctx, gs, steps, modes):
    p = _lib.default_progressive_params()
    bufs = _lib.ResultBuffers()
    packed, lens = pack_pinned(gs)
    times = {m: [] for m in modes}
    for i in range(steps + 1):
        for m in modes:
            ctx.set_repeat_penalty(MODES[m])
            t0 = time.perf_counter()
            ctx.set_genomes_packed(packed, lens)
            ctx.progressive_align(p, fetch=True, out=bufs, compact=True)
            if i:
                times[m].append((time.perf_counter() - t0) * 1e3)
    ctx.set_repeat_penalty(0)
    return {m: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for m, v in times.items()}


def repeat_workload(n=8, L=2_000_000, seed=61, families=((40, 1500, 0.05), (60, 400, 0.08), (20, 5000, 0.03)), div=0.02):
    """n genomes of one ancestor (star, point mutations and short indels at div/2 per branch, tracked) that carries planted families
    (copies, element length, divergence of every copy from the element); every copy has its own ancestor coordinates, so the truth
    pairs copy k with copy k only"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, L).astype(np.uint8)
    for copies, ln, d in families:
        e = rng.integers(0, 4, ln).astype(np.uint8)
        for k, p in enumerate(rng.choice(L - ln, copies, replace=False).tolist()):
            c = synth.mutate(e, d, rng, indel_frac=0.0)[:ln]
            anc[p:p + len(c)] = synth.revcomp(c) if k % 2 else c
    gs, origins = [], []
    for g in range(n):
        x, o = synth.mutate(anc, div / 2, np.random.default_rng(seed * 100 + g), origin=np.arange(1, L + 1, dtype=np.int64))
        gs.append(x); origins.append(o)
    return gs, origins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--profile-step", type=int, default=0)
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        c4 = synth.make_config("C4")
        if a.profile_step:
            c4_steps(ctx, c4, a.profile_step, ["negative"])
            return
        out = {"device": ctx.device_name(), "multiplicity_ms": {}, "multiplicity_windows": {}}
        out["multiplicity_ms"]["C4"] = multiplicity_ms(ctx, c4, a.reps)
        out["multiplicity_windows"]["C4"] = int(sum(len(g) - _lib.seed_length(root_pattern(c4)) + 1 for g in c4))
        out["c4_step_ms"] = c4_steps(ctx, c4, a.steps, list(MODES))
        gs, origins = repeat_workload()
        acc = {}
        for m, v in MODES.items():
            ctx.set_repeat_penalty(v)
            ctx.set_genomes(gs)
            r = ctx.progressive_align(_lib.default_progressive_params())
            s = accuracy.score_alignment(r, origins)
            acc[m] = {"sensitivity": round(s["sensitivity"], 6), "ppv": round(s["ppv"], 6), "n_iv": int(r["n_iv"])}
        ctx.set_repeat_penalty(0)
        out["accuracy"] = {"workload": "8 x 2 Mbp star, divergence 0.02, planted families (copies, length, divergence) "
                                       "(40, 1500, 0.05), (60, 400, 0.08), (20, 5000, 0.03)", **acc}
        if not a.skip_c5:
            c5 = synth.make_config("C5")
            out["multiplicity_ms"]["C5"] = multiplicity_ms(ctx, c5, a.reps)
            out["multiplicity_windows"]["C5"] = int(sum(len(g) - _lib.seed_length(root_pattern(c5)) + 1 for g in c5))
        print(json.dumps(out))
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
