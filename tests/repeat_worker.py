"""One process of tests/test_gpu_repeat_penalty.py::test_device_chain_equals_host_chain: a progressive alignment with the repeat
penalty on of a C4-shaped set with planted repeats; the parent runs it on each chain route (as is,
MAUVE_CANON_DEVICE_MIN=1, MAUVE_HOST_CHAIN=1) and compares every run with the oracle.
usage: python -m tests.repeat_worker <out.npz>"""
import sys

import numpy as np


def worker_genomes(scale=0.02):
    """C4 at `scale`, every genome with the same planted repeat family appended (tests.repeat_ref.repeat_genomes)"""
    from mauvealigner_amd import synth
    from tests.repeat_ref import repeat_genomes
    gs = synth.make_config("C4", scale=scale)
    rep = repeat_genomes(len(gs), 20000, 9, copies=16)
    return [np.concatenate([g, r]) for g, r in zip(gs, rep)]


def main():
    out = sys.argv[1]
    from mauvealigner_amd import _lib
    gs = worker_genomes()
    ctx = _lib.Context(0)
    res = {}
    try:
        p = _lib.default_progressive_params()
        pat = _lib.get_seed(_lib.default_seed_weight(sum(len(g) for g in gs) // len(gs)), 0)
        ctx.set_genomes(gs)
        res["max_mult"] = np.array(max(int(ctx.seed_multiplicity(g, pat).max()) for g in range(len(gs))))
        for mode in (1, 2):
            ctx.set_repeat_penalty(mode)
            r = ctx.progressive_align(p)
            for k in ("cols", "col_off", "dp_score", "left", "right", "reverse"):
                res["m%d_%s" % (mode, k)] = r[k]
            res["m%d_n_gap_dp" % mode] = np.array(r["n_gap_dp"])
        ctx.set_repeat_penalty(0)
    finally:
        ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
