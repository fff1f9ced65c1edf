"""One process of tests/test_gpu_repeat_penalty.py::test_device_chain_equals_host_chain: a progressive alignment with the repeat
penalty on of a C4-shaped set with planted repeats; the parent runs it once as is and once with MAUVE_HOST_CHAIN=1.
usage: python -m tests.repeat_worker <out.npz>"""
import sys

import numpy as np


def main():
    out = sys.argv[1]
    from mauvealigner_amd import _lib, synth
    from tests.test_gpu_repeat_penalty import repeat_genomes
    gs = synth.make_config("C4", scale=0.02)
    rep = repeat_genomes(len(gs), 20000, 9, copies=16)
    gs = [np.concatenate([g, r]) for g, r in zip(gs, rep)]      # every genome carries the same planted repeat family
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
        ctx.set_repeat_penalty(0)
    finally:
        ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
