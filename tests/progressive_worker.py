"""The refinement and walk sets of tests/progressive_cases.py through the library, in this process or in a child that has switches of
the library set in its environment (tests/test_gpu_progressive.py):  python -m tests.progressive_worker <reference.pickle>

reference() is computed once by the parent (no GPU): per refinement set and number of rounds the interval assembled from
tests/progressive_ref.py and the oracle's counters, per walk set the oracle's result.  run() compares the library with all of it and
runs check_walk on every result."""
import pickle
import sys

import numpy as np

from tests import progressive_cases as Cs
from tests import progressive_ref as R

FIELDS = ("left", "right", "reverse", "col_off", "cols", "dp_score")


def params(mod, case, **kw):
    p = dict(case["params"])
    p.update(kw)
    return mod.default_params(**p)


def reference():
    from oracle import pyoracle as O
    ref = {}
    for c in list(Cs.refinement_sets()) + [Cs.clade_set()]:
        expect = Cs.expect_clade if c["name"] == "clade" else Cs.expect_refinement
        for rounds in Cs.ROUNDS:
            e = O.progressive_align(c["genomes"], params(O, c, refine_rounds=rounds), tree=c["tree"])["aln"]
            ref[("refine", c["name"], rounds)] = (expect(c, rounds), e)
    for c in Cs.walk_sets():
        ref[("walk", c["name"])] = O.progressive_align(c["genomes"], params(O, c), tree=c["tree"])["aln"]
    return ref


def job(name):
    sys.stderr.write("[job] %s\n" % name)
    sys.stderr.flush()


def same(res, e, what):
    for k in FIELDS:
        assert np.array_equal(res[k], e[k]), (what, k)
    assert res["n_gap_dp"] == e["n_gap_dp"] and res["n_dp_cells"] == e["n_dp_cells"], (what, "counters")


def run(ctx, _lib, ref):
    for c in list(Cs.refinement_sets()) + [Cs.clade_set()]:
        ctx.set_genomes(c["genomes"])
        for rounds in Cs.ROUNDS:
            job("refine/%s/%d" % (c["name"], rounds))
            want, e = ref[("refine", c["name"], rounds)]
            r = ctx.progressive_align(params(_lib, c, refine_rounds=rounds), tree=c["tree"])
            for k in ("left", "right", "col_off", "cols", "dp_score"):
                assert np.array_equal(r[k], want[k]), (c["name"], rounds, k)
            assert not r["reverse"].any()
            same(r, e, (c["name"], rounds))
            R.check_walk(c["genomes"], r["tree"], r)
    for c in Cs.walk_sets():
        job("walk/" + c["name"])
        ctx.set_genomes(c["genomes"])
        r = ctx.progressive_align(params(_lib, c), tree=c["tree"])
        same(r, ref[("walk", c["name"])], c["name"])
        if c["table"] is not None:
            assert R.interval_table(r, multi_only=False) == c["table"], c["name"]
        R.check_walk(c["genomes"], r["tree"], r)


def main():
    from mauvealigner_amd import _lib
    with open(sys.argv[1], "rb") as f:
        ref = pickle.load(f)
    ctx = _lib.Context(0)
    try:
        run(ctx, _lib, ref)
    finally:
        ctx.close()
    print("OK")


if __name__ == "__main__":
    main()
