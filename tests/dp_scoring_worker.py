"""The cases of tests/test_gpu_dp_scoring.py and one process of it.  The DP routes are switches read once per process
(MAUVE_DP_ONE_WAVE, MAUVE_DP_NOSCAN, MAUVE_DP_WIDE_MIN, MAUVE_DP_NO_WIDE, MAUVE_DP_CLUSTER, MAUVE_CANON_DEVICE_MIN), so the parent
starts one child per route; the cases are built from fixed seeds, the oracle's results are computed once by the parent
(reference / whole_reference) and handed over in a file.

usage: python -m tests.dp_scoring_worker dp <reference file> <group>[,<group>...]
       python -m tests.dp_scoring_worker whole <reference file>
       python -m tests.dp_scoring_worker front

Before every launch the child writes a line "[job] <name>" to stderr, so that the parent can tell which of the library's
MAUVE_TRACE lines (the class counts of a launch) belongs to which case."""
import pickle
import sys

import numpy as np

from tests import scoring_schemes as SS
from tests.align_helpers import long_gap_pair, seqs, whole_compare      # noqa: F401  (the cases below use them; tests import them from here too)

HOLE_GAP_OPEN = -50000


def shapes():
    """group -> list of (case name, intervals of one launch): the smallest shapes that reach each kernel family's edges"""
    rng = np.random.default_rng(77)
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    a = rnd(800)
    g = {}
    # sub-wave groups: class boundaries (16 / 32 rows), unequal neighbours, empty members, single bases
    g["subwave"] = [
        ("pairs", [seqs(rng, l, 0.2) for l in ([16, 16], [17, 3], [16, 176], [33, 100], [1, 1], [5, 0], [0, 7])]),
        ("triples", [seqs(rng, l, 0.2) for l in ([9, 8, 30], [16, 0, 100], [0, 0, 5])]),
        ("fives", [seqs(rng, [int(rng.integers(0, 13)) for _ in range(5)], 0.2) for _ in range(100)]),
    ]
    # one wave per interval: both orientations of the scan, the 256-row band edge, tall and flat, unrelated and identical sequences
    g["onewave"] = [
        ("pairs", [seqs(rng, list(s)) for s in ((700, 20), (20, 700), (257, 255), (255, 257), (65, 64), (1, 900), (900, 1), (300, 299))]
                  + [[a, rnd(30)], [a[:300], a[:300].copy()]]),
        ("fives", [seqs(rng, [250, 260, 255, 0, 258]), seqs(rng, [20, 18, 1200, 22, 19])]),
    ]
    # a workgroup per interval: one and two super-bands (2048 rows) either way, band edges, a short last stripe; small pairs beside them
    g["wide"] = [
        ("pairs", [seqs(rng, list(s)) for s in ((2049, 300), (300, 2049), (257, 3), (3, 257), (512, 513), (1100, 257), (64 * 17 + 1, 700))]
                  + [seqs(rng, [int(rng.integers(1, 60)), int(rng.integers(1, 60))]) for _ in range(50)]),
        ("fives", [seqs(rng, [300, 10, 0, 2100, 12])]),
    ]
    return g


def swapped_pair(rng, L):
    """a = A...A + Z, b = Z' + C...C: all that the two share lies L columns off the diagonal, and what the band does reach (the A's
    and C's of Z) is worth less, whatever gaps cost -- the band is live even where gaps are free"""
    z = rng.integers(0, 4, L, dtype=np.uint8)
    z2 = z.copy()
    mut = rng.random(L) < 0.05
    z2[mut] = (z2[mut] + 1) % 4
    return [np.concatenate([np.zeros(L, np.uint8), z]), np.concatenate([z2, np.ones(L, np.uint8)])]


def match_cases(rng, genomes, lengths=(1, 63, 64, 65, 300, 417)):
    """matches over `genomes` for the sum-of-pairs scorers: forward, reverse and absent components at every length, at least two
    components present, the first present one forward"""
    N = len(genomes)
    ln, st = [], []
    for L in lengths:
        for _ in range(6):
            row = []
            for g in range(N):
                u = rng.random()
                p = int(rng.integers(1, len(genomes[g]) - L + 2))
                row.append(0 if u < 0.25 else (-p if u < 0.6 else p))
            while sum(1 for s in row if s) < 2:
                g = int(rng.integers(0, N))
                if not row[g]:
                    row[g] = int(rng.integers(1, len(genomes[g]) - L + 2))
            first = min(g for g in range(N) if row[g])
            row[first] = abs(row[first])
            ln.append(L)
            st.append(row)
    return np.array(ln, np.int64), np.array(st, np.int64)


def dp_jobs():
    """every launch of the DP tests: (group, name, (matrix, gap_open, gap_extend), band_from or None, intervals)"""
    jobs = []
    for group, cases in shapes().items():
        for scheme in SS.NAMES:
            for name, ivs in cases:
                jobs.append((group, "%s/%s/%s" % (group, name, scheme), SS.SCHEMES[scheme], None, ivs))
    rng = np.random.default_rng(78)
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    cut = long_gap_pair(rng, 3000, 500)
    tiny = [[np.array([1], np.uint8), np.array([2], np.uint8)], [np.zeros(0, np.uint8), rnd(9)], [rnd(64), rnd(65)], [rnd(129), rnd(1)]]
    swap = swapped_pair(rng, 1100)
    for scheme in ("asym", "zero_gaps", "huge"):
        jobs.append(("banded", "banded/cut/%s" % scheme, SS.SCHEMES[scheme], 1000, [cut]))
        jobs.append(("banded", "banded/swap/%s" % scheme, SS.SCHEMES[scheme], 1000, [swap]))
        jobs.append(("banded", "banded/tiny/%s" % scheme, SS.SCHEMES[scheme], 0, tiny))
    # the admission boundary of the scans under `edge`: total length 600 is admitted, 700 is not; both have a dimension above 256
    jobs.append(("boundary", "boundary/edge", SS.SCHEMES["edge"], None, [seqs(rng, [400, 300]), seqs(rng, [350, 250])]))
    # workgroup entries that the scans do not admit because of their LENGTH, in a call with no band and an ordinary scheme
    jobs.append(("hole", "hole/1600", (SS.ASYM, HOLE_GAP_OPEN, -30), None, [seqs(rng, [1600, 1600])]))
    jobs.append(("hole", "hole/32way", (SS.HOXD70,) + SS.DEFAULT_GAPS, None, [seqs(rng, [660] * 32, 0.1), seqs(rng, [650] * 32, 0.1)]))
    return jobs


def _oracle_dp(O, ivs, scheme, band_from, transpose=False, banded=None):
    m, go, ge = scheme
    sc = SS.make(O.Scoring, SS.transposed(m) if transpose else m, go, ge)
    out = []
    for iv in ivs:
        b = (band_from is not None and max(len(x) for x in iv) > band_from) if banded is None else banded
        c, s = O.align_interval(iv, scoring=sc, banded=b)
        out.append((c, s))
    return out


def reference():
    """the oracle's columns and scores of every job -> {job name: [(cols, score), ...]}"""
    from oracle import pyoracle as O
    return {name: _oracle_dp(O, ivs, scheme, band_from) for _, name, scheme, band_from, ivs in dp_jobs()}


def run_dp(ref_path, groups):
    from mauvealigner_amd import _lib
    with open(ref_path, "rb") as f:
        ref = pickle.load(f)
    ctx = _lib.Context(0)
    done = 0
    try:
        for group, name, scheme, band_from, ivs in dp_jobs():
            if group not in groups:
                continue
            sys.stderr.write("[job] %s\n" % name)
            sys.stderr.flush()
            cols, score = ctx.dp_batch(ivs, scoring=SS.make(_lib.Scoring, *scheme), band_from=band_from)
            for iv, c, s, (ec, es) in zip(ivs, cols, score, ref[name]):
                assert len(c) == len(ec) and np.array_equal(c, ec) and int(s) == es, (name, [len(x) for x in iv], int(s), es)
            done += 1
    finally:
        ctx.close()
    print("OK %d" % done)


# ---- the whole path under a scheme: align, align with score-weighted LCBs, progressive_align at the call site's defaults ----
WHOLE_SCHEMES = ("asym", "unit")
WHOLE_CONFIGS = (("C3", 0.02), ("C4", 0.02))
WHOLE_KINDS = ("align", "align_sp", "progressive")


def whole_genomes(cfg, scale):
    from mauvealigner_amd import synth
    return synth.make_config(cfg, scale=scale)


def whole_params(mod, kind, scoring):
    """the parameter structure of binding `mod` (_lib or pyoracle) for one kind of run"""
    p = mod.default_progressive_params() if kind == "progressive" else mod.default_params(lcb_scoring=1 if kind == "align_sp" else 0)
    p.scoring = scoring
    return p


def whole_oracle(O, gs, kind, scoring):
    names = ["g%d" % i for i in range(len(gs))]
    fn = O.progressive_align if kind == "progressive" else O.align
    return fn(gs, whole_params(O, kind, scoring), names=names, want_xmfa=True)


def whole_reference():
    from oracle import pyoracle as O
    ref = {}
    for cfg, scale in WHOLE_CONFIGS:
        gs = whole_genomes(cfg, scale)
        for scheme in WHOLE_SCHEMES:
            for kind in WHOLE_KINDS:
                ref[(cfg, scheme, kind)] = whole_oracle(O, gs, kind, SS.fill(O.Scoring, scheme))
    return ref


def whole_run(ctx, _lib, gs, kind, scoring):
    ctx.set_genomes(gs)
    names = ["g%d" % i for i in range(len(gs))]
    fn = ctx.progressive_align if kind == "progressive" else ctx.align
    return fn(whole_params(_lib, kind, scoring), names=names, want_xmfa=True)


def run_whole(ctx, _lib, ref):
    for cfg, scale in WHOLE_CONFIGS:
        gs = whole_genomes(cfg, scale)
        for scheme in WHOLE_SCHEMES:
            for kind in WHOLE_KINDS:
                sys.stderr.write("[job] whole/%s/%s/%s\n" % (cfg, scheme, kind))
                sys.stderr.flush()
                whole_compare(whole_run(ctx, _lib, gs, kind, SS.fill(_lib.Scoring, scheme)), ref[(cfg, scheme, kind)], kind, len(gs))


# ---- the device front end of the DP stage (mauve_align sizes and orders its intervals on the device) at the admission boundary ----
def front_genomes():
    """two genomes that share their flanks and nothing in between: one gap of 1600 x 1600 unrelated bases, among the small ones of the flanks"""
    from mauvealigner_amd import synth
    rng = np.random.default_rng(91)
    left, right = rng.integers(0, 4, 4000, dtype=np.uint8), rng.integers(0, 4, 4000, dtype=np.uint8)
    g = [np.concatenate([left, rng.integers(0, 4, 1600, dtype=np.uint8), right]) for _ in range(2)]
    g[1] = np.concatenate([synth.mutate(left, 0.05, rng), g[1][4000:5600], synth.mutate(right, 0.05, rng)])
    return g


def front_scoring(cls):
    return SS.make(cls, SS.ASYM, HOLE_GAP_OPEN, -30)


def run_front():
    from mauvealigner_amd import _lib
    from oracle import pyoracle as O
    gs = front_genomes()
    e = O.align(gs, O.default_params(scoring=front_scoring(O.Scoring), recursive=0), names=["g0", "g1"], want_xmfa=True)   # (recursive anchoring would cut the gap at chance matches)
    st, ln = np.abs(e["aln"]["anchor_start"]), e["aln"]["anchor_length"]
    gap = (st[1:] - st[:-1] - ln[:-1, None]).sum(axis=1)                     # bases between two anchors, both genomes together
    assert int(gap.max()) >= 2685 and e["aln"]["n_gap_dp"] > 1, gap.max()    # the big gap is not admitted (test_gpu_dp_scoring), small ones beside it
    ctx = _lib.Context(0)
    try:
        sys.stderr.write("[job] front\n")
        sys.stderr.flush()
        ctx.set_genomes(gs)
        r = ctx.align(_lib.default_params(scoring=front_scoring(_lib.Scoring), recursive=0), names=["g0", "g1"], want_xmfa=True)
        whole_compare(r, e, "align", 2)
    finally:
        ctx.close()
    print("OK")


def main():
    if sys.argv[1] == "front":
        run_front()
        return
    mode, ref_path = sys.argv[1], sys.argv[2]
    if mode == "dp":
        run_dp(ref_path, sys.argv[3].split(","))
        return
    from mauvealigner_amd import _lib
    with open(ref_path, "rb") as f:
        ref = pickle.load(f)
    ctx = _lib.Context(0)
    try:
        run_whole(ctx, _lib, ref)
    finally:
        ctx.close()
    print("OK")


if __name__ == "__main__":
    main()
