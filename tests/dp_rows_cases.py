"""The cases of tests/test_gpu_dp_rows_per_lane.py and one process of it.  The one-wave scan sweep (dp_batch.hip: dp3_interval) holds 1, 2, 3
or 4 rows (orientation A) or columns (B) of a step on every lane, by the length of the dimension on the lanes: 33..64 one, 65..128 two,
129..192 three, the rest four.  These are the smallest shapes at which the three-row form can go wrong: the lane dimension at and around
128 and 192, both orientations, profiles that grow across those edges between the steps of one interval, an empty member, the last row at
each of a lane's three positions and on lane 63, and long runs of X and Y that the walk follows across lane borders.

usage: python -m tests.dp_rows_cases <reference file>

The DP routes are switches read once per process, so the test starts one child per route; the oracle's results are computed once by the
parent (reference) and handed over in a file.  Before every launch the child writes a line "[job] <name>" to stderr, so that the parent
can tell which of the library's MAUVE_TRACE lines belongs to which launch."""
import pickle
import sys

import numpy as np

from tests import scoring_schemes as SS
from tests.align_helpers import seqs

LANE_DIMS = (127, 128, 129, 130, 131, 160, 190, 191, 192, 193)
SCHEMES = ("default", "asym", "unit")


def planted(rng, L, at, k, div=0.03):
    """(a, b, c): a of L bases, b = a with k unrelated bases inserted at `at`, c = a without its k bases from `at`; b and c lightly mutated"""
    a = rng.integers(0, 4, L, dtype=np.uint8)

    def mut(x):
        x = x.copy()
        hit = rng.random(len(x)) < div
        x[hit] = (x[hit] + 1) % 4
        return x
    b = np.concatenate([a[:at], rng.integers(0, 4, k, dtype=np.uint8), a[at:]])
    c = np.concatenate([a[:at], a[at + k:]])
    return a, mut(b), mut(c)


def intervals():
    """list of (what, interval): every interval has five sequence slots (one launch holds them all), the unused ones empty"""
    rng = np.random.default_rng(1293)
    out = []

    def add(what, iv):
        iv = list(iv)
        out.append((what, iv + [np.zeros(0, np.uint8)] * (5 - len(iv))))
    for L in LANE_DIMS:
        # the profile on the lanes (a short partner: few columns, orientation A) and the sequence on the lanes (a short profile: few rows, B) ...
        a, b = seqs(rng, [L, L // 3])
        add("A/short/%d" % L, [a, b])
        add("B/short/%d" % L, [b, a])
        # ... and partners of nearly the same length, a little shorter and a little longer: a long diagonal, whichever way the rule turns it
        a, b = seqs(rng, [L, L - 3])
        add("A/near/%d" % L, [a, b])
        add("B/near/%d" % L, [b, a])
    for m in (130, 131, 132, 190, 191, 192):                  # the last row on each of its lane's positions; 190..192: on lane 63
        add("last/%d" % m, seqs(rng, [m, 50]))
        add("last/t/%d" % m, seqs(rng, [50, m]))
    # profiles that grow across 128 and across 192 between the steps
    add("grow/3/128", seqs(rng, [122, 127, 131], 0.2))
    add("grow/3/192", seqs(rng, [186, 191, 189], 0.2))
    add("grow/5/128", seqs(rng, [118, 124, 127, 131, 126], 0.2))
    add("grow/5/192", seqs(rng, [180, 186, 189, 184, 190], 0.2))
    add("grow/5/both", seqs(rng, [100, 125, 150, 170, 191], 0.2))
    add("empty/middle", seqs(rng, [150, 0, 160]))
    add("empty/two", seqs(rng, [131, 0, 0, 140, 135]))
    # a 40-base insertion and a 40-base deletion: the walk runs 40 cells along one gap state, across lane borders, either way round
    a, b, c = planted(rng, 150, 61, 40)
    for what, iv in (("ins", [a, b]), ("ins/t", [b, a]), ("del", [a, c]), ("del/t", [c, a]), ("both", [c, b]), ("three", [a, b, c])):
        add("planted/" + what, iv)
    # small steps first, then a sequence of more than one band: a workgroup entry (MAUVE_DP_WIDE_MIN=1) whose first steps are its first wave's
    for i, l in enumerate(([150, 160, 140, 300], [190, 185, 300], [131, 60, 129, 0, 280])):
        add("mixed/%d" % i, seqs(rng, l))
    a, b, c = planted(rng, 180, 100, 40)
    add("planted/180/del", [a, c])
    add("planted/180/del/t", [c, a])
    return out


def scheme(name):
    return (SS.HOXD70,) + SS.DEFAULT_GAPS if name == "default" else SS.SCHEMES[name]


def reference():
    """the oracle's columns and scores -> {scheme name: [(cols, score), ...]} in the order of intervals()"""
    from oracle import pyoracle as O
    ivs = [iv for _, iv in intervals()]
    return {name: [O.align_interval(iv, scoring=SS.make(O.Scoring, *scheme(name))) for iv in ivs] for name in SCHEMES}


def run(ref_path):
    from mauvealigner_amd import _lib
    with open(ref_path, "rb") as f:
        ref = pickle.load(f)
    cases = intervals()
    ivs = [iv for _, iv in cases]
    ctx = _lib.Context(0)
    done = 0
    try:
        for name in SCHEMES:
            sys.stderr.write("[job] %s\n" % name)
            sys.stderr.flush()
            cols, score = ctx.dp_batch(ivs, scoring=SS.make(_lib.Scoring, *scheme(name)))
            for (what, iv), c, s, (ec, es) in zip(cases, cols, score, ref[name]):
                assert len(c) == len(ec) and np.array_equal(c, ec) and int(s) == es, (name, what, [len(x) for x in iv], int(s), es)
                done += 1
    finally:
        ctx.close()
    print("OK %d" % done)


if __name__ == "__main__":
    run(sys.argv[1])
