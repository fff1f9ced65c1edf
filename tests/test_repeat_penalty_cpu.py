"""CPU-side checks of the repeat penalty (progressiveMauve --repeat-penalty): the new exports and constants of the
built library, the CPU reference of tests/repeat_ref.py on hand-computed cases, the oracle's restatement of S11d against that
reference and end to end, the penalized golden fixture, and the mirror's mems::penalize_repeats."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, synth
from oracle import pyoracle as O
from tests import repeat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_exports_and_constants():
    L = _lib.load()
    for s in ("mauve_set_repeat_penalty", "mauve_seed_multiplicity", "mauve_match_sp_scores_repeat"):
        assert hasattr(L, s), s
        assert s in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "mauve_hip.h")) as f:
        hdr = f.read()
    consts = {k: int(v) for k, v in re.findall(r"#define MAUVE_REPEAT_PENALTY_(\w+) (\d+)", hdr)}
    assert consts == {"OFF": 0, "NEGATIVE": 1, "ZERO": 2}
    assert (_lib.REPEAT_PENALTY_OFF, _lib.REPEAT_PENALTY_NEGATIVE, _lib.REPEAT_PENALTY_ZERO) == (0, 1, 2)
    assert (R.OFF, R.NEGATIVE, R.ZERO) == (0, 1, 2)


def test_null_context_is_refused():
    L = _lib.load()
    assert L.mauve_set_repeat_penalty(None, 1) == -1
    assert L.mauve_seed_multiplicity(None, 0, _lib.C.c_uint64(7), None) == -1


def _codes(s):
    return np.array(["ACGT".index(ch) for ch in s], np.uint8)


def test_reference_multiplicity_hand_cases():
    solid3, solid4 = 0b111, 0b1111
    # one mer on both strands: ACG and CGT are one canonical mer; a base touched by the unique window GTT counts as unique
    assert R.multiplicity(_codes("ACGTT"), solid3).tolist() == [2, 2, 1, 1, 1]
    assert R.multiplicity(_codes("AAAAA"), solid3).tolist() == [3] * 5
    # ACGT and GTAC are their own reverse complements: one window, counted once
    assert R.multiplicity(_codes("ACGT"), solid4).tolist() == [1] * 4
    assert R.window_counts(_codes("ACGTACGT"), solid4).tolist() == [2, 2, 1, 2, 2]
    assert R.multiplicity(_codes("ACGTACGT"), solid4).tolist() == [2, 2, 1, 1, 1, 1, 2, 2]
    # shorter than the span: no window, every base 1
    assert R.multiplicity(_codes("AC"), solid3).tolist() == [1, 1]
    # a contig join in front of base 3: the two windows across it are invalid, the two others still count each other
    assert R.window_counts(_codes("AAAAAA"), solid3, contig_starts=[0, 3]).tolist() == [2, 0, 0, 2]
    assert R.multiplicity(_codes("AAAAAA"), solid3, contig_starts=[0, 3]).tolist() == [2] * 6
    # an ambiguous base: no window covers it validly -> 1
    inv = np.zeros(7, bool); inv[3] = True
    assert R.multiplicity(_codes("AAAAAAA"), solid3, invalid=inv).tolist() == [2, 2, 2, 1, 2, 2, 2]
    # saturation at 255
    assert R.multiplicity(np.zeros(400, np.uint8), solid3).tolist() == [255] * 400


def test_reference_pair_penalty_hand_cases():
    s = np.array([100, 100, 100, 100, -50, 0, 91])
    r = np.array([1, 2, 3, 255, 7, 9, 4])
    assert R.penalize(s, r, R.OFF).tolist() == s.tolist()
    assert R.penalize(s, r, R.NEGATIVE).tolist() == [100, 0, -33, -99, -50, 0, -45]
    assert R.penalize(s, r, R.ZERO).tolist() == [100, 50, 33, 0, -50, 0, 22]


def test_reference_match_scores_hand_case():
    # two genomes, one forward match of 3 columns and its reverse-strand twin; identity scores 10, mismatch -5
    M = np.full((4, 4), -5); np.fill_diagonal(M, 10)
    g0, g1 = _codes("ACGTA"), _codes("TACGT")
    m0, m1 = np.array([1, 2, 3, 1, 1], np.uint8), np.array([1, 1, 1, 2, 3], np.uint8)
    length = np.array([3, 3])
    start = np.array([[1, 2], [3, -2]])             # ACG/ACG; GTA against the reverse complement of ACG (= CGT): G/C T/G A/T
    off = R.sp_scores_repeat([g0, g1], [m0, m1], length, start, R.OFF, M)
    assert off.tolist() == [30, -15]
    # forward: columns (p0=0,p1=1) r=1, (1,2) r=2, (2,3) r=3 -> 10 + 0 + 10*(2-3)/3 = 10 + 0 - 3
    neg = R.sp_scores_repeat([g0, g1], [m0, m1], length, start, R.NEGATIVE, M)
    zero = R.sp_scores_repeat([g0, g1], [m0, m1], length, start, R.ZERO, M)
    assert neg.tolist() == [7, -15] and zero.tolist() == [18, -15]


def test_mirror_declares_penalize_repeats():
    """progressiveMauve.cpp:606-609 assigns the libMems global: a program doing the same compiles against the mirror"""
    src = r'''
#include "libMems/ProgressiveAligner.h"
using namespace mems;
int main(int argc, char **)
{
    penalize_repeats = true;
    if (argc > 1) penalize_repeats = false;
    mems::ProgressiveAligner aligner(2);
    (void)aligner;
    return mems::penalize_repeats ? 0 : 1;
}
'''
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "rp.cpp")
        with open(p, "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", p, "-o", os.path.join(td, "rp.o")])
    with open(os.path.join(ROOT, "include", "libMems", "ProgressiveAligner.h")) as f:
        hdr = f.read()
    assert "inline bool penalize_repeats = false;" in hdr


def _oracle_patterns():
    """every rank of w = 9..31 (spans 13..49, 32- and 64-bit keys), a solid and the coding seed"""
    pats = [O.get_seed(w, r) for w in range(9, 32) for r in range(3)]
    return [p for p in pats if p] + [O.get_seed(12, O.SOLID_SEED), O.get_seed(11, O.CODING_SEED)]


def test_oracle_multiplicity_matches_reference():
    """orc_seed_multiplicity (written from S11d.1-2) equals the numpy reference: planted forward and reverse-complement copies,
    palindromic windows, more than 255 copies, genomes of span - 1, span and span + 1 bases, every rank of w = 9..31"""
    rng = np.random.default_rng(21)
    gs = R.repeat_genomes(2, 6000, 13, copies=10, elem=(200, 400))
    half = rng.integers(0, 4, 12).astype(np.uint8)
    pal = np.concatenate([half, synth.revcomp(half)])            # a palindromic 24-base stretch: its windows at the centre are their own rc
    for k in range(6):
        gs[1][300 + 900 * k:300 + 900 * k + 24] = pal
    gs.append(np.concatenate([np.tile(rng.integers(0, 4, 60).astype(np.uint8), 280), rng.integers(0, 4, 500).astype(np.uint8)]))
    pats = _oracle_patterns()
    assert max(O.seed_length(p) for p in pats) == 49
    seen_sat = seen_rep = False
    for pat in pats:
        span = O.seed_length(pat)
        short = [rng.integers(0, 4, span + d).astype(np.uint8) for d in (-1, 0, 1)] + [np.zeros(span + 1, np.uint8)]
        for g in gs + short:
            got, exp = O.seed_multiplicity(g, pat), R.multiplicity(g, pat)
            assert got.dtype == np.uint8 and np.array_equal(got, exp), (hex(pat), len(g), np.flatnonzero(got != exp)[:10])
            seen_sat |= bool((got == 255).any()); seen_rep |= bool(((got > 1) & (got < 255)).any())
    assert seen_sat and seen_rep
    centre = gs[1][306:318]
    assert np.array_equal(centre, synth.revcomp(centre))          # (the centre window of every planted stretch is its own rc)
    assert O.seed_multiplicity(np.zeros(0, np.uint8), pats[0]).shape == (0,)


def test_oracle_penalized_scores_match_reference():
    """orc_match_sp_scores_repeat (S11d.3) equals the numpy reference in both modes, with reverse and absent components; OFF is
    orc_match_sp_scores"""
    gs = R.repeat_genomes(4, 12000, 7, elem=(200, 600))
    M = np.array([list(r) for r in O.default_scoring().matrix], np.int64)
    for pat in (O.get_seed(11, 0), O.get_seed(13, 1)):
        ln, st = O.find_matches(gs, pat)
        st = st.copy()
        st[::5, 2] = 0
        st[1::7, 0] = 0
        assert (st < 0).any() and (st == 0).any()
        mults = [O.seed_multiplicity(g, pat) for g in gs]
        plain = O.match_sp_scores(gs, ln, st)
        assert np.array_equal(O.match_sp_scores_repeat(gs, mults, ln, st, R.OFF), plain)
        assert np.array_equal(plain, R.sp_scores_repeat(gs, mults, ln, st, R.OFF, M))
        for mode in (R.NEGATIVE, R.ZERO):
            got = O.match_sp_scores_repeat(gs, mults, ln, st, mode)
            assert np.array_equal(got, R.sp_scores_repeat(gs, mults, ln, st, mode, M)), mode
            assert (got < plain).any()
    # the hand case of test_reference_match_scores_hand_case through the oracle
    M2 = O.default_scoring()
    for a in range(4):
        for b in range(4):
            M2.matrix[a][b] = 10 if a == b else -5
    g0, g1 = _codes("ACGTA"), _codes("TACGT")
    m0, m1 = np.array([1, 2, 3, 1, 1], np.uint8), np.array([1, 1, 1, 2, 3], np.uint8)
    ln, st = np.array([3, 3]), np.array([[1, 2], [3, -2]])
    assert O.match_sp_scores_repeat([g0, g1], [m0, m1], ln, st, R.NEGATIVE, M2).tolist() == [7, -15]
    assert O.match_sp_scores_repeat([g0, g1], [m0, m1], ln, st, R.ZERO, M2).tolist() == [18, -15]


@pytest.mark.parametrize("mode", [R.NEGATIVE, R.ZERO])
def test_oracle_blocks_and_repeats_end_to_end(mode):
    """the genomes' own search pairs the tagged repeat copies out of order: under OFF they hold the blocks apart, with the penalty
    the blocks form one LCB; length scoring ignores the mode"""
    gs, _, _ = R._blocks_and_repeats(3, tag=16)
    p = O.default_params(lcb_scoring=1, seed_weight=11, lcb_weight=10000)

    def n_lcb(r):
        return len(set(r["aln"]["anchor_lcb"].tolist()))
    off = O.align(gs, p)
    assert n_lcb(off) > 1
    assert n_lcb(O.align(gs, p, repeat_penalty=mode)) == 1
    keys = ("left", "right", "reverse", "col_off", "cols", "dp_score", "anchor_start")
    lp = O.default_params(seed_weight=11, lcb_weight=10000)
    a, b = O.align(gs, lp)["aln"], O.align(gs, lp, repeat_penalty=mode)["aln"]
    assert all(np.array_equal(a[k], b[k]) for k in keys)
    again = O.align(gs, p, repeat_penalty=R.OFF)["aln"]            # the explicit OFF is the plain entry
    assert all(np.array_equal(again[k], off["aln"][k]) for k in keys)


def test_oracle_identity_without_repeats():
    """where every multiplicity is 1 every mode gives the OFF result: align, progressive_align and along a given tree"""
    gs = synth.make_config("C4", scale=0.004)[:4]
    kw = dict(lcb_scoring=1, seed_weight=15)
    pat = O.get_seed(15, 0)
    assert all((O.seed_multiplicity(g, pat) == 1).all() for g in gs)
    tree = (np.array([-1, -1, -1, -1, 0, 1, 4], np.int32), np.array([-1, -1, -1, -1, 3, 2, 5], np.int32))
    keys = ("left", "right", "reverse", "col_off", "cols", "dp_score")
    base = [O.align(gs, O.default_params(**kw))["aln"], O.progressive_align(gs, O.default_progressive_params(**kw))["aln"],
            O.progressive_align(gs, O.default_progressive_params(**kw), tree=tree)["aln"]]
    for mode in (R.NEGATIVE, R.ZERO):
        got = [O.align(gs, O.default_params(**kw), repeat_penalty=mode)["aln"],
               O.progressive_align(gs, O.default_progressive_params(**kw), repeat_penalty=mode)["aln"],
               O.progressive_align(gs, O.default_progressive_params(**kw), tree=tree, repeat_penalty=mode)["aln"]]
        for x, y in zip(got, base):
            assert all(np.array_equal(x[k], y[k]) for k in keys), mode


def test_oracle_unknown_mode_is_refused():
    gs = R.repeat_genomes(2, 3000, 1)
    with pytest.raises(RuntimeError):
        O.align(gs, O.default_params(lcb_scoring=1), repeat_penalty=3)
    with pytest.raises(RuntimeError):
        O.progressive_align(gs, O.default_progressive_params(), repeat_penalty=-1)


def test_golden_repeat_fixture_reproduces():
    """the penalized progressive fixture (NEGATIVE, default progressive parameters) is what the oracle computes, and differs from OFF"""
    z = np.load(os.path.join(GOLDEN, "g4x6k_repeat.npz"))
    N = int(z["nseq"])
    gs = [z["genome%d" % g] for g in range(N)]
    names = ["g%d" % g for g in range(N)]
    r = O.progressive_align(gs, O.default_progressive_params(), names=names, want_xmfa=True, repeat_penalty=int(z["repeat_penalty"]))
    for k in ("left", "right", "reverse", "col_off", "cols", "dp_score"):
        assert np.array_equal(r["aln"][k], z[k]), k
    assert np.array_equal(r["tree"][0], z["tree_left"]) and np.array_equal(r["tree"][1], z["tree_right"])
    with open(os.path.join(GOLDEN, "g4x6k_repeat.xmfa")) as f:
        assert f.read() == r["xmfa"]
    off = O.progressive_align(gs, O.default_progressive_params())["aln"]
    assert not all(np.array_equal(off[k], z[k]) for k in ("left", "right", "cols"))
    pat = int(z["pattern"])
    assert max(int(O.seed_multiplicity(g, pat).max()) for g in gs) > 1
