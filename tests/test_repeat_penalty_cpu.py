"""CPU-side checks of the repeat penalty (progressiveMauve --repeat-penalty): the new exports and constants of the
built library, the CPU reference of tests/repeat_ref.py on hand-computed cases, and the mirror's mems::penalize_repeats."""
import os
import re
import subprocess
import tempfile

import numpy as np

from mauvealigner_amd import _lib
from tests import repeat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
