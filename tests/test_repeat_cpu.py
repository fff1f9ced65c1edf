"""The repeat map without a GPU: the plain-Python reference (tests/repeat_map_ref.py) is tied to the oracle -- its
families, taken with extension off, are the oracle's seed match enumeration on every planted case -- it gives the records written out
by hand for the four basic shapes, every planted case (tests/repeat_map_cases.py) yields the record it is aimed at, and the product
library exports the two entry points."""
import numpy as np
import pytest

from mauvealigner_amd import _lib
from oracle import pyoracle as O
from tests import repeat_map_cases as RC
from tests import repeat_map_ref as RM

PATTERNS = {"w15": O.get_seed(15, 0), "solid8": O.get_seed(8, O.SOLID_SEED),
            "w12": O.get_seed(12, 0), "w11": O.get_seed(11, 0)}


def test_library_exports_the_repeat_map():
    L = _lib.load()
    assert hasattr(L, "mauve_repeat_matches") and hasattr(L, "mauve_repeat_fetch")
    assert "mauve_repeat_matches" in _lib.EXPORTS and "mauve_repeat_fetch" in _lib.EXPORTS
    assert hasattr(_lib.Context, "repeat_matches")


def test_reference_reads_the_seed_like_the_oracle():
    for pat in PATTERNS.values():
        care, span = RM.care_offsets(pat)
        assert span == O.seed_length(pat) and len(care) == O.seed_weight(pat)
    rng = np.random.default_rng(5)
    g = rng.integers(0, 4, 700).astype(np.uint8)
    for pat in PATTERNS.values():
        F, R, span = RM.window_mers(g, pat)
        canon, strand = O.mers(g, pat)
        assert [min(f, r) for f, r in zip(F, R)] == canon.tolist() and [int(r < f) for f, r in zip(F, R)] == strand.tolist()


@pytest.mark.parametrize("name", list(PATTERNS))
def test_families_equal_the_oracles_enumeration(name):
    """extension off: one seed-length record per family = O.seed_match_enumerate (which knows no contig table: masks left out)"""
    pat = PATTERNS[name]
    span = O.seed_length(pat)
    for c in RC.all_cases(pat, walks=False) + [RC.walk(pat, 1, 64), RC.walk(pat, 129, 0)]:
        for lo, hi in ((2, 32), (3, 5)):
            fam = RM.repeat_matches(c.codes, pat, lo, hi, extend=False)
            m, o, s = O.seed_match_enumerate(c.codes, pat, lo, hi)
            orc = RM.canonical([(span, tuple(int(x) for x in s[o[i]:o[i + 1]])) for i in range(len(m))])
            assert fam == orc, (c.name, lo, hi)


def _acgt(s):
    return np.array(["ACGT".index(ch) for ch in s], np.uint8)


def test_hand_cases():
    """solid seed of weight 4 (span 4) on sequences short enough to check by eye; every record written out"""
    pat = 0b1111
    E = "ACGGTCA"
    # a direct pair: E at 2 and at 13 (0-based), unlike bases around
    g = _acgt("TT" + E + "AAAC" + E + "CC")
    assert RM.repeat_matches(g, pat) == [(7, (3, 14))]
    # an inverted pair: E at 2, its reverse complement TGACCGT at 12
    g = _acgt("TT" + E + "GAG" + "TGACCGT" + "TT")
    assert RM.repeat_matches(g, pat) == [(7, (3, -13))]
    # a perfect palindrome of 12 bases at 2, arms ACGGTC | GACCGT: the outermost windows start at 2 and 10; after three steps they start
    # at 5 and 7, a fourth would put both at 6 -- the walk stops in front of it.  Arms of 3 + span = 7 bases: 2 .. 8 and 7 .. 13
    g = _acgt("TT" + "ACGGTCGACCGT" + "TT")
    rec = RM.repeat_matches(g, pat)
    assert rec == [(7, (3, -8))], rec
    # F-R-F: E at 2, reverse complement at 12, E at 22: one 3-fold record, the middle component reverse
    g = _acgt("TT" + E + "AAA" + "TGACCGT" + "CCA" + E + "GG")
    assert RM.repeat_matches(g, pat) == [(7, (3, -13, 23))]
    assert RM.repeat_matches(g, pat, max_multi=2) == [] and RM.repeat_matches(g, pat, min_multi=4) == []


@pytest.mark.parametrize("name", list(PATTERNS))
def test_planted_cases_yield_their_records(name):
    """liveness: the reference, on its own, finds in every planted genome the record the case is aimed at"""
    pat = PATTERNS[name]
    cases = RC.all_cases(pat, walks=False)
    assert len(cases) >= 36                                   # of 42 builders: at most the self-complementary pair and the don't-care plants are missing
    for c in cases:
        c.aim(c.reference(pat))


@pytest.mark.parametrize("name", ["w15", "solid8"])
def test_walk_round_cases_yield_their_records(name):
    pat = PATTERNS[name]
    for lo in RC.EDGES:
        for hi in RC.EDGES:
            c = RC.walk(pat, lo, hi)
            c.aim(c.reference(pat))


def test_liveness_examples_named_by_the_rule():
    pat, span = PATTERNS["w15"], 21
    rec = RC.copies(pat, 31).reference(pat)                   # 33 copies
    assert rec and max(len(r[1]) for r in rec) <= 32 and not any(len(r[1]) == 33 for r in rec)
    assert any(len(r[1]) == 32 for r in RC.copies(pat, 30).reference(pat))
    c = RC.inverted(pat, 0, 3 * span)                         # spacer 0: the arms' windows stop one apart, never crossed
    (ln, (s0, s1)), = [r for r in c.reference(pat) if len(r[1]) == 2 and r[1][1] < 0 and r[0] >= 3 * span]
    assert 0 < (-s1 - 1) - ((s0 - 1) + ln - span) <= 2
    c = RC.chain(pat, "span+1")
    rec = c.reference(pat)
    diag = [r for r in rec if len(r[1]) == 2 and r[1][1] - r[1][0] == rec[0][1][1] - rec[0][1][0]]
    assert len(diag) == 2 and diag[0][1][0] + diag[0][0] < diag[1][1][0]             # two records of one diagonal, apart
    rec = RC.chain(pat, "span").reference(pat)
    assert len([r for r in rec if len(r[1]) == 2 and r[1][1] - r[1][0] == rec[0][1][1] - rec[0][1][0]]) == 1
