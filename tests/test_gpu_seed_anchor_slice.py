"""A finder pass clears and scans the hit table only where one of its hits can be anchored (anchor_range, seed_pass.hip): the slice of
the lowest genome of the wanted set, or -- no set wanted -- every genome but the highest.  seed_mums must equal the oracle's find_matches
whichever slice a pass takes, with the stale entries that earlier passes on the same context left outside it, and with a match at the
very first window of the slice, where the run detection's look-back reaches into the genome in front.

Four unrelated random genomes of about 20 k bases with planted common stretches:
  ALL : in all four, at the END of genome 0 (a full-mask pass leaves hits in the last windows of genome 0, the halo of genome 1's slice)
  S12 : in genomes 1 and 2 only, at the START of genome 1
  S13 : in genomes 1 and 3 only;  S23 : in genomes 2 and 3 only (reverse complement in genome 3)."""
import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
PAT = O.get_seed(11, 0)
LENS = (20000, 20013, 19991, 20007)


def _rc(s):
    return (3 - s)[::-1]


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(77)
    gs = [rng.integers(0, 4, L, dtype=np.uint8) for L in LENS]
    s_all, s12, s13, s23 = (rng.integers(0, 4, n, dtype=np.uint8) for n in (1500, 1200, 1000, 1000))
    gs[0][LENS[0] - 1500:] = s_all
    gs[1][:1200] = s12; gs[1][5000:6500] = s_all; gs[1][9000:10000] = s13
    gs[2][3000:4200] = s12; gs[2][8000:9500] = s_all; gs[2][12000:13000] = s23
    gs[3][1000:2500] = s_all; gs[3][6000:7000] = s13; gs[3][15000:16000] = _rc(s23)
    return gs


@pytest.fixture(scope="module")
def ctx(genomes):
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    c.set_genomes(genomes)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected(genomes):
    """the oracle's lists, made once: mask -> (length, start)"""
    return {mask: O.find_matches(genomes, PAT, mode=O.MODE_MEM, mask=mask, extend=True) for mask in (0b1111, 0, 0b0110)}


def _same(ctx, expected, mask):
    ln, st = ctx.seed_mums(PAT, mode=O.MODE_MEM, mask=mask, extend=True)
    eln, est = expected[mask]
    assert np.array_equal(ln, eln) and np.array_equal(st, est)


def _long_with(est, eln, genomes_in):
    """matches of >= 900 bases whose components are exactly the given genomes"""
    want = np.zeros(est.shape[1], bool); want[list(genomes_in)] = True
    return ((est != 0) == want).all(axis=1) & (eln >= 900)


def test_full_mask_anchors_in_genome_0(ctx, expected):
    eln, est = expected[0b1111]
    assert len(eln) > 0 and _long_with(est, eln, (0, 1, 2, 3)).any()
    _same(ctx, expected, 0b1111)


def test_no_mask_anchors_up_to_the_last_but_one_genome(ctx, expected):
    eln, est = expected[0]
    assert _long_with(est, eln, (1, 3)).any() and _long_with(est, eln, (2, 3)).any()      # anchored in genomes 1 and 2 = N - 2
    assert (est[_long_with(est, eln, (2, 3))][:, 3] < 0).any()
    _same(ctx, expected, 0)


def test_inner_slice_after_a_full_pass(ctx, expected):
    """mask 0b0110 anchors in genome 1; the full-mask pass before it leaves its hits in genome 0, up to the last window in front of
    the slice, and the pass without a mask leaves them in genome 2 behind it"""
    eln, est = expected[0b0110]
    first = _long_with(est, eln, (1, 2)) & (est[:, 1] == 1)
    assert first.any(), "no match at the first window of the anchor genome"
    for before in (0b1111, 0):
        _same(ctx, expected, before)
        _same(ctx, expected, 0b0110)
    _same(ctx, expected, 0b1111)
