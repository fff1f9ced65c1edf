"""The seed pass without a value array out of the extraction: seed_extract_all writes the keys and a strand bitmap, and
the first sort pass makes every value from the window's own index and its bit.  seed_mums must equal the oracle's find_matches (MEM mode,
full mask, extension on) where that first pass is row-scanned (> 64 tiles) or reads the raw tile histograms (<= 64), where the last tile
and the last bitmap word are partial, where genome borders fall at every offset inside a thread's four windows, with 32- and 64-bit keys
and with narrow and wide values.  Every input holds an inverted stretch, so the matches there carry the strand bit: a bitmap of zeros
fails.  The paths that keep the value array (a single genome's sorted list) are pinned too."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096


def make_case(lens, seed, rate=0.03):
    """Genomes of exactly the given lengths: substitution-only copies of one ancestor (its first len bases), the middle tenth of genome 1
    replaced by its reverse complement."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, max(lens), dtype=np.uint8)
    gs = []
    for L in lens:
        g = anc[:L].copy()
        hit = np.flatnonzero(rng.random(L) < rate)
        g[hit] = (g[hit] + rng.integers(1, 4, len(hit), dtype=np.uint8)) & 3
        gs.append(g)
    a, b = int(lens[1] * 0.45), int(lens[1] * 0.55)
    gs[1][a:b] = (3 - gs[1][a:b])[::-1]
    return gs


def windows(gs, pat):
    return sum(max(0, len(g) - O.seed_length(pat) + 1) for g in gs)


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, gs, pat):
    full = (1 << len(gs)) - 1
    eln, est = O.find_matches(gs, pat, mode=O.MODE_MEM, mask=full, extend=True)
    assert len(eln) > 0 and (est < 0).any(), "the oracle found no match on the reverse strand: the case does not test the strand bits"
    ctx.set_genomes(gs)
    ln, st = ctx.seed_mums(pat, mode=O.MODE_MEM, mask=full, extend=True)
    assert np.array_equal(ln, eln) and np.array_equal(st, est)


BIG = (90001, 90001, 90001)


@pytest.mark.parametrize("weight", [11, 19])
def test_row_scanned_first_pass(ctx, weight):
    """more than 64 tiles; the last tile and the last bitmap word are partial; weight 19: 64-bit keys"""
    pat = O.get_seed(weight, 0)
    gs = make_case(BIG, 1)
    P = windows(gs, pat)
    assert P > 64 * TILE and P % TILE != 0 and P % 64 != 0
    check(ctx, gs, pat)


def test_raw_first_pass(ctx):
    """at most 64 tiles: the first pass sums the raw tile histograms itself"""
    pat = O.get_seed(11, 0)
    gs = make_case((30011, 30011), 2)
    assert 9216 < windows(gs, pat) <= 64 * TILE
    check(ctx, gs, pat)


@pytest.mark.parametrize("lens", [(20001, 20001, 20001), (20002, 20002, 20002), (20003, 20003, 20003), (20001, 20002, 20003)])
def test_genome_borders_inside_a_thread(ctx, lens):
    """lengths 4k+1, 4k+2, 4k+3: a thread's four windows straddle a genome border at every offset"""
    check(ctx, make_case(lens, 3 + lens[0] % 4 + lens[2] % 4), O.get_seed(11, 0))


_WIDE_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
from mauvealigner_amd import _lib
from oracle import pyoracle as O
from tests.test_gpu_seed_strand_bitmap import BIG, check, make_case
c = _lib.Context(0)
check(c, make_case(BIG, 1), O.get_seed(11, 0))
c.close()
print("child ok")
"""


def test_wide_values():
    """the first case with 64-bit values (MAUVE_WIDE_INDEX=1 is read once per process: a child)"""
    env = dict(os.environ)
    env.update({"MAUVE_WIDE_INDEX": "1", "MAUVE_TRACE": "1"})
    r = subprocess.run([sys.executable, "-c", _WIDE_SCRIPT % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [s for s in r.stderr.splitlines() if "seed pass:" in s]
    assert lines and all("wide window index (64-bit values)" in s for s in lines), lines


def test_single_genome_list_keeps_its_values(ctx):
    """the sorted mer list of one genome (seed_extract with only_seq, full sort, export) still carries a value array"""
    gs = make_case(BIG, 1)
    ctx.set_genomes(gs)
    for w in (11, 19):
        pat = O.get_seed(w, 0)
        mer, pos = ctx.sorted_mer_list(1, pat)
        emer, epos = O.sorted_mer_list(gs[1], pat)
        assert np.array_equal(mer, emer) and np.array_equal(pos, epos)
