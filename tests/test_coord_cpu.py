"""CPU-side checks of the coordinate translation: the numpy restatement of tests/coord_ref.py, which is the expected value of
the GPU tests, against the definition itself -- a walk over every interval, column by column, with a running next position per genome --
and the new entry points in the export list of the built library."""
import os

import numpy as np

from mauvealigner_amd import _lib, synth
from oracle import pyoracle as O
from tests.coord_ref import CoordRef

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("mauve_coord_index", "mauve_coord_index_alignment", "mauve_coord_index_size", "mauve_column_positions", "mauve_seqpos_to_column", "mauve_translate_positions")


def _walk(left, right, rev, col_off, cols):
    """the definition: per interval a running next position per genome.  -> per column the positions (0 = no residue), the residue last
    seen at or before it and the first residue of the interval (all signed), and per residue (genome, position) -> (interval, column)"""
    n_iv, N = left.shape
    pos = np.zeros((len(cols), N), np.int64)
    before = np.zeros((len(cols), N), np.int64)
    first = np.zeros((len(cols), N), np.int64)
    where = {}
    for i in range(n_iv):
        nxt = [int(right[i, g]) if rev[i, g] else int(left[i, g]) for g in range(N)]
        seen = [0] * N
        for c in range(int(col_off[i]), int(col_off[i + 1])):
            for g in range(N):
                if cols[c] >> g & 1:
                    assert left[i, g] != 0
                    where[(g, nxt[g])] = (i, c - int(col_off[i]))
                    pos[c, g] = seen[g] = -nxt[g] if rev[i, g] else nxt[g]
                    nxt[g] += -1 if rev[i, g] else 1
                before[c, g] = seen[g]
        for g in range(N):
            if left[i, g]:
                assert nxt[g] == (left[i, g] - 1 if rev[i, g] else right[i, g] + 1)          # the columns hold what the ends say
                first[col_off[i]:col_off[i + 1], g] = -right[i, g] if rev[i, g] else left[i, g]
    return pos, before, first, where


def test_restatement_equals_the_column_walk():
    total = 0
    for name, want in (("g3x5k_inv", 15014), ("g4x3k_tree", 13496), ("g5x3k_unique", 15386)):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        left, right, rev, col_off, cols = z["left"], z["right"], z["reverse"], z["col_off"], z["cols"]
        N = left.shape[1]
        pos, before, first, where = _walk(left, right, rev, col_off, cols)
        assert len(where) == want, (name, len(where))
        R = CoordRef(left, right, rev, col_off, cols)
        iv = np.repeat(np.arange(len(left)), np.diff(col_off))
        col = np.arange(len(cols)) - col_off[iv]
        # rule 1, both modes: every column
        p0, d0 = R.column_positions(iv, col, nearest=False)
        assert np.array_equal(p0, pos)
        assert np.array_equal(d0, ((pos != 0).astype(np.uint64) << np.arange(N, dtype=np.uint64)).sum(axis=1).astype(np.uint32))
        p1, d1 = R.column_positions(iv, col, nearest=True)
        assert np.array_equal(p1, np.where(pos != 0, pos, np.where(before != 0, before, first))) and np.array_equal(d1, d0)
        assert np.any((p1 != 0) & (p0 == 0))                                                    # gapped columns occur
        # rule 2: every residue, and rule 3 on top of it
        keys = np.array(sorted(where), np.int64)
        wi, wc = R.seqpos_to_column(keys[:, 0], keys[:, 1])
        exp = np.array([where[tuple(k)] for k in keys.tolist()], np.int64)
        assert np.array_equal(wi, exp[:, 0]) and np.array_equal(wc, exp[:, 1])
        t, td, ti = R.translate_positions(keys[:, 0], keys[:, 1])
        assert np.array_equal(ti, exp[:, 0]) and np.array_equal(t, pos[col_off[exp[:, 0]] + exp[:, 1]])
        assert np.array_equal(np.abs(t[np.arange(len(keys)), keys[:, 0]]), keys[:, 1])          # the genome asked for: its own position
        total += len(where)
    assert total == 15014 + 13496 + 15386


def test_hand_case_with_a_gap_in_front_of_the_first_residue():
    """the corner the fixtures above do not have: a present genome gapped in the interval's first columns (rule 1, nearest: the first
    residue after the column), on both strands; an absent genome stays 0 in either mode"""
    left, right, rev = np.array([[1, 11, 21, 0]]), np.array([[5, 12, 22, 0]]), np.array([[0, 0, 1, 0]], np.int8)
    cols = np.array([1, 1, 7, 7, 1], np.uint32)
    R = CoordRef(left, right, rev, [0, 5], cols)
    pos, before, first, where = _walk(left, right, rev, np.array([0, 5]), cols)
    p0, d0 = R.column_positions([0] * 5, range(5))
    p1, d1 = R.column_positions([0] * 5, range(5), nearest=True)
    assert p0.tolist() == pos.tolist() == [[1, 0, 0, 0], [2, 0, 0, 0], [3, 11, -22, 0], [4, 12, -21, 0], [5, 0, 0, 0]]
    assert p1.tolist() == np.where(pos != 0, pos, np.where(before != 0, before, first)).tolist()
    assert p1[0].tolist() == [1, 11, -22, 0] and p1[1].tolist() == [2, 11, -22, 0] and p1[4].tolist() == [5, 12, -21, 0]
    assert d0.tolist() == d1.tolist() == [1, 1, 7, 7, 1]
    assert R.seqpos_to_column([2, 2, 1, 3, 0], [22, 21, 12, 5, 6])[1].tolist() == [2, 3, 3, -1, -1]


def test_uncovered_positions_are_reported_as_such():
    """add_unaligned = 0 leaves bases out of the alignment: rule 2 answers (-1, -1) exactly for the bases no [left, right] holds"""
    gs = synth.make_config("C4", scale=0.02)
    a = O.align(gs, O.default_params(add_unaligned=0))["aln"]
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    for g, seq in enumerate(gs):
        p = np.arange(1, len(seq) + 1, dtype=np.int64)
        iv, col = R.seqpos_to_column(np.full(len(p), g), p)
        cov = R.covered(g, len(seq))
        assert cov.any() and not cov.all(), g                   # both classes occur
        assert 0.005 < 1 - cov.mean() < 0.2, (g, 1 - cov.mean())
        assert np.array_equal(iv >= 0, cov) and np.array_equal(col >= 0, cov)
        hit = np.flatnonzero(cov)
        assert np.all(a["left"][iv[hit], g] <= p[hit]) and np.all(p[hit] <= a["right"][iv[hit], g])
        back, _ = R.column_positions(iv[hit], col[hit])
        assert np.array_equal(np.abs(back[:, g]), p[hit])       # the column found holds that very base


def test_new_entry_points_are_exported():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
