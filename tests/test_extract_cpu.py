"""CPU-side checks of the column extraction: the numpy restatement of tests/extract_ref.py, which is the expected value of
the GPU tests, against things it did not produce -- the rows of the committed XMFA texts (the oracle's writer), counts from a separate
column walk, and a scalar walk written out here -- and the new entry points in the export list of the built library."""
import os

import numpy as np
import pytest

from mauvealigner_amd import _lib
from tests.extract_ref import ExtractRef, parse_xmfa, xmfa_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("mauve_default_extract_params", "mauve_extract_select", "mauve_extract_fetch")
# fixture: (columns, core columns with require = all genomes, polymorphic core columns)
COUNTS = {"g2x2k": (2016, 1991, 76), "g3x5k_inv": (5054, 4969, 212), "g4x3k_tree": (4599, 2750, 279), "g5x3k_unique": (3432, 2953, 258),
          "g4x6k_repeat": (6091, 5880, 608)}


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = z["left"].shape[1]
    a = dict(left=z["left"], right=z["right"], reverse=z["reverse"], col_off=z["col_off"], cols=z["cols"])
    return a, [z["genome%d" % g] for g in range(N)]


def ref_of(a, gs, invalid=None):
    return ExtractRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], gs, invalid)


def _walk(a, gs, invalid=None):
    """the definition, scalar: per interval a running next position per genome -> the letters of every column, uint8 [N, n_cols]"""
    n_iv, N = a["left"].shape
    out = np.full((N, len(a["cols"])), ord("-"), np.uint8)
    for i in range(n_iv):
        for g in range(N):
            if not a["left"][i, g]:
                continue
            rev = bool(a["reverse"][i, g])
            nxt = int(a["right"][i, g]) if rev else int(a["left"][i, g])
            for c in range(int(a["col_off"][i]), int(a["col_off"][i + 1])):
                if a["cols"][c] >> g & 1:
                    b = int(gs[g][nxt - 1])
                    out[g, c] = ord("ACGT"[3 - b] if rev else "ACGT"[b])
                    if invalid is not None and invalid[g] is not None and invalid[g][nxt - 1]:
                        out[g, c] = ord("N")
                    nxt += -1 if rev else 1
    return out


def _poly(m):
    """per column: do the ACGT cells show two different letters?"""
    return np.array([len(set(m[:, c].tolist()) & set(b"ACGT")) >= 2 for c in range(m.shape[1])], bool)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_restatement_equals_the_golden_xmfa_rows_and_the_pinned_counts(name):
    a, gs = load(name)
    N = len(gs)
    E = ref_of(a, gs)
    n_cols, n_core, n_poly = COUNTS[name]
    rows, siv, scol, roff = E.extract()
    with open(os.path.join(GOLDEN, name + ".xmfa")) as f:
        text = f.read()
    want = xmfa_matrix(text, N)
    assert rows.shape == want.shape == (N, n_cols) and np.array_equal(rows, want)
    assert np.array_equal(roff, a["col_off"]) and np.array_equal(a["col_off"][siv] + scol, np.arange(n_cols))
    blocks = parse_xmfa(text, N)
    assert len(blocks) == len(a["left"])
    for i, blk in enumerate(blocks):                                                # per interval, a genome with no entry is all '-'
        for g in range(N):
            got = rows[g, roff[i]:roff[i + 1]]
            assert (g in blk) == bool(a["left"][i, g])
            assert np.array_equal(got, blk[g][3]) if g in blk else np.all(got == ord("-"))
    # the scalar walk, and the counts from it and from the restatement
    w = _walk(a, gs)
    assert np.array_equal(w, rows)
    full = (1 << N) - 1
    core = (a["cols"] & full) == full
    poly = _poly(w)
    assert (int(core.sum()), int((core & poly).sum())) == (n_core, n_poly)
    c_rows, c_iv, c_col, c_off = E.extract(require=full)
    assert c_rows.shape == (N, n_core) and np.array_equal(c_rows, w[:, core]) and not np.any(c_rows == ord("-"))
    assert np.array_equal(a["col_off"][c_iv] + c_col, np.flatnonzero(core)) and c_off[-1] == n_core
    p_rows, p_iv, p_col, _ = E.extract(require=full, polymorphic=True)
    assert p_rows.shape == (N, n_poly) and np.array_equal(p_rows, w[:, core & poly])


def test_fixtures_exercise_the_complement_and_the_absent_rows():
    for name, n_rev_full in (("g3x5k_inv", 1), ("g4x3k_tree", 7)):
        a, gs = load(name)
        full = np.all(a["left"] != 0, axis=1)
        assert int(np.count_nonzero(full & np.any(a["reverse"] != 0, axis=1))) == n_rev_full
    a, gs = load("g4x3k_tree")
    k = np.count_nonzero(a["left"], axis=1)
    assert int(np.count_nonzero((k >= 2) & (k <= 3))) == 8


def test_projection_drop_empty_require_and_ranges():
    a, gs = load("g4x3k_tree")
    E, w = ref_of(a, gs), _walk(a, gs)
    cols, off = a["cols"], a["col_off"]
    # projection onto a permuted subset: the rows in that order, every column
    rows, siv, scol, roff = E.extract(keep=[3, 0])
    assert np.array_equal(rows, w[[3, 0]]) and len(siv) == len(cols)
    # drop_empty: the columns where neither kept genome has a residue leave
    rows, siv, scol, roff = E.extract(keep=[3, 0], drop_empty=True)
    m = (cols & 0b1001) != 0
    assert 0 < m.sum() < len(cols) and np.array_equal(rows, w[[3, 0]][:, m]) and np.array_equal(off[siv] + scol, np.flatnonzero(m))
    assert np.array_equal(roff, np.concatenate([[0], np.cumsum(m)])[off])
    # require not a subset of keep: genome 1 must be present, rows 2 and 0 are written
    rows, siv, scol, roff = E.extract(keep=[2, 0], require=0b0010)
    m = (cols & 2) != 0
    assert np.array_equal(rows, w[[2, 0]][:, m]) and np.any(rows == ord("-"))
    # polymorphic on a projection counts the kept rows only
    rows, _, _, _ = E.extract(keep=[1, 2], polymorphic=True)
    assert np.array_equal(rows, w[[1, 2]][:, _poly(w[[1, 2]])]) and rows.shape[1] > 0
    # overlapping and empty ranges: columns repeat, range_off has equal neighbours
    big = int(np.argmax(np.diff(off)))
    n = int(off[big + 1] - off[big])
    rg = ([big, 0, big, 1, big], [0, 0, n // 3, 2, n], [n // 2, 0, n - n // 3, 5, 0])
    rows, siv, scol, roff = E.extract(ranges=rg, require=0b0001)
    x = np.concatenate([off[i] + c + np.arange(l) for i, c, l in zip(*rg)])
    m = (cols[x] & 1) != 0
    assert np.array_equal(off[siv] + scol, x[m]) and np.array_equal(rows, w[:, x[m]])
    assert np.array_equal(roff, np.concatenate([[0], np.cumsum(m)])[np.concatenate([[0], np.cumsum(rg[2])])])
    assert roff[1] == roff[2] and roff[4] == roff[5] and len(set(x.tolist())) < len(x)
    r0 = E.extract(ranges=(np.zeros(0, np.int64),) * 3)
    assert r0[0].shape == (4, 0) and r0[3].tolist() == [0]


def test_ambiguous_bases_print_n_and_do_not_count_as_polymorphic():
    a, gs = load("g3x5k_inv")
    rng = np.random.default_rng(15)
    inv = [rng.random(len(g)) < 0.05 for g in gs]
    inv[1] = None
    E, w = ref_of(a, gs, inv), _walk(a, gs, inv)
    plain = _walk(a, gs)
    assert np.any(w[0] == ord("N")) and np.any(w[2] == ord("N")) and not np.any(w[1] == ord("N"))
    assert np.array_equal(w == ord("N"), (w != plain))
    rev_iv = np.flatnonzero(np.any(a["reverse"] != 0, axis=1))
    assert any(np.any(w[:, a["col_off"][i]:a["col_off"][i + 1]] == ord("N")) for i in rev_iv)        # on the reverse strand too
    rows, _, _, _ = E.extract()
    assert np.array_equal(rows, w)
    p_rows, p_iv, p_col, _ = E.extract(polymorphic=True)
    pw, pp = _poly(w), _poly(plain)
    assert np.array_equal(p_rows, w[:, pw]) and np.any(p_rows == ord("N"))                             # still written with its Ns
    assert np.any(pp & ~pw) and not np.any(pw & ~pp)                                                   # an N took the second letter away


def test_new_entry_points_are_exported():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
