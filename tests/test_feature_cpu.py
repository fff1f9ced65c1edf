"""CPU checks of the range map and the interval-overlap join: the library exports the new entry points, and the restatement
the GPU tests compare against (tests/feature_ref.py) is pinned -- on a hand case with every array written out, against the single-position
calls of the S14 restatement and the column bits of the committed fixtures, against the host walk of the mirror's
CompactGappedAlignment (tests/cpp/feature_map_test.cpp), and, for the join, against a per-base coverage count."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib
from tests import feature_cases as FC
from tests import feature_ref as FR
from tests.test_project_cpu import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("g3x5k_inv", "g4x3k_tree", "g5x3k_unique", "g4x6k_repeat")
NEW_SYMBOLS = ("mauve_map_ranges", "mauve_map_ranges_fetch", "mauve_range_overlaps")


def test_library_exports_the_new_entry_points():
    """the entry points include/mauve_hip.h declares for S21 are dynamic symbols of the built library and named in the loader's list"""
    L = _lib.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name in NEW_SYMBOLS:
        assert name in syms and name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "mauve_hip.h")) as f:
        hdr = f.read()
    assert "mauve_range_map_sizes" in hdr and all(name + "(" in hdr for name in NEW_SYMBOLS)


def test_hand_case_every_array_written_out():
    m = FR.map_ranges(FC.ref_of(FC.HAND), *FC.HAND_QUERIES)
    for k in FR.ARRAYS:
        assert m[k].dtype == np.int64 and m[k].tolist() == FC.HAND_WANT[k], k
    t = FR.map_ranges(FC.ref_of(FC.TIES), *FC.TIES_QUERIES)
    assert t["piece_iv"][t["best"]].tolist() == FC.TIES_BEST_IV
    e = FR.map_ranges(FC.ref_of(FC.HAND), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert e["piece_off"].tolist() == [0] and e["n_res"].shape == (0, 3)


def _independent_checks(a, q, lens=None):
    R = FC.ref_of(a)
    seq, lo, hi = (np.asarray(v, np.int64) for v in q)
    m = FR.map_ranges(R, *q)
    P, N = m["n_res"].shape
    s, iv, col, last = seq[m["piece_query"]], m["piece_iv"], m["piece_col"], m["piece_col"] + m["piece_len"] - 1
    # the columns of the clipped ends by S14's rule 2
    i1, c1 = R.seqpos_to_column(s, m["clip_lo"])
    i2, c2 = R.seqpos_to_column(s, m["clip_hi"])
    assert np.array_equal(i1, iv) and np.array_equal(i2, iv)
    assert np.array_equal(col, np.minimum(c1, c2)) and np.array_equal(last, np.maximum(c1, c2))
    assert np.array_equal(c1 > c2, R.rev[iv, s] & (m["clip_lo"] < m["clip_hi"]))    # they swap on a reverse row
    # the extents by S14's rule 1: the first residue at or behind the first column, the last one at or before the last column
    first, _ = R.column_positions(iv, col, nearest=False)
    x0, x1 = R.col_off[iv] + col, R.col_off[iv] + last
    n_res = np.zeros((P, N), np.int64)
    for p in range(P):
        n_res[p] = R.bits[x0[p]:x1[p] + 1].sum(axis=0) * (R.left[iv[p]] != 0)        # the popcount of the fixture's column bits
    assert np.array_equal(m["n_res"], n_res)
    at_last, _ = R.column_positions(iv, last, nearest=True)                           # the residue in the last column, else the one before it
    in_front = R.cum[x0] - R.cum[R.col_off[iv]]                                       # residues of the interval in front of the range
    for p in range(P):
        for g in range(N):
            if n_res[p, g] == 0:
                assert m["ext_left"][p, g] == 0 and m["ext_right"][p, g] == 0
                continue
            # the range's first residue of g: at the first column if g has one there, else the residue that follows the one in front of it
            start = first[p, g] if first[p, g] else int(R._signed(iv[p:p + 1], in_front[p:p + 1])[0, g])
            end = at_last[p, g]
            lo_g, hi_g = sorted((abs(int(start)), abs(int(end))))
            sign = -1 if R.rev[iv[p], g] else 1
            assert (m["ext_left"][p, g], m["ext_right"][p, g]) == (sign * lo_g, sign * hi_g), (p, g)
            assert hi_g - lo_g + 1 == n_res[p, g]
    # the query's own row is exactly the clip
    k = np.arange(P)
    assert np.array_equal(m["n_res"][k, s], m["clip_hi"] - m["clip_lo"] + 1)
    assert np.array_equal(np.abs(m["ext_left"][k, s]), m["clip_lo"]) and np.array_equal(np.abs(m["ext_right"][k, s]), m["clip_hi"])
    # per query the clipped lengths sum to the covered bases of the range
    for g in np.unique(seq):
        top = int(R.right[:, g].max()) + 2
        cov = np.concatenate([[0], np.cumsum(R.covered(g, top))])
        sel = seq == g
        assert np.array_equal(m["covered"][sel], cov[np.minimum(hi[sel], top)] - cov[np.minimum(lo[sel] - 1, top)])
    size = m["clip_hi"] - m["clip_lo"] + 1
    for qi in range(len(seq)):
        a0, a1 = m["piece_off"][qi], m["piece_off"][qi + 1]
        assert np.all(np.diff(m["clip_lo"][a0:a1]) > 0)                              # ascending in the genome
        if a1 > a0:
            b = m["best"][qi]
            assert a0 <= b < a1 and all((size[b], iv[b]) >= (size[p], iv[p]) for p in range(a0, a1))
        else:
            assert m["best"][qi] == -1
    return m


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_against_the_coordinate_rules_on_the_fixtures(name):
    a = load(name)
    _independent_checks(a, FC.random_queries(a, 11))


def test_restatement_against_the_coordinate_rules_on_the_built_alignment():
    a, lens = FC.built(5, 3)
    q = FC.built_queries(a, lens)
    m = _independent_checks(a, tuple(v[::3] for v in q))
    assert np.any(m["n_res"] == 0) and np.any(np.diff(m["piece_off"]) > 3)


def _build_feature_map_test(td):
    exe = os.path.join(td, "feature_map_test")
    lib = os.path.join(ROOT, "mauvealigner_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "feature_map_test.cpp"), "-o", exe,
                           "-L" + lib, "-lmauve_hip", "-Wl,-rpath," + lib])
    return exe


def parse_pieces(stdout, N):
    """the `piece` lines of tests/cpp/feature_map_test.cpp -> the piece arrays of a range map"""
    rows, per = [], []
    for line in stdout.splitlines():
        if line.startswith("piece "):
            head, tail = line[6:].split("|")
            rows.append([int(x) for x in head.split()])
            per.append([[int(x) for x in t.split(":")] for t in tail.split()])
    rows, per = np.array(rows, np.int64).reshape(-1, 6), np.array(per, np.int64).reshape(-1, N, 3)
    out = {k: rows[:, j] for j, k in enumerate(FR.PER_PIECE[:2] + ("clip_lo", "clip_hi", "piece_col", "piece_len"))}
    out.update(n_res=per[:, :, 0], ext_left=per[:, :, 1], ext_right=per[:, :, 2])
    return out


def parse_rows(stdout, N):
    """the `row` lines -> dict(piece_iv, rearranged, identity, ortholog, overlap)"""
    head, per = [], []
    for line in stdout.splitlines():
        if line.startswith("row "):
            h, tail = line[4:].split("|")
            h = h.split()
            head.append((int(h[1]), int(h[2]), float.fromhex(h[3])))
            per.append([[int(x) for x in t.split(":")] for t in tail.split()])
    per = np.array(per, np.int64).reshape(-1, N, 2)
    return dict(piece_iv=np.array([h[0] for h in head], np.int64), rearranged=np.array([h[1] for h in head], np.int8),
                identity=np.array([h[2] for h in head], np.float64), ortholog=per[:, :, 0], overlap=per[:, :, 1])


def test_mirror_host_walk_gives_the_restatements_pieces():
    """tests/cpp/feature_map_test.cpp, host C++ only: SeqPosToColumn, copyRange, LeftEnd / RightEnd / Length of the mirror's
    CompactGappedAlignment on the golden XMFA of g4x3k_tree give the restatement's pieces"""
    a = load("g4x3k_tree")
    N = a["left"].shape[1]
    q = tuple(v[::4] for v in FC.random_queries(a, 13))
    want = FR.map_ranges(FC.ref_of(a), *q)
    with tempfile.TemporaryDirectory() as td:
        exe = _build_feature_map_test(td)
        path = os.path.join(td, "ranges.txt")
        np.savetxt(path, np.stack([np.asarray(v, np.int64) for v in q], axis=1), fmt="%d")
        r = subprocess.run([exe, os.path.join(GOLDEN, "g4x3k_tree.xmfa"), path], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    got = parse_pieces(r.stdout, N)
    assert len(want["piece_iv"]) > 100
    assert FR.same(got, want, FR.PER_PIECE + FR.PER_ROW) == []


def _per_base_join(tab, queries):
    """the join written another way: a coverage row per table entry over the bases of the query"""
    ts, tl, th = (np.asarray(v, np.int64) for v in tab)
    out = []
    for s, lo, hi in zip(*queries):
        a, b = sorted((abs(int(lo)), abs(int(hi))))
        if b == 0 or b - a > 20000:
            out.append(None if b else (0, -1, 0))
            continue
        base = np.arange(a, b + 1, dtype=np.int64)[:, None]
        shared = ((base >= tl[None, :]) & (base <= th[None, :]) & (ts[None, :] == s)).sum(axis=0)
        top = int(shared.max()) if len(ts) else 0
        out.append((int(np.count_nonzero(shared)), int(np.flatnonzero(shared == top)[-1]) if top else -1, top))
    return out


def test_join_restatement_against_a_per_base_count():
    for k, g in zip(("n_hit", "best", "overlap"), FR.range_overlaps(FC.JOIN_TAB, FC.JOIN_QUERIES)):
        assert g.tolist() == FC.JOIN_WANT[k], k
    for k, g in zip(("n_hit", "best", "overlap"), FR.range_overlaps(FC.JOIN_TIES_TAB, FC.JOIN_TIES_QUERIES)):
        assert g.tolist() == FC.JOIN_TIES_WANT[k], k
    cases = [(FC.JOIN_TAB, FC.JOIN_QUERIES), (FC.JOIN_TIES_TAB, FC.JOIN_TIES_QUERIES)]
    for m in (1, 63, 64, 65, 1025):
        tab = FC.shuffled_table(m, 100 + m)
        cases.append((tab, FC.shuffled_queries(tab, 120, m)))
    checked = 0
    for tab, q in cases:
        got = FR.range_overlaps(tab, q)
        for k, w in enumerate(_per_base_join(tab, q)):
            if w is not None:                                                        # (a range of more than 20000 bases is left to the planted cases)
                assert (got[0][k], got[1][k], got[2][k]) == w, (k, w)
                checked += 1
    assert checked > 600
