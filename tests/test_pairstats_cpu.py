"""CPU-side checks of the pairwise column statistics: the numpy restatement of tests/pairstats_ref.py, which is the expected
value of the GPU tests, against a scalar per-pair state machine written out here, against hand-counted cases and pinned counts; the
invariants of the record; the two host helpers of the built library (no device needed) against numpy; the new entry points in the
export list; and the helpers against mems::computeSPScore and mems::IdentityMatrix in C++ (tests/cpp/pairstats_host_test.cpp)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, synth
from tests import pairstats_ref as PR
from tests.extract_ref import ExtractRef
from tests.test_extract_cpu import COUNTS, load, ref_of
from tests.test_gpu_extract import HAND, HAND_GENOMES, _codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mauve_pair_stats", "mauve_pair_stats_identity", "mauve_pair_stats_sp_score")


def scalar_record(x, y):
    """the definition: one pass over the cells x, y (letters as bytes) of one range, the run state of computeSPScore"""
    s = [0] * PR.WORDS
    code = {ord(ch): k for k, ch in enumerate("ACGTN")}
    gap = ord("-")
    open_side = 0                                       # 1: an only_a run is open, 2: an only_b run
    for cx, cy in zip(x.tolist(), y.tolist()):
        if cx == gap and cy == gap:
            s[29] += 1                                  # neither scores nor interrupts
        elif cx != gap and cy != gap:
            s[5 * code[cx] + code[cy]] += 1
            open_side = 0
        else:
            side = 1 if cy == gap else 2
            s[24 + side] += 1
            if open_side != side:
                s[26 + side] += 1
            open_side = side
    return s


def scalar_stats(E, pairs, ranges):
    """per-range records [R, P, 32] by the scalar rule, range after range"""
    rows, _, _, roff = E.extract(ranges=ranges)
    out = np.zeros((len(roff) - 1, len(pairs[0]), PR.WORDS), np.int64)
    for r in range(len(roff) - 1):
        for p, (a, b) in enumerate(zip(*pairs)):
            out[r, p] = scalar_record(rows[a, roff[r]:roff[r + 1]], rows[b, roff[r]:roff[r + 1]])
    return out


def some_ranges(a, rng, n=40):
    """random ranges with empty and overlapping ones, as test_extract_golden_fixtures draws them"""
    lens = np.diff(a["col_off"])
    r_iv = rng.integers(0, len(lens), n)
    r_col = (rng.random(n) * (lens[r_iv] + 1)).astype(np.int64)
    r_len = (rng.random(n) * (lens[r_iv] - r_col + 1)).astype(np.int64)
    r_len[::7] = 0
    return r_iv, r_col, r_len


def check_invariants(per, lens, pairs):
    """slots 0..26 and 29 sum to the range's length; 30, 31 are zero; runs <= columns, and a run needs a column; the pair (b, a) is the
    transposition of (a, b)"""
    assert np.array_equal(per[..., :27].sum(axis=-1) + per[..., 29], np.broadcast_to(np.asarray(lens)[:, None], per.shape[:2]))
    assert not np.any(per[..., 30:]) and not np.any(per < 0)
    for only, runs in ((25, 27), (26, 28)):
        assert np.all(per[..., runs] <= per[..., only]) and np.array_equal(per[..., runs] > 0, per[..., only] > 0)
    where = {(int(a), int(b)): p for p, (a, b) in enumerate(zip(*pairs))}
    n_mirrored = 0
    for (a, b), p in where.items():
        q = where.get((b, a))
        if q is None:
            continue
        n_mirrored += 1
        assert np.array_equal(per[:, q, :25].reshape(-1, 5, 5), per[:, p, :25].reshape(-1, 5, 5).transpose(0, 2, 1))
        assert np.array_equal(per[:, q, [25, 26, 27, 28, 29]], per[:, p, [26, 25, 28, 27, 29]])
    return n_mirrored


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_restatement_equals_the_scalar_state_machine(name):
    a, gs = load(name)
    N = len(gs)
    E = ref_of(a, gs)
    ordered = tuple(np.array(v, np.int32) for v in zip(*[(x, y) for x in range(N) for y in range(N) if x != y]))
    rng = np.random.default_rng(len(name))
    for ranges in (None, some_ranges(a, rng)):
        per = PR.pair_stats(E, ordered, ranges, per_range=True)
        assert np.array_equal(per, scalar_stats(E, ordered, ranges))
        lens = np.diff(a["col_off"]) if ranges is None else ranges[2]
        assert check_invariants(per, lens, ordered) == N * (N - 1)
        assert np.array_equal(PR.pair_stats(E, ordered, ranges), per.sum(axis=0))             # the totals are the sum of the per-range records
    # the default pair list is the upper triangle in row-major order, and the whole alignment is every interval once
    tot = PR.pair_stats(E)
    up = PR.all_pairs(N)
    assert list(zip(*up)) == [(x, y) for x in range(N) for y in range(x + 1, N)]
    assert np.array_equal(tot, PR.pair_stats(E, up)) and tot.shape == (N * (N - 1) // 2, PR.WORDS)
    assert np.all(tot[:, :27].sum(axis=1) + tot[:, 29] == COUNTS[name][0])


def test_hand_case():
    """test_extract_hand_case's alignment: rows ACGTACGTACGTACGTACGT / CCCCCGGGGG-----TTTTT / TTACGTACGTAAAACCCGGT"""
    E = ExtractRef(HAND["left"], HAND["right"], HAND["reverse"], HAND["col_off"], HAND["cols"], [_codes(s) for s in HAND_GENOMES])
    st = PR.pair_stats(E, ([0, 1, 1], [1, 2, 0]))
    s01, s12, s10 = st
    assert s01[:25].sum() == 15 and s01[PR.DIAG].sum() == 4 and s01[25:30].tolist() == [5, 0, 1, 0, 0]
    assert s12[:25].sum() == 15 and s12[PR.DIAG].sum() == 3 and s12[25:30].tolist() == [0, 5, 0, 1, 0]
    assert np.array_equal(s10[:25].reshape(5, 5), s01[:25].reshape(5, 5).T) and s10[25:30].tolist() == [0, 5, 0, 1, 0]
    # A against C C C C C, ...: the letter table of (0, 1), rows = the letter of genome 0
    assert s01[:25].reshape(5, 5)[:4, :4].tolist() == [[0, 2, 1, 1], [0, 1, 2, 1], [0, 1, 1, 1], [0, 1, 1, 2]]
    # a window that cuts the gap run of genome 1 (columns 10..14) in two ranges: each range opens a run of its own
    per = PR.pair_stats(E, ([0], [1]), ([0, 0], [8, 12], [4, 6]), per_range=True)
    assert per[0, 0, 25:30].tolist() == [2, 0, 1, 0, 0] and per[1, 0, 25:30].tolist() == [3, 0, 1, 0, 0]
    assert per[0, 0, :25].sum() == 2 and per[1, 0, :25].sum() == 3


def test_pinned_counts_of_the_first_pair():
    want = {"g2x2k": (1991, 1915, [10, 15, 5, 7, 0]), "g4x3k_tree": (3065, 2960, [273, 285, 18, 18, 976])}
    for name, (both, equal, rest) in want.items():
        a, gs = load(name)
        s = PR.pair_stats(ref_of(a, gs))[0]
        assert (int(s[:25].sum()), int(s[PR.DIAG].sum()), s[25:30].tolist()) == (both, equal, rest), name


def test_ambiguous_bases_fill_the_fifth_letter():
    a, gs = load("g3x5k_inv")
    rng = np.random.default_rng(16)
    inv = [rng.random(len(g)) < 0.05 for g in gs]
    inv[1] = None
    E = ref_of(a, gs, inv)
    pairs = (np.array([0, 0, 1]), np.array([1, 2, 2]))
    per = PR.pair_stats(E, pairs, per_range=True)
    assert np.array_equal(per, scalar_stats(E, pairs, None))
    t = per.sum(axis=0)[:, :25].reshape(3, 5, 5)
    assert t[0, 4, :4].sum() > 0 and t[0, :, 4].sum() == 0                 # genome 1 has no ambiguous base
    assert t[1, 4, 4] > 0 and t[1, 4, :4].sum() > 0 and t[1, :4, 4].sum() > 0


def _scoring(matrix, go, ge):
    sc = _lib.Scoring()
    for x in range(4):
        for y in range(4):
            sc.matrix[x][y] = int(matrix[x][y])
    sc.gap_open, sc.gap_extend = go, ge
    return sc


def test_host_helpers_of_the_library():
    """mauve_pair_stats_identity / mauve_pair_stats_sp_score on records of the restatement: the default scoring, an asymmetric matrix,
    the zero denominator, N scoring as A"""
    a, gs = load("g4x3k_tree")
    rng = np.random.default_rng(3)
    inv = [rng.random(len(g)) < 0.03 for g in gs]
    E = ref_of(a, gs, inv)
    per = PR.pair_stats(E, per_range=True)
    assert np.any(per[..., :25].sum(axis=-1) == 0) and np.any(per[..., 24] > 0)                 # pairs that never meet in an interval; N against N
    d = _lib.default_scoring()
    skew = [[5, -1, -2, -3], [-4, 6, -5, -6], [-7, -8, 7, -9], [-10, -11, -12, 8]]
    for st in (per, per.sum(axis=0), per[0, 0], np.zeros((0, PR.WORDS), np.int64)):
        ident = _lib.pair_stats_identity(st)
        assert ident.shape == st.shape[:-1] and ident.dtype == np.float64 and np.array_equal(ident, PR.identity(st))
        for sc, m, go, ge in ((None, [list(r) for r in d.matrix], d.gap_open, d.gap_extend), (_scoring(skew, -17, -3), skew, -17, -3)):
            score = _lib.pair_stats_sp_score(st, sc)
            assert score.shape == st.shape[:-1] and score.dtype == np.int64 and np.array_equal(score, PR.sp_score(st, m, go, ge))
    assert (d.gap_open, d.gap_extend) == (-400, -30)
    zero = np.zeros(PR.WORDS, np.int64)
    zero[25], zero[27], zero[29] = 7, 2, 11                                                      # no column with two residues
    assert _lib.pair_stats_identity(zero) == 0.0 and _lib.pair_stats_sp_score(zero) == 2 * -400 + 5 * -30
    n = np.zeros(PR.WORDS, np.int64)
    n[5 * 4 + 1], n[5 * 2 + 4], n[24] = 3, 5, 2                                                  # N/C, G/N, N/N score as A/C, G/A, A/A
    assert _lib.pair_stats_sp_score(n, _scoring(skew, -17, -3)) == 3 * skew[0][1] + 5 * skew[2][0] + 2 * skew[0][0]
    assert _lib.pair_stats_identity(n) == 2 / 10                                                 # N against N counts as equal
    with pytest.raises(ValueError):
        _lib.pair_stats_identity(np.zeros((2, 31), np.int64))


def test_new_entry_points_are_exported():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "mauve_hip.h")) as f:
        assert "#define MAUVE_PAIR_STATS_WORDS %d\n" % _lib.PAIR_STATS_WORDS in f.read()
    assert PR.WORDS == _lib.PAIR_STATS_WORDS


def test_host_helpers_equal_compute_sp_score_and_identity_matrix():
    """tests/cpp/pairstats_host_test.cpp on the golden XMFAs: host C++ only"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "pairstats_host_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pairstats_host_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        for name in ("g2x2k", "g3x5k_inv", "g4x3k_tree"):
            a, gs = load(name)
            mfa = os.path.join(td, name + ".mfa")
            with open(mfa, "w") as f:
                for g, s in enumerate(gs):
                    f.write(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()))
            r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", name + ".xmfa"), mfa], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
