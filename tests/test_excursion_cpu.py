"""CPU-side checks of the excursions of the column scores: the restatement of tests/excursion_ref.py, which is the
expected value of the GPU tests, against the worked example of S18, a hand case, pinned fixture totals and what the reference's own
program printed (src/evd.cpp built on the mirror; stored in tests/golden/reference_evd.json, and built and run again where the reference
tree is present); the four-rule walk against the max-form; the host helper of the built library against numpy; the new entry points in
the export list; computeMatchScores + computeGapScores of the mirror against its computeSPScore (tests/cpp/excursion_host_test.cpp)."""
import hashlib
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, synth
from tests import excursion_ref as XR
from tests.extract_ref import ExtractRef
from tests.test_compat_headers import REFERENCE
from tests.test_extract_cpu import COUNTS, load, ref_of
from tests.test_gpu_extract import HAND, HAND_GENOMES, _codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_EVD = os.path.join(ROOT, "tests", "golden", "reference_evd.json")
NEW = ("mauve_excursions_pairs", "mauve_excursions_core", "mauve_excursions_fetch", "mauve_excursion_thresholds")
# 2 on the diagonal, -1 off it; a gap column costs 3 where it opens a run and 1 where it extends one
SIMPLE = ([[2 if x == y else -1 for y in range(4)] for x in range(4)], -3, -1)
# the worked example of S18: mismatch, mismatch, match, mismatch, match
EXAMPLE = dict(left=np.array([[1, 1]]), right=np.array([[5, 5]]), reverse=np.zeros((1, 2), np.int8), col_off=np.array([0, 5]), cols=np.full(5, 3, np.uint32))
EXAMPLE_GENOMES = [_codes("AAAAA" + "GG"), _codes("CCACA" + "GG")]
# fixture: (pair excursions, core excursions of all genomes, largest height, pair streams not at 0 at their end, exact returns to zero)
TOTALS = {"g2x2k": (76, 69, 553, 0, 0), "g3x5k_inv": (436, 141, 610, 18, 2), "g4x3k_tree": (838, 179, 11950, 167, 2),
          "g4x6k_repeat": (1828, 399, 880, 0, 7), "g5x3k_unique": (1057, 3, 949, 4, 0)}


def scoring_of(matrix, gap_open, gap_extend):
    sc = _lib.Scoring()
    for x in range(4):
        for y in range(4):
            sc.matrix[x][y] = int(matrix[x][y])
    sc.gap_open, sc.gap_extend = int(gap_open), int(gap_extend)
    return sc


def default_scoring():
    d = _lib.default_scoring()
    return [list(r) for r in d.matrix], d.gap_open, d.gap_extend


def test_worked_example():
    E = ExtractRef(EXAMPLE["left"], EXAMPLE["right"], EXAMPLE["reverse"], EXAMPLE["col_off"], EXAMPLE["cols"], EXAMPLE_GENOMES)
    for walker in (XR.walk_rules, XR.walk):
        assert XR.walk_rules([1, 1, -2, 1, -2], range(5))[0].tolist() == [2]
        for r in (XR.excursions_pairs(E, *SIMPLE, walker=walker), XR.excursions_core(E, SIMPLE[0], walker=walker)):
            assert (r.height.tolist(), r.end_col.tolist(), r.stream_off.tolist(), r.tail.tolist()) == ([2], [4], [0, 1], [[0, 0]])
        r = XR.excursions_pairs(E, *SIMPLE, ranges=([0], [0], [4]), walker=walker)                 # cut in front of the last match
        assert (r.height.tolist(), r.stream_off.tolist(), r.tail.tolist()) == ([], [0, 0], [[1, 2]])
    # a restatement that ended an excursion at zero would report two records here
    ended_at_zero, x, h = [], 0, 0
    for v in [1, 1, -2, 1, -2]:
        x = max(0, x + v)
        h = max(h, x)
        if x == 0 and h:
            ended_at_zero.append(h)
            h = 0
    assert ended_at_zero == [2, 1]


def test_hand_case_with_a_gap_run_cut_by_a_range_boundary():
    """test_extract_hand_case's alignment: rows ACGTACGTACGTACGTACGT / CCCCCGGGGG-----TTTTT / TTACGTACGTAAAACCCGGT"""
    E = ExtractRef(HAND["left"], HAND["right"], HAND["reverse"], HAND["col_off"], HAND["cols"], [_codes(s) for s in HAND_GENOMES])
    # pair (0, 1): A/C C/C G/C T/C A/C | C/G G/G T/G A/G C/G | five columns of genome 0 alone | T/T A/T C/T G/T T/T
    v = [1, -2, 1, 1, 1, 1, -2, 1, 1, 1, 3, 1, 1, 1, 1, -2, 1, 1, 1, -2]
    occ, got = XR.pair_values(*[XR.letter_codes(E.extract()[0])[g] for g in (0, 1)], *SIMPLE)
    assert occ.tolist() == list(range(20)) and got.tolist() == v
    # x: 1, then 1 - 2 < 0: the record (1, column 1); from column 2 on 1 2 3 4 2 3 4 5 8 9 10 11 12 10 11 12 13 11
    r = XR.excursions_pairs(E, *SIMPLE, pairs=([0], [1]))
    assert (r.height.tolist(), r.end_col.tolist(), r.tail.tolist()) == ([1], [1], [[11, 13]])
    # the run of columns 10..14 whole, then cut at column 12: each range opens a run of its own
    r = XR.excursions_pairs(E, *SIMPLE, pairs=([0], [1]), ranges=([0, 0, 0], [10, 10, 12], [5, 2, 3]))
    assert r.tail.tolist() == [[7, 7], [4, 4], [5, 5]]
    # core of all three genomes: the five columns genome 1 lacks are no columns of the stream
    c = XR.excursions_core(E, SIMPLE[0])
    occ, _ = XR.core_values(XR.letter_codes(E.extract()[0]), [0, 1, 2], SIMPLE[0])
    assert occ.tolist() == list(range(10)) + list(range(15, 20)) and len(c.stream_off) == 2
    assert np.array_equal(XR.excursions_pairs(E, *SIMPLE, walker=XR.walk_rules).tail, XR.excursions_pairs(E, *SIMPLE).tail)


def test_max_form_equals_the_four_rules():
    """random value streams with exact returns to zero, empty streams, streams that start low"""
    rng = np.random.default_rng(18)
    returns = 0
    for trial in range(300):
        n = int(rng.integers(0, 400))
        v = rng.choice([-3, -2, -1, 0, 1, 2, 5], n, p=[.1, .25, .15, .1, .25, .1, .05]).astype(np.int64)
        cols = np.cumsum(rng.integers(1, 4, n))
        a, b = XR.walk_rules(v, cols), XR.walk(v, cols)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tuple(a[2]) == tuple(b[2]), trial
        x = 0
        for t in v.tolist():
            returns += x > 0 and x + t == 0
            x = max(0, x + t)
    assert returns > 100


def count_returns(E, matrix, gap_open, gap_extend):
    """exact returns to zero of the pair streams: x > 0 in front of a column, 0 behind it, x + v == 0"""
    codes = XR.letter_codes(E.extract()[0])
    n = 0
    for i in range(E.n_iv):
        part = codes[:, E.col_off[i]:E.col_off[i + 1]]
        for a, b in zip(*XR.all_pairs(E.N)):
            _, v = XR.pair_values(part[a], part[b], matrix, gap_open, gap_extend)
            x = 0
            for t in v.tolist():
                n += x > 0 and x + t == 0
                x = max(0, x + t)
    return n


@pytest.mark.parametrize("name", sorted(TOTALS))
def test_fixture_totals(name):
    """all pairs, whole intervals, default scoring: the pinned totals, by the four rules and by the max-form"""
    a, gs = load(name)
    E = ref_of(a, gs)
    m, go, ge = default_scoring()
    for walker in (XR.walk_rules, XR.walk):
        p = XR.excursions_pairs(E, m, go, ge, walker=walker)
        c = XR.excursions_core(E, m, walker=walker)
        got = (len(p.height), len(c.height), int(max(p.height.max(initial=0), c.height.max(initial=0))), int(np.count_nonzero(p.tail[:, 0])))
        assert got == TOTALS[name][:4], got
        assert np.array_equal(p.stream_off[1:] - p.stream_off[:-1] >= 0, np.ones(len(p.tail), bool)) and p.stream_off[-1] == len(p.height)
        assert np.all(p.tail[:, 1] >= p.tail[:, 0]) and np.all(p.tail >= 0) and np.all(p.height > 0)
    assert count_returns(E, m, go, ge) == TOTALS[name][4]


def test_host_helper_of_the_library():
    """mauve_excursion_thresholds against numpy and against the restatement, at n = 0, 1, 19, 20, 10001"""
    rng = np.random.default_rng(4)
    for n in (0, 1, 19, 20, 10001):
        h = rng.integers(1, 50000, n).astype(np.int64)
        thr, above = _lib.excursion_thresholds(h)
        assert thr.dtype == np.int64 and thr.shape == (4,) and above.shape == (4,)
        s = np.sort(h)
        want_t, want_a = [], []
        for f in (.95, .99, .999, .9999):
            idx = min(int(n * f), n - 1) if n else 0
            want_t.append(int(s[idx]) if n else 0)
            want_a.append(n - idx if n else 0)
        assert thr.tolist() == want_t and above.tolist() == want_a, n
        assert (thr.tolist(), above.tolist()) == XR.thresholds(h)
    assert _lib.excursion_thresholds([7, 3, 5])[0].tolist() == [7, 7, 7, 7]


def test_new_entry_points_are_exported():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "mauve_hip.h")) as f:
        assert "#define MAUVE_EXCURSION_CHUNK %d\n" % _lib.EXCURSION_CHUNK in f.read()


def test_match_and_gap_scores_equal_compute_sp_score():
    """tests/cpp/excursion_host_test.cpp on the golden XMFAs: host C++ only"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "excursion_host_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "excursion_host_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        for name in sorted(TOTALS):
            a, gs = load(name)
            mfa = os.path.join(td, name + ".mfa")
            with open(mfa, "w") as f:
                f.write(evd_inputs(name)[1])
            r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", name + ".xmfa"), mfa], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
            assert "excursions %d\n" % TOTALS[name][0] in r.stdout                # the tool's loop over those scores, written out in the test


# ---- the reference's own program: src/evd.cpp, run in a directory that holds alignjob.0/evolved.dat and alignjob.0/evolved_seqs.fas ----
def evd_inputs(name):
    """-> (the committed XMFA of the fixture, its genomes as a multi-FastA, the digest of the two)"""
    with open(os.path.join(ROOT, "tests", "golden", name + ".xmfa")) as f:
        xmfa = f.read()
    _, gs = load(name)
    fas = "".join(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()) for g, s in enumerate(gs))
    return xmfa, fas, hashlib.sha256((xmfa + "\0" + fas).encode()).hexdigest()


def run_evd(exe, name, td):
    """the program's standard output on the fixture"""
    xmfa, fas, _ = evd_inputs(name)
    job = os.path.join(td, name, "alignjob.0")
    os.makedirs(job)
    with open(os.path.join(job, "evolved.dat"), "w") as f:
        f.write(xmfa)
    with open(os.path.join(job, "evolved_seqs.fas"), "w") as f:
        f.write(fas)
    return subprocess.run([exe, "1"], capture_output=True, text=True, check=True, cwd=os.path.join(td, name)).stdout


def build_evd(src_dir, td):
    exe = os.path.join(td, "evd")
    lib = os.path.join(ROOT, "mauvealigner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(src_dir, "evd.cpp"), "-o", exe,
                           "-L" + lib, "-lmauve_hip", "-Wl,-rpath," + lib])
    return exe


def parse_evd(stdout):
    """-> (excursions, the four thresholds, the four counts above them)"""
    total = int(re.search(r"Total number of excursions: (-?\d+)", stdout).group(1))
    thr = [int(t) for t in re.findall(r"% score threshold: (-?\d+)", stdout)]
    above = [int(t) for t in re.findall(r"Number excursions above [\d.]+%: (-?\d+)", stdout)]
    assert len(thr) == 4 and len(above) == 4
    return total, thr, above


def restated_evd(name):
    a, gs = load(name)
    p = XR.excursions_pairs(ref_of(a, gs), *default_scoring())
    thr, above = _lib.excursion_thresholds(p.height)
    assert (thr.tolist(), above.tolist()) == XR.thresholds(p.height)
    return len(p.height), thr.tolist(), above.tolist()


@pytest.mark.parametrize("name", sorted(TOTALS))
def test_restatement_equals_what_evd_printed(name):
    """the stored output of src/evd.cpp on the fixture (made on the digest of its input) against the restatement and the host helper"""
    with open(GOLDEN_EVD) as f:
        ref = json.load(f)
    digest = evd_inputs(name)[2]
    assert digest in ref, "the input differs from the one the stored output was made on"
    assert parse_evd(ref[digest]["stdout"]) == restated_evd(name)
    assert ref[digest]["fixture"] == name and "Total number of simulations: 1\n" in ref[digest]["stdout"]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present")
def test_reference_evd_compiles_unmodified_and_runs_on_the_mirror():
    """src/evd.cpp, where it lies, against -I include: it needs INVALID_SCORE, computeMatchScores, computeGapScores and the scoring scheme
    from libMems/Islands.h.  Built and run on every fixture, it prints what the stored output holds and what the restatement gives"""
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(REFERENCE, "evd.cpp")])
    with open(GOLDEN_EVD) as f:
        ref = json.load(f)
    with tempfile.TemporaryDirectory() as td:
        exe = build_evd(REFERENCE, td)
        for name in sorted(TOTALS):
            out = run_evd(exe, name, td)
            assert out == ref[evd_inputs(name)[2]]["stdout"], name
            assert parse_evd(out) == restated_evd(name), name
