"""An alignment scored against a correct one, the parts that need no GPU: the numpy restatement tests/score_ref.py against
accuracy.score_alignment_reference and against what src/scoreAlignment.cpp printed (tests/golden/reference_tools.json);
accuracy.truth_alignment against the XMFA file the tool read; the host entry mauve_score_totals_from; the header and the export list; the
mirror's bookkeeping in C++ under the address and undefined-behaviour sanitizers (tests/cpp/score_host_test.cpp)."""
import functools
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, accuracy, synth
from tests import score_ref as SR
from tests.test_accuracy import GOLDEN, SCORE_CASES, score_case, sha256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mauve_score_truth", "mauve_score_alignment", "mauve_score_totals_from")
COUNTS = ("tp", "tn", "fp", "fn")


@functools.lru_cache(maxsize=None)
def case(k):
    """case k of SCORE_CASES -> dict(genomes, origins, truth, calc, records, reference, golden); computed once, shared (with the GPU tests), never changed"""
    seed, n, length, div = SCORE_CASES[k]
    gs, org = synth.star_genomes(n, length, div, seed, inversions=0, track=True)
    _, _, r, org2 = score_case(*SCORE_CASES[k])
    assert all(np.array_equal(a, b) for a, b in zip(org, org2))
    truth = accuracy.truth_alignment(gs, org)
    with open(GOLDEN) as f:
        gold = json.load(f)["score_alignment"][k]
    assert tuple(gold["case"]) == SCORE_CASES[k]
    return dict(genomes=gs, origins=org, truth=truth, calc=r["aln"], n=n, records=SR.score_records(truth, r["aln"], n),
                reference=accuracy.score_alignment_reference(r["aln"], org), golden=gold)


def tool_ratios(gold):
    """the four ratios scoreAlignment printed: sensitivity, specificity, correct fraction, wrong fraction"""
    return [float(x) for x in re.findall(r"= ([0-9.e+-]+)$", gold["stdout"], re.M)][:4]


def check_ratios(t, gold, what):
    want = tool_ratios(gold)
    got = [t["sensitivity"], t["specificity"], (t["tp"] + t["tn"]) / t["total"], (t["fp"] + t["fn"]) / t["total"]]
    assert len(want) == 4
    for g, w in zip(got, want):
        assert abs(g - w) <= 6e-6 * max(1.0, abs(g)), (what, got, want)


def residues(aln, n):
    """residues of every genome in the alignment, by the columns"""
    cols = np.asarray(aln["cols"], np.uint32)
    return [int(np.count_nonzero(cols >> np.uint32(g) & np.uint32(1))) for g in range(n)]


def check_row_sums(rec, truth, n):
    have = residues(truth, n)
    for i in range(n):
        assert not rec[i, i].any() and not rec[i, :, 6:].any()
        for j in range(n):
            if i != j:
                assert rec[i, j, :6].sum() == have[i], (i, j, rec[i, j], have[i])


@pytest.mark.parametrize("k", range(len(SCORE_CASES)))
def test_restatement_equals_the_reference_rule_and_the_tool(k):
    c = case(k)
    rec = c["records"]
    assert rec.shape == (c["n"], c["n"], SR.WORDS) and rec.dtype == np.int64
    t = SR.totals(rec)
    for key in COUNTS:
        assert t[key] == c["reference"][key], (key, t, c["reference"])
    assert t["total"] == c["reference"]["total"]
    check_ratios(t, c["golden"], SCORE_CASES[k])
    slots = rec[..., :6].reshape(-1, 6).sum(axis=0)
    assert (slots > 0).all(), slots                                # no class is tested on zeros
    check_row_sums(rec, c["truth"], c["n"])


def test_issue_figures_of_the_four_genome_case():
    t = SR.totals(case(2)["records"])
    assert SCORE_CASES[2] == (5, 4, 4000, 0.15) and (t["tp"], t["tn"], t["fp"], t["fn"]) == (22723, 902, 353, 577)


def xmfa_of(aln, genomes, names):
    """the one-block XMFA text of a forward one-interval alignment, rebuilt from its arrays"""
    left, right, cols = np.asarray(aln["left"]), np.asarray(aln["right"]), np.asarray(aln["cols"], np.uint32)
    assert left.shape[0] == 1 and not np.asarray(aln["reverse"]).any() and aln["col_off"].tolist() == [0, len(cols)]
    out = ["#FormatVersion Mauve1\n"]
    for g in range(left.shape[1]):
        present = (cols >> np.uint32(g) & np.uint32(1)).astype(bool)
        assert left[0, g] == 1 and right[0, g] == len(genomes[g]) == np.count_nonzero(present)
        row = np.full(len(cols), ord("-"), np.uint8)
        row[present] = np.frombuffer(b"ACGT", np.uint8)[np.asarray(genomes[g])]
        text = row.tobytes().decode()
        out.append("> %d:1-%d + %s\n" % (g + 1, len(genomes[g]), names[g]))
        out.extend(text[p:p + 80] + "\n" for p in range(0, len(cols), 80))
    out.append("=\n")
    return "".join(out)


@pytest.mark.parametrize("k", range(len(SCORE_CASES)))
def test_truth_alignment_is_the_file_the_tool_read(k):
    c = case(k)
    names = ["g%d.fa" % g for g in range(c["n"])]
    text = xmfa_of(c["truth"], c["genomes"], names)
    assert sha256(text) == c["golden"]["truth_sha256"]
    assert text == accuracy.truth_xmfa(c["genomes"], c["origins"], names)
    t = c["truth"]
    assert t["left"].dtype == np.int64 and t["right"].dtype == np.int64 and t["reverse"].dtype == np.int8 and t["col_off"].dtype == np.int64 and t["cols"].dtype == np.uint32
    assert t["cols"].min() > 0


def test_truth_alignment_refuses_inversions():
    gs, org = synth.star_genomes(3, 6000, 0.08, 11, inversions=2, track=True)
    with pytest.raises(ValueError):
        accuracy.truth_alignment(gs, org)
    with pytest.raises(ValueError):
        accuracy.truth_xmfa(gs, org, ["a", "b", "c"])


@pytest.mark.parametrize("k", range(len(SCORE_CASES)))
def test_truth_against_itself_is_all_correct(k):
    c = case(k)
    for aln in (c["truth"], c["calc"]):
        rec = SR.score_records(aln, aln, c["n"])
        assert not rec[..., 1:5].any() and rec[..., 0].sum() > 0
        check_row_sums(rec, aln, c["n"])
    assert SR.score_records(c["truth"], c["truth"], c["n"])[..., 5].sum() > 0


def test_restatement_hand_case():
    """two genomes, T: columns AB AB A- -B AB (positions 1..4 / 1..4); C: genome 0's base 2 against genome 1's base 3, base 3 of genome 0 in an
    interval without genome 1, base 4 nowhere"""
    T = dict(left=[[1, 1]], right=[[4, 4]], reverse=[[0, 0]], col_off=[0, 5], cols=[3, 3, 1, 2, 3])
    # C's first interval: columns (0:1, 1:1) (1:2) (0:2, 1:3); its second: (0:3)
    Cc = dict(left=[[1, 1], [3, 0]], right=[[2, 3], [3, 0]], reverse=[[0, 0], [0, 0]], col_off=[0, 3, 4], cols=[3, 2, 3, 1])
    rec = SR.score_records(T, Cc, 2)
    # genome 0: base 1 -> T 1, C 1: tp; base 2 -> T 2, C 3: fp_base; base 3 -> T none, C: interval lacks genome 1: tn; base 4 -> T 4, C nowhere: fn_unaligned
    assert rec[0, 1].tolist() == [1, 1, 0, 1, 0, 1, 0, 0]
    # genome 1: base 1 -> tp; base 2 -> T 2 of genome 0, C a gap inside: fp_gap; base 3 -> T none, C base 2: fn_base; base 4 -> fn_unaligned
    assert rec[1, 0].tolist() == [1, 0, 1, 1, 1, 0, 0, 0]
    t = SR.totals(rec)
    assert (t["tp"], t["fp"], t["fn"], t["tn"], t["unaligned_fn"], t["total"]) == (1, 1, 2, 1, 1, 5)


def test_totals_from_equals_the_restatement():
    """mauve_score_totals_from through _lib: host code of the product library, no GPU"""
    for k in range(len(SCORE_CASES)):
        rec = case(k)["records"]
        got, want = _lib.score_totals(rec), SR.totals(rec)
        assert got == want and set(got) >= set(case(k)["reference"])
    rng = np.random.default_rng(17)
    for n in (1, 2, 7, 32):
        rec = rng.integers(0, 1 << 40, (n, n, _lib.SCORE_WORDS)).astype(np.int64)
        assert _lib.score_totals(rec) == SR.totals(rec)
    assert _lib.score_totals(np.zeros((3, 3, 8), np.int64))["total"] == 0
    for bad in (np.zeros((2, 3, 8), np.int64), np.zeros((2, 2, 6), np.int64), np.zeros(8, np.int64)):
        with pytest.raises(ValueError):
            _lib.score_totals(bad)


def test_new_entry_points_are_declared_and_exported():
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "mauve_hip.h")) as f:
        hdr = f.read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(r"^(int|void) %s\(" % name, hdr, re.M), name
    assert "#define MAUVE_SCORE_WORDS %d\n" % _lib.SCORE_WORDS in hdr and SR.WORDS == _lib.SCORE_WORDS
    assert "typedef struct { int64_t tp, tn, fp, fn, total, unaligned_fn; } mauve_score_totals;" in hdr
    assert [f[0] for f in _lib.ScoreTotals._fields_] == ["tp", "tn", "fp", "fn", "total", "unaligned_fn"]


def test_host_side_under_sanitizers():
    """tests/cpp/score_host_test.cpp with the library's host source of the totals: a stand-alone program, host C++ only (the sanitizer
    runtimes are linked into it, so it runs the same whatever the environment preloads)"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "score_host_test")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "score_host_test.cpp"), os.path.join(ROOT, "mauvealigner_amd", "csrc", "score_host.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
