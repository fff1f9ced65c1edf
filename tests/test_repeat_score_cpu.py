"""A repeat map scored against a correct repeat alignment, the parts that need no GPU: the plain-Python restatement
tests/repeat_score_ref.py against the hand figures of tests/repeat_score_cases.py; the generator repeat_accuracy.planted_repeats and the
condition that the repeat map's own restatement finds every planted pair of undiverged copies; the host entry mauve_repeat_score_ppv; the
header and the export list; the mirror's bookkeeping in C++ under the address and undefined-behaviour sanitizers
(tests/cpp/repeat_score_host_test.cpp)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, repeat_accuracy, synth
from tests import repeat_map_ref as MR
from tests import repeat_score_cases as RC
from tests import repeat_score_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mauve_repeat_score", "mauve_repeat_score_ppv"]


def popcount(a):
    return int(sum(bin(int(v)).count("1") for v in a))


def consistent(res, records, nseq):
    t = res["totals"]
    length, mult, off, starts = records
    assert t["components_hit"] == popcount(res["comp_hit"]) and t["component_pairs_hit"] == popcount(res["pair_hit"])
    assert 0 <= t["sp_exact"] <= t["sp_truepos"] <= t["sp_possible"]
    assert t["components"] == int(np.sum(mult)) and t["component_pairs"] == int(np.sum(mult * (mult - 1) // 2)) and t["reserved"] == 0
    assert t["components_hit"] <= t["components"] and t["component_pairs_hit"] <= t["component_pairs"]
    P = res["pair_records"]
    assert P.shape == (nseq, nseq, SR.WORDS) and not P[np.tril_indices(nseq)].any() and not P[:, :, 3].any()
    assert (P[:, :, 2] <= P[:, :, 1]).all() and (P[:, :, 1] <= P[:, :, 0]).all()
    assert [int(P[:, :, k].sum()) for k in range(3)] == [t["sp_possible"], t["sp_truepos"], t["sp_exact"]]
    for r in range(len(length)):                               # a hit component has a partner; bits stay inside the multiplicity
        m = int(mult[r])
        assert int(res["comp_hit"][r]) >> m == 0 and bin(int(res["comp_hit"][r])).count("1") != 1
        seen = 0
        for c in range(m):
            w = int(res["pair_hit"][off[r] + c])
            assert w >> m == 0 and w & ((2 << c) - 1) == 0     # only bits above c
            if w:
                seen |= w | 1 << c
        assert seen == int(res["comp_hit"][r])


@pytest.mark.parametrize("name", list(RC.CASES))
def test_restatement_gives_the_hand_figures(name):
    c = RC.CASES[name]
    res = SR.score(c["truth"], c["records"], c["row_offset"])
    assert res["totals"] == c["totals"], name
    consistent(res, c["records"], c["truth"]["left"].shape[1])


def test_concatenated_form_equals_genome_coordinates():
    a, b = RC.CASES["hand3"], RC.CASES["hand3_concat"]
    ra, rb = SR.score(a["truth"], a["records"], a["row_offset"]), SR.score(b["truth"], b["records"], b["row_offset"])
    assert ra["totals"] == rb["totals"]
    for k in ("pair_records", "comp_hit", "pair_hit"):
        assert np.array_equal(ra[k], rb[k]), k


def test_hand_tables():
    """the tables of three cases spelled out, not only their counts"""
    r = SR.score(RC.CASES["tandem"]["truth"], RC.CASES["tandem"]["records"])
    assert r["comp_hit"].tolist() == [7] and r["pair_hit"].tolist() == [0b110, 0b100, 0] and r["pair_records"][0, 1].tolist() == [10, 10, 10, 0]
    r = SR.score(RC.CASES["nested"]["truth"], RC.CASES["nested"]["records"])
    assert r["comp_hit"].tolist() == [3, 7] and r["pair_hit"].tolist() == [2, 0, 6, 4, 0]
    assert r["pair_records"][0, 1].tolist() == [10, 10, 10, 0] and r["pair_records"][1, 2].tolist() == [10, 10, 10, 0]
    r = SR.score(RC.CASES["indel"]["truth"], RC.CASES["indel"]["records"])
    assert r["pair_records"][0, 1].tolist() == [9, 9, 5, 0]
    r = SR.score(RC.CASES["walk_back"]["truth"], RC.CASES["walk_back"]["records"])
    assert r["comp_hit"][0] == 3 and not r["comp_hit"][1:].any() and r["pair_hit"][0] == 2 and not r["pair_hit"][1:].any()


@pytest.mark.parametrize("seed,nrows,ncols,nrec", [(1, 2, 65, 4), (2, 5, 130, 12), (3, 32, 40, 9)])
def test_random_cases_are_consistent(seed, nrows, ncols, nrec):
    c = RC.random_case(seed, nrows, ncols, nrec)
    res = SR.score(c["truth"], c["records"])
    consistent(res, c["records"], nrows)
    assert 0 < res["totals"]["sp_truepos"] and res["totals"]["sp_exact"] < res["totals"]["sp_possible"]


# the planted input of the condition below: weight 15, 20 kb, 3 families of 2, 3 and 4 undiverged copies of 300 bases or more
PLANT_LENGTH, PLANT_FAMILIES, PLANT_SEED = 20000, [(300, 2, 0.0), (400, 3, 0.0), (350, 4, 0.0)], 0


def test_planted_repeats_generator():
    g, T = repeat_accuracy.planted_repeats(PLANT_LENGTH, PLANT_FAMILIES, PLANT_SEED)
    g2, T2 = repeat_accuracy.planted_repeats(PLANT_LENGTH, PLANT_FAMILIES, PLANT_SEED)
    assert np.array_equal(g, g2) and all(np.array_equal(T[k], T2[k]) for k in ("left", "right", "reverse", "col_off", "cols"))
    assert not np.array_equal(g, repeat_accuracy.planted_repeats(PLANT_LENGTH, PLANT_FAMILIES, PLANT_SEED + 1)[0])
    assert len(g) == PLANT_LENGTH and g.dtype == np.uint8 and T["left"].shape == (3, 4)
    spans = sorted((int(T["left"][f, r]), int(T["right"][f, r])) for f in range(3) for r in range(4) if T["left"][f, r])
    assert len(spans) == 9 and all(a[1] < b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] >= 1 and spans[-1][1] <= PLANT_LENGTH
    assert (T["left"][0, 2:] == 0).all() and (T["left"][1, 3:] == 0).all() and (T["left"] > 0).sum() == 9
    for f, (el, m, _) in enumerate(PLANT_FAMILIES):
        assert T["reverse"][f, 0] == 0 and T["reverse"][f, :m].any()              # copy 0 forward, a reversed copy in every family
        first = g[T["left"][f, 0] - 1:T["right"][f, 0]]
        assert T["col_off"][f + 1] - T["col_off"][f] == el and (T["cols"][T["col_off"][f]:T["col_off"][f + 1]] == (1 << m) - 1).all()
        for r in range(1, m):
            x = g[T["left"][f, r] - 1:T["right"][f, r]]
            assert np.array_equal(synth.revcomp(x) if T["reverse"][f, r] else x, first)
    # diverged copies: gaps appear and the rows still tile their extents
    g, T = repeat_accuracy.planted_repeats(8000, [(500, 3, 0.1)], 7)
    P = SR.truth_positions(T)[0]
    for r in range(3):
        q = P[r][P[r] > 0]
        assert len(q) == T["right"][0, r] - T["left"][0, r] + 1 and set(q.tolist()) == set(range(int(T["left"][0, r]), int(T["right"][0, r]) + 1))
    assert (P == 0).any()
    with pytest.raises(ValueError):
        repeat_accuracy.planted_repeats(1000, [(400, 3, 0.0)], 1)
    with pytest.raises(ValueError):
        repeat_accuracy.planted_repeats(1000, [(40, 1, 0.0)], 1)


def test_undiverged_planted_repeats_are_found_exactly():
    """a condition on the input, not a measurement: with mutation rate 0 the repeat map's restatement aligns every planted pair exactly"""
    g, T = repeat_accuracy.planted_repeats(PLANT_LENGTH, PLANT_FAMILIES, PLANT_SEED)
    records = MR.as_csr(MR.repeat_matches(g, _lib.get_seed(15, 0)))
    res = SR.score(T, records)
    t = res["totals"]
    assert t["sp_possible"] == 300 * 1 + 400 * 3 + 350 * 6 and t["sp_exact"] == t["sp_possible"] == t["sp_truepos"]
    consistent(res, records, 4)


def test_ppv_host_entry():
    rng = np.random.default_rng(5)
    for k in range(40):
        v = rng.integers(0, 1000, 8)
        if k % 4 == 0:
            v[0] = 0
        if k % 5 == 0:
            v[3] = 0
        if k % 7 == 0:
            v[5] = 0
        t = dict(zip(SR.TOTALS, (int(x) for x in v)))
        got = _lib.repeat_score_ppv(t)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.nan_to_num(np.array([v[1], v[2], v[4], v[6]], np.float64) / np.array([v[0], v[0], v[3], v[5]], np.float64), nan=0.0, posinf=0.0)
        assert [got[n] for n in ("sensitivity", "exact_sensitivity", "component_ppv", "pairwise_ppv")] == want.tolist(), v
        assert got == SR.ppv(t)
    z = _lib.repeat_score_ppv(dict.fromkeys(SR.TOTALS, 0))
    assert set(z.values()) == {0.0}
    assert _lib.repeat_score_ppv(_lib.RepeatScoreTotals(4, 3, 2, 8, 6, 6, 2, 0)) == dict(sensitivity=0.75, exact_sensitivity=0.5, component_ppv=0.75, pairwise_ppv=2 / 6)


def test_symbols_in_header_and_exports():
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "mauve_hip.h")) as f:
        hdr = f.read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(r"^(int|void) %s\(" % name, hdr, re.M), name
    assert ("typedef struct { int64_t sp_possible, sp_truepos, sp_exact, components, components_hit, component_pairs, component_pairs_hit, reserved; } "
            "mauve_repeat_score_totals;") in hdr
    assert tuple(f[0] for f in _lib.RepeatScoreTotals._fields_) == SR.TOTALS and _lib.C.sizeof(_lib.RepeatScoreTotals) == 64
    assert _lib.REPEAT_SCORE_WORDS == SR.WORDS


def test_host_side_under_sanitizers():
    """tests/cpp/repeat_score_host_test.cpp with the library's host source of the figures: a stand-alone program, host C++ only (the
    sanitizer runtimes are linked into it, so it runs the same whatever the environment preloads)"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "repeat_score_host_test")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                               "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "repeat_score_host_test.cpp"),
                               os.path.join(ROOT, "mauvealigner_amd", "csrc", "repeat_score_host.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
