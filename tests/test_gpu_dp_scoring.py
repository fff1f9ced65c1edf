"""The kernels that take a scoring scheme, under schemes other than the default (tests/scoring_schemes.py): every DP kernel family of
dp_batch.hip on every route, the admission boundary of the scan formulations, the sum-of-pairs scorers, and the whole path.  Bit-exact
against the CPU oracle, which tests/test_dp_scoring_cpu.py holds against two independent statements of S7 under the same schemes."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import dp_ref as R
from tests import dp_scoring_worker as W
from tests import scoring_schemes as SS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MAUVE_DP_ONE_WAVE", "MAUVE_DP_NOSCAN", "MAUVE_DP_NO_GROUPS", "MAUVE_DP_WIDE_MIN", "MAUVE_DP_BIG_MAX", "MAUVE_DP_NO_WIDE", "MAUVE_DP_CLUSTER",
            "MAUVE_DP_CLASS", "MAUVE_DP_TB_BUDGET", "MAUVE_CANON_DEVICE_MIN", "MAUVE_HOST_CHAIN")


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dp_reference(tmp_path_factory):
    """the oracle's result of every DP case, computed once for all routes"""
    ref = W.reference()
    path = str(tmp_path_factory.mktemp("dp_scoring") / "dp_ref.pickle")
    with open(path, "wb") as f:
        pickle.dump(ref, f)
    return ref, path


def _child(args, extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra, MAUVE_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "tests.dp_scoring_worker"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("OK"), str(extra) + "\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return r.stderr


TRACE = re.compile(r"\[trace\] dp_core: \d+ round\(s\); (\d+) intervals: (\d+) workgroup, (\d+) one-wave, (\d+) two/wave, (\d+) four/wave")


def _classes(stderr):
    """job name -> (intervals, workgroup, one-wave, two per wave, four per wave) of its launch, from the library's trace"""
    out, job = {}, None
    for line in stderr.splitlines():
        if line.startswith("[job] "):
            job = line[6:].strip()
        m = TRACE.search(line)
        if m and job is not None:
            out[job] = tuple(int(x) for x in m.groups())
    return out


BASE = "subwave,onewave,wide"
ROUTES = {
    "default": ({}, BASE + ",banded,boundary,hole"),
    "one_wave": ({"MAUVE_DP_ONE_WAVE": "1"}, BASE + ",boundary"),
    "one_wave_noscan": ({"MAUVE_DP_ONE_WAVE": "1", "MAUVE_DP_NOSCAN": "1"}, BASE),
    "wide": ({"MAUVE_DP_WIDE_MIN": "1"}, BASE + ",boundary,banded"),
    "wide_stripes": ({"MAUVE_DP_WIDE_MIN": "1", "MAUVE_DP_NO_WIDE": "1"}, BASE),
    "wide_no_cluster": ({"MAUVE_DP_WIDE_MIN": "1", "MAUVE_DP_CLUSTER": "0"}, BASE),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_dp_kernels_under_schemes(route, dp_reference):
    """ctx.dp_batch(scoring=) against O.align_interval(scoring=), columns and scores, every scheme of the table in one child process per
    route.  `pos_ext` and `huge` send every interval beyond the sub-wave classes to the fall-back kernels (the anti-diagonal sweep, the stripe
    pipeline) at any switches; `edge` does it for one of two intervals of a launch.  The library's trace shows which classes a launch held:
    a route must not pass because everything ran in one family."""
    extra, groups = ROUTES[route]
    cls = _classes(_child(["dp", dp_reference[1], groups], extra))
    assert len(cls) == sum(1 for g, *_ in W.dp_jobs() if g in groups.split(","))
    for scheme in SS.NAMES:
        n, big, med, s32, s16 = cls["subwave/fives/" + scheme]
        assert big == 0 and med < n                                            # the small intervals share waves
        for name in ("onewave/pairs/", "onewave/fives/", "wide/pairs/", "wide/fives/"):
            n, big, med, s32, s16 = cls[name + scheme]
            if route.startswith("one_wave"):
                assert big == 0 and med >= (2 if "pairs" in name else 1), (name, scheme)
            elif route.startswith("wide"):
                assert big >= (6 if "pairs" in name else 1), (name, scheme)      # every shape with a dimension above one band of 256 rows
        if not route.startswith("one_wave"):
            n, big, med, s32, s16 = cls["wide/pairs/" + scheme]
            assert big >= 2 and n - big >= 50                                  # workgroups beside the waves, at default switches too
    if "boundary" in groups:
        n, big, med, s32, s16 = cls["boundary/edge"]
        if route != "default":
            assert (big, med) == ((0, 2) if route == "one_wave" else (2, 0))       # both sides of the boundary in one kernel class
    if "hole" in groups:
        assert cls["hole/1600"][:2] == (1, 1) and cls["hole/32way"][:2] == (2, 2)      # workgroup entries, which is where the hole was
    if "banded" in groups:
        for scheme in ("asym", "zero_gaps", "huge"):
            assert cls["banded/cut/" + scheme][:2] == (1, 1) and cls["banded/tiny/" + scheme][1] >= 3   # (a banded step exists only in the workgroup kernel)


def test_scheme_beyond_the_domain_is_refused(ctx):
    """the domain of mauve_scoring (mauve_hip.h).  (1) Entries lie within +-MAUVE_SCORING_MAX = 2^20: the limit itself is
    accepted and exact, one past it is MAUVE_ERR_ARG from every entry point, and the message names the limit; so is a positive gap_open.  (2) The scheme fits the 32-bit
    DP at the lengths it is used on (SS.dp_need < 2^29): a pair just inside is accepted and exact, one base more is refused; gap_extend
    = -2^20 on a 3 kb pair, whose unclamped boundary row would wrap, is refused; mauve_align checks the largest interval its parameters admit"""
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(5)
    ivs = [W.seqs(rng, [40, 37]), W.seqs(rng, [300, 280])]
    at = (SS.ASYM, -(1 << 20), -7)
    assert all(SS.dp_need(at, [len(s) for s in iv]) < SS.DP_SCORE_MAX for iv in ivs)
    cols, score = ctx.dp_batch(ivs, scoring=SS.make(_lib.Scoring, *at))
    for iv, c, s in zip(ivs, cols, score):
        ec, es = O.align_interval(iv, scoring=SS.make(O.Scoring, *at))
        assert np.array_equal(c, ec) and int(s) == es
    bad = []
    for field in ("gap_open", "gap_extend", "matrix"):
        for v in ((1 << 20) + 1, -(1 << 20) - 1):
            s = SS.make(_lib.Scoring, SS.ASYM, -250, -45)
            if field == "matrix":
                s.matrix[2][1] = v
            else:
                setattr(s, field, v)
            bad.append(s)
    genomes = [rng.integers(0, 4, 500, dtype=np.uint8) for _ in range(2)]
    ctx.set_genomes(genomes)
    for s in bad:
        for call in (lambda: ctx.dp_batch(ivs, scoring=s), lambda: ctx.dp_batch(ivs, scoring=s, band_from=100),
                     lambda: ctx.match_sp_scores([10], [[1, 1]], scoring=s), lambda: ctx.align(_lib.default_params(scoring=s))):
            with pytest.raises(RuntimeError, match=r"\(-1\).*1048576"):
                call()
    # (1) a positive gap_open, small as it may be: a path alternating X and Y would collect it in every column
    for v in (1, 400):
        s = SS.make(_lib.Scoring, SS.ASYM, v, -45)
        for call in (lambda: ctx.dp_batch(ivs, scoring=s), lambda: ctx.dp_batch(ivs, scoring=s, band_from=100),
                     lambda: ctx.match_sp_scores([10], [[1, 1]], scoring=s), lambda: ctx.align(_lib.default_params(scoring=s))):
            with pytest.raises(RuntimeError, match=r"\(-1\).*positive gap_open"):
                call()
    # (2) at its boundary, per interval: 2 k |open| + (L + k n) |extend| + k max|S| against 2^29
    steep = (SS.ASYM, -250, -60000)
    inside, outside = W.seqs(rng, [2237, 2236], 0.05), W.seqs(rng, [2237, 2237], 0.05)
    assert SS.dp_need(steep, [2237, 2236]) < SS.DP_SCORE_MAX <= SS.dp_need(steep, [2237, 2237])
    for band_from in (None, 100000):
        cols, score = ctx.dp_batch([ivs[0], inside], scoring=SS.make(_lib.Scoring, *steep), band_from=band_from)
        ec, es = O.align_interval(inside, scoring=SS.make(O.Scoring, *steep))
        assert np.array_equal(cols[1], ec) and int(score[1]) == es
        with pytest.raises(RuntimeError, match=r"\(-1\).*536870912"):
            ctx.dp_batch([ivs[0], outside], scoring=SS.make(_lib.Scoring, *steep), band_from=band_from)
    wrap = (SS.ASYM, -250, -(1 << 20))                      # inside (1); row 0 of a pair reaches 2 x 2^20 x 2048 = 2^32 after 2048 columns
    with pytest.raises(RuntimeError, match=r"\(-1\).*536870912"):
        ctx.dp_batch([W.seqs(rng, [3000, 2900])], scoring=SS.make(_lib.Scoring, *wrap))
    # the whole path: two resident genomes, intervals of up to max_gapped_len bases each
    tall = (SS.ASYM, -250, -20000)
    assert SS.dp_need(tall, [5000, 5000]) < SS.DP_SCORE_MAX <= SS.dp_need(tall, [10000, 10000])
    with pytest.raises(RuntimeError, match=r"\(-1\).*536870912"):
        ctx.align(_lib.default_params(scoring=SS.make(_lib.Scoring, *tall)))
    r = ctx.align(_lib.default_params(scoring=SS.make(_lib.Scoring, *tall), max_gapped_len=5000))
    e = O.align(genomes, O.default_params(scoring=SS.make(O.Scoring, *tall), max_gapped_len=5000))
    assert np.array_equal(r["cols"], e["aln"]["cols"]) and np.array_equal(r["dp_score"], e["aln"]["dp_score"])
    ctx.align(_lib.default_params(scoring=SS.make(_lib.Scoring, *tall), gapped=0))        # (no DP, nothing to fit)


def test_device_front_end_at_the_admission_boundary():
    """mauve_align sizes and orders its DP intervals on the device (dpf_run), and that front end decides as dp_core does whether the stripe
    pipeline is launched: a gap of 1600 x 1600 bases at gap_open -50000 is a workgroup entry that the scans do not admit, in a call
    without a band.  Default switches, one child for the trace"""
    assert 2685 * 2 * -W.HOLE_GAP_OPEN >= 1 << 28 > 2684 * 2 * -W.HOLE_GAP_OPEN
    err = _child(["front"], {})
    m = re.search(r"\[trace\] dp \(device front[^)]*\): (\d+) intervals \((\d+) workgroup", err)
    assert m and int(m.group(2)) >= 1, err[-2000:]


# ---- the sum-of-pairs scorers (S11, S11d) ----
@pytest.mark.parametrize("N", [3, 5])
def test_match_sp_scores_under_schemes(ctx, N):
    """sp_score_matches: forward, reverse and absent components, lengths around the wave (1, 63, 64, 65) and a few hundred; against the numpy
    restatement and the oracle.  S11 reads S[b_x][b_y] for genomes x < y: the transposed matrix gives other scores"""
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(40 + N)
    genomes = [rng.integers(0, 4, 3000, dtype=np.uint8) for _ in range(N)]
    ln, st = W.match_cases(rng, genomes)
    ctx.set_genomes(genomes)
    for name in ("asym", "skew"):
        matrix = SS.SCHEMES[name][0]
        ref = R.match_sp_scores(genomes, ln, st, matrix)
        got = ctx.match_sp_scores(ln, st, scoring=SS.fill(_lib.Scoring, name))
        assert np.array_equal(got, ref)
        assert np.array_equal(got, O.match_sp_scores(genomes, ln, st, scoring=SS.fill(O.Scoring, name)))
        assert np.any(ref != R.match_sp_scores(genomes, ln, st, SS.HOXD70)) and np.any(ref != R.match_sp_scores(genomes, ln, st, SS.transposed(matrix)))


@pytest.mark.parametrize("N", [3, 5])
def test_repeat_penalized_scores_under_schemes(ctx, N):
    """sp_score_matches<NEGATIVE | ZERO>: the penalty divides the positive pair scores only, and `skew` has positive mismatches"""
    from mauvealigner_amd import _lib
    from tests.repeat_ref import repeat_genomes
    genomes = repeat_genomes(N, 4000, 3 + N, copies=10, elem=(150, 400))
    pat = O.get_seed(11, 0)
    mults = [O.seed_multiplicity(g, pat) for g in genomes]
    assert max(int(m.max()) for m in mults) >= 3
    rng = np.random.default_rng(50 + N)
    ln, st = W.match_cases(rng, genomes)
    ctx.set_genomes(genomes)
    for name in ("asym", "skew"):
        matrix = SS.SCHEMES[name][0]
        plain = R.match_sp_scores(genomes, ln, st, matrix)
        for mode in (1, 2):
            ref = R.match_sp_scores(genomes, ln, st, matrix, mults, mode)
            got = ctx.match_sp_scores_repeat(pat, mode, ln, st, scoring=SS.fill(_lib.Scoring, name))
            assert np.array_equal(got, ref), (name, mode)
            assert np.array_equal(got, O.match_sp_scores_repeat(genomes, mults, ln, st, mode, scoring=SS.fill(O.Scoring, name)))
            assert np.any(ref != plain)                                                   # the penalty is in force on these matches
            assert np.any(ref != R.match_sp_scores(genomes, ln, st, SS.HOXD70, mults, mode))
            assert np.any(ref != R.match_sp_scores(genomes, ln, st, SS.transposed(matrix), mults, mode))


# ---- the whole path ----
@pytest.fixture(scope="module")
def whole_reference(tmp_path_factory):
    ref = W.whole_reference()
    path = str(tmp_path_factory.mktemp("dp_scoring_whole") / "whole_ref.pickle")
    with open(path, "wb") as f:
        pickle.dump(ref, f)
    return ref, path


def test_whole_path_under_schemes(ctx, whole_reference):
    """align, align with score-weighted LCBs (sp_score_matches, sp_default_min_weight) and progressive_align at the call site's defaults
    (sum-of-pairs LCB weights, weight scaling, two refinement rounds: dp_sp_scores) under `asym` and `unit`, on C3 and C4.  That these
    schemes matter on these inputs -- the expected result is neither the default's nor the transposed matrix's -- is asserted on the same
    W.whole_reference() by tests/test_dp_scoring_cpu.py::test_the_schemes_matter_on_the_whole_path (it needs no GPU)"""
    from mauvealigner_amd import _lib
    W.run_whole(ctx, _lib, whole_reference[0])


def test_whole_path_under_schemes_device_chain(whole_reference):
    """the same in a process with MAUVE_CANON_DEVICE_MIN=1: the device chain scores its records itself (ch_sp_scores) and the device tail
    assembles the result"""
    err = _child(["whole", whole_reference[1]], {"MAUVE_CANON_DEVICE_MIN": "1"})
    assert "chain (device)" in err
