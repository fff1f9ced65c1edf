"""The CPU oracle under the scoring schemes of tests/scoring_schemes.py: against the exhaustive optimum (tests/bruteforce.py),
against the plain restatement of S7 (tests/dp_ref.py: columns and score) and, for the sum-of-pairs scorers (S11, S13), against
numpy / Python restatements.  Every test also shows that the scheme matters on its inputs: the reference result differs
from the default scheme's and, for an asymmetric matrix, from the transposed matrix's."""
import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O
from tests import bruteforce as B
from tests import dp_ref as R
from tests import scoring_schemes as SS
from tests import dp_scoring_worker as W
from tests.dp_scoring_worker import match_cases


@pytest.mark.parametrize("name", SS.NAMES)
def test_dp_optimal_vs_exhaustive_schemes(name):
    """test_dp_optimal_vs_exhaustive's check (tests/test_oracle.py) under every scheme: the oracle's score is the exhaustive
    optimum and its path scores what it says, on 60 random tiny profile-against-sequence steps"""
    matrix, go, ge = SS.SCHEMES[name]
    sc = SS.fill(O.Scoring, name)
    differs_default = differs_transposed = False
    for seed in range(60):
        rng = np.random.default_rng(100 + seed)
        m, n = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        k = int(rng.integers(1, 4))
        cnt = np.zeros((m, 4), dtype=np.uint8)
        for i in range(m):
            for _ in range(int(rng.integers(1, k + 1))):
                cnt[i, int(rng.integers(0, 4))] += 1
        seq = rng.integers(0, 4, n, dtype=np.uint8)
        ops, score = O.profile_dp(cnt, k, seq, scoring=sc)
        if m == 0 and n == 0:
            assert score == 0 and len(ops) == 0
            continue
        best = B.brute_best_score(cnt.tolist(), k, seq.tolist(), matrix, go, ge)
        assert score == best, (seed, m, n, k)
        assert B.score_path(ops.tolist(), cnt.tolist(), k, seq.tolist(), matrix, go, ge) == score
        differs_default |= best != B.brute_best_score(cnt.tolist(), k, seq.tolist(), SS.HOXD70, *SS.DEFAULT_GAPS)
        differs_transposed |= best != B.brute_best_score(cnt.tolist(), k, seq.tolist(), SS.transposed(matrix), go, ge)
    assert differs_default
    assert differs_transposed == (matrix is not SS.UNIT)          # (random profile columns are mixed, so this shows under zero_gaps too)


def _intervals(seed, count=40):
    """2-5 sequence slots of 0-60 bases: related sequences, empty members, an unrelated one now and then"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        nseq = int(rng.integers(2, 6))
        base = rng.integers(0, 4, 60, dtype=np.uint8)
        iv = []
        for _ in range(nseq):
            u = rng.random()
            L = int(rng.integers(0, 61))
            if u < 0.15:
                iv.append(np.zeros(0, np.uint8))
            elif u < 0.25:
                iv.append(rng.integers(0, 4, L, dtype=np.uint8))
            else:
                iv.append(synth.mutate(base, 0.2, rng, indel_frac=0.3)[:L])
        out.append(iv)
    return out


@pytest.mark.parametrize("name", SS.NAMES)
def test_oracle_equals_the_plain_restatement(name):
    """O.align_interval(scoring=) against dp_ref.align_interval: columns and score, about 40 intervals per scheme"""
    matrix, go, ge = SS.SCHEMES[name]
    sc = SS.fill(O.Scoring, name)
    ivs = _intervals(7)
    ref = [R.align_interval(iv, matrix, go, ge) for iv in ivs]
    for iv, (rc, rs) in zip(ivs, ref):
        ec, es = O.align_interval(iv, scoring=sc)
        assert ec.tolist() == rc and es == rs, [len(s) for s in iv]
    # the scheme matters on these inputs
    assert ref != [R.align_interval(iv, SS.HOXD70, *SS.DEFAULT_GAPS) for iv in ivs]
    other = [R.align_interval(iv, SS.transposed(matrix), go, ge) for iv in ivs]
    assert (ref != other) == (name in SS.ASYMMETRIC)


def test_restatement_equals_the_oracle_at_the_default():
    """the restatement itself, where the oracle has long been checked (HOXD70, -400 / -30)"""
    for iv in _intervals(8, 25):
        ec, es = O.align_interval(iv)
        rc, rs = R.align_interval(iv, SS.HOXD70, *SS.DEFAULT_GAPS)
        assert ec.tolist() == rc and es == rs


@pytest.mark.parametrize("name", ["asym", "skew"])
@pytest.mark.parametrize("N", [3, 5])
def test_match_sp_scores_schemes(name, N):
    matrix = SS.SCHEMES[name][0]
    rng = np.random.default_rng(40 + N)
    genomes = [rng.integers(0, 4, 3000, dtype=np.uint8) for _ in range(N)]
    ln, st = match_cases(rng, genomes)
    ref = R.match_sp_scores(genomes, ln, st, matrix)
    assert np.array_equal(O.match_sp_scores(genomes, ln, st, scoring=SS.fill(O.Scoring, name)), ref)
    assert np.any(ref != R.match_sp_scores(genomes, ln, st, SS.HOXD70))
    assert np.any(ref != R.match_sp_scores(genomes, ln, st, SS.transposed(matrix)))
    # S11 reads S[b_x][b_y] for x < y: the transposed matrix is what the swapped pair order would read
    assert np.array_equal(O.match_sp_scores(genomes, ln, st, scoring=SS.fill(O.Scoring, name, transpose=True)),
                          R.match_sp_scores(genomes, ln, st, SS.transposed(matrix)))


@pytest.mark.parametrize("name", ["asym", "skew"])
def test_sp_score_cols_schemes(name):
    """S13 objective: O.sp_score_cols against the restatement, on the columns the oracle aligned (empty members included)"""
    matrix, go, ge = SS.SCHEMES[name]
    sc = SS.fill(O.Scoring, name)
    ivs = _intervals(9, 30)
    cols = [O.align_interval(iv, scoring=sc)[0] for iv in ivs]
    ref = [R.sp_score_cols(iv, c, matrix, go, ge) for iv, c in zip(ivs, cols)]
    assert [O.sp_score_cols(iv, c, scoring=sc) for iv, c in zip(ivs, cols)] == ref
    assert ref != [R.sp_score_cols(iv, c, SS.HOXD70, *SS.DEFAULT_GAPS) for iv, c in zip(ivs, cols)]
    assert ref != [R.sp_score_cols(iv, c, SS.transposed(matrix), go, ge) for iv, c in zip(ivs, cols)]
    # the open / extend rule: a run of one-sided columns costs open once; swapping the two must show
    assert ref != [R.sp_score_cols(iv, c, matrix, ge, go) for iv, c in zip(ivs, cols)]


# ---- what the cases of tests/test_gpu_dp_scoring.py rely on (no GPU needed to know it) ----
def test_the_gpu_dp_cases_are_where_they_should_be():
    """the admission boundary of the scan kernels (dp3_admissible: total length x sequences x max(|open|, |extend|) < 2^28 and no
    positive gap term), the live band, and that the scheme matters on every case"""
    ref = W.reference()
    jobs = {name: (scheme, band_from, ivs) for _, name, scheme, band_from, ivs in W.dp_jobs()}
    lim = 1 << 28
    total = lambda iv: sum(len(s) for s in iv)
    scheme, _, ivs = jobs["boundary/edge"]
    assert [total(iv) for iv in ivs] == [700, 600] and 600 * 2 * -scheme[1] < lim <= 700 * 2 * -scheme[1]
    assert all(max(len(s) for s in iv) > 256 for iv in ivs)
    scheme, _, ivs = jobs["hole/1600"]
    assert total(ivs[0]) == 3200 and 3200 * 2 * -scheme[1] >= lim and 3200 * 2 * 400 < lim      # (the default scheme admits it)
    scheme, _, ivs = jobs["hole/32way"]
    assert scheme == (SS.HOXD70, -400, -30) and [[len(s) for s in iv] for iv in ivs] == [[660] * 32, [650] * 32]
    assert 650 * 32 * 32 * 400 < lim <= 660 * 32 * 32 * 400
    # `huge`: nothing with a dimension beyond one band of 256 rows is admitted
    for group in ("onewave", "wide"):
        for _, ivs in W.shapes()[group]:
            assert all(total(iv) * len(iv) * 1000000 >= lim for iv in ivs if max(len(s) for s in iv) > 256)
    # every case lies inside the domain of its scheme (mauve_hip.h at mauve_scoring), so the library accepts it and nothing can wrap
    assert all(SS.dp_need(scheme, [len(s) for s in iv]) < SS.DP_SCORE_MAX for scheme, _, ivs in jobs.values() for iv in ivs)
    # no clamp in sight: the oracle's scores stay far above -2^29
    assert min(s for name in ref for _, s in ref[name]) > -(1 << 24)
    # the band is live: the banded optimum is below the full one.  Under `zero_gaps` the pair with 500 bases inserted and 500 dropped is
    # aligned as well inside the band as outside it -- free gaps find as many chance matches near the diagonal as the shifted copy
    # offers -- so the swapped pair stands in there.  Under `huge` no input of this size can leave the band: between two sequences of
    # equal length a second gap run costs 2 x 10^6, more than 3 kb of matches give back, and ONE run of |n - m| columns always fits the band
    for name in ("banded/cut/asym", "banded/swap/asym", "banded/swap/zero_gaps"):
        scheme, band_from, ivs = jobs[name]
        assert ref[name][0][1] < W._oracle_dp(O, ivs, scheme, None)[0][1], name
    # the expected result (columns and score) differs from the default scheme's in every case; from the transposed matrix's in every case
    # under `asym` and `skew`, and in some case of every kernel family under the other schemes that can show it
    flat = lambda res: [(c.tolist(), s) for c, s in res]
    for scheme in SS.NAMES:
        for group, cases in W.shapes().items():
            live = []
            for case, ivs in cases:
                name = "%s/%s/%s" % (group, case, scheme)
                mine = flat(ref[name])
                assert mine != flat(W._oracle_dp(O, ivs, (SS.HOXD70,) + SS.DEFAULT_GAPS, None)), name
                live.append(mine != flat(W._oracle_dp(O, ivs, SS.SCHEMES[scheme], None, transpose=True)))
            if scheme in ("asym", "skew"):
                assert all(live), (group, scheme)
            assert any(live) == (scheme in SS.ASYMMETRIC), (group, scheme)


def test_the_schemes_matter_on_the_whole_path():
    """the oracle's whole-path result under `asym` is neither the default scheme's nor the transposed matrix's, under `unit` not the
    default's: the columns of every kind of run, and the LCB weights where they are scores"""
    ref = W.whole_reference()
    for cfg, scale in W.WHOLE_CONFIGS:
        gs = W.whole_genomes(cfg, scale)
        for kind in W.WHOLE_KINDS:
            others = {"default": W.whole_oracle(O, gs, kind, SS.default(O.Scoring)),
                      "asym_t": W.whole_oracle(O, gs, kind, SS.fill(O.Scoring, "asym", transpose=True))}
            for scheme, against in (("asym", ("default", "asym_t")), ("unit", ("default",))):
                mine = ref[(cfg, scheme, kind)]
                for o in against:
                    assert not np.array_equal(mine["aln"]["cols"], others[o]["aln"]["cols"]), (cfg, kind, scheme, o)
                    if kind == "align_sp":
                        assert not np.array_equal(mine["lcbs"]["weight"], others[o]["lcbs"]["weight"]), (cfg, scheme, o)
