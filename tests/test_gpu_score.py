"""An alignment scored against a correct one on the device: mauve_score_truth + mauve_score_alignment against the numpy
restatement tests/score_ref.py, counter for counter (everything is integer: every comparison is for equality)."""
import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O
from tests import score_ref as SR
from tests.test_accuracy import SCORE_CASES
from tests.test_gpu_coord import _disjoint_alignment
from tests.test_score_cpu import COUNTS, case, check_ratios, check_row_sums

pytestmark = pytest.mark.gpu
BLOCK = 448                 # columns per block record of the index (CO_BLOCK, coord_index.hpp); a word is 64 columns, a sample 512 residues
KEYS = ("left", "right", "reverse", "col_off", "cols")


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _index(ctx, a):
    ctx.coord_index_alignment(*[a[k] for k in KEYS])


def _score(ctx, T, Cc, N):
    """index C, load T, score: the records equal the restatement; -> records"""
    _index(ctx, Cc)
    ctx.score_truth(T)
    rec = ctx.score_alignment()
    want = SR.score_records(T, Cc, N)
    assert rec.shape == want.shape and rec.dtype == np.int64
    assert np.array_equal(rec, want), (np.argwhere(rec != want)[:5], rec[rec != want][:5], want[rec != want][:5])
    check_row_sums(rec, T, N)
    return rec


def _slots(rec):
    return rec[..., :6].reshape(-1, 6).sum(axis=0)


# ---- 1. the tool's cases ----
@pytest.mark.parametrize("k", range(len(SCORE_CASES)))
def test_score_tool_cases(ctx, k):
    from mauvealigner_amd import _lib
    c = case(k)
    _index(ctx, c["calc"])
    ctx.score_truth(c["truth"])
    rec = ctx.score_alignment()
    assert np.array_equal(rec, c["records"]), np.argwhere(rec != c["records"])[:5]
    t = _lib.score_totals(rec)
    for key in COUNTS + ("total",):
        assert t[key] == c["reference"][key], (key, t, c["reference"])
    check_ratios(t, c["golden"], SCORE_CASES[k])


# ---- 2. reverse strands, several intervals, absent genomes ----
@pytest.fixture(scope="module")
def inverted():
    gs = synth.star_genomes(3, 6000, 0.08, 11, inversions=2)
    T = O.align(gs)["aln"]
    Cc = O.align(gs, O.default_params(seed_weight=11, recursive=0))["aln"]
    return gs, {k: T[k] for k in KEYS}, {k: Cc[k] for k in KEYS}


def test_score_reverse_strands_and_absent_genomes(ctx, inverted):
    gs, T, Cc = inverted
    assert T["left"].shape == (11, 3) and T["reverse"].any(axis=1).sum() == 2
    assert Cc["left"].shape == (15, 3) and Cc["reverse"].any(axis=1).sum() == 2 and (Cc["left"] == 0).sum() == 20
    want = SR.score_records(T, Cc, 3)
    assert _slots(want).tolist() == [35386, 42, 26, 48, 26, 442] and (_slots(want) > 0).all()
    rec = _score(ctx, T, Cc, 3)
    assert _slots(rec).tolist() == [35386, 42, 26, 48, 26, 442]
    # T and C swapped (the default alignment covers every base: nothing is unaligned in it)
    rec = _score(ctx, Cc, T, 3)
    assert _slots(rec).tolist() == [35386, 42, 26, 0, 74, 442]


def test_score_resident_route(ctx, inverted):
    """C from mauve_align + mauve_coord_index: the columns are still on the device"""
    from mauvealigner_amd import _lib
    gs, T, Cc = inverted
    ctx.set_genomes(gs)
    ctx.score_truth(T)
    sz = ctx.align(_lib.default_params(seed_weight=11, recursive=0), fetch=False)
    assert sz["n_iv"] == 15
    ctx.coord_index()
    rec = ctx.score_alignment()
    want = SR.score_records(T, Cc, 3)
    assert (_slots(want) > 0).all() and np.array_equal(rec, want), np.argwhere(rec != want)[:5]
    # and the other way round: the truth fetched from the device, the index of the oracle's arrays
    r = ctx.align(_lib.default_params())
    assert np.array_equal(r["cols"], T["cols"])
    ctx.score_truth(r)
    _index(ctx, Cc)
    assert np.array_equal(ctx.score_alignment(), want)


# ---- 3. index geometry ----
def _two(parts):
    """intervals of 2 genomes from lists of column masks, positions running on from interval to interval"""
    n_iv = len(parts)
    left, right = np.zeros((n_iv, 2), np.int64), np.zeros((n_iv, 2), np.int64)
    at = [1, 1]
    for i, m in enumerate(parts):
        m = np.asarray(m, np.uint32)
        for g in range(2):
            n = int(np.count_nonzero(m >> np.uint32(g) & np.uint32(1)))
            if n:
                left[i, g], right[i, g] = at[g], at[g] + n - 1
                at[g] += n
    cols = np.concatenate([np.asarray(m, np.uint32) for m in parts]) if parts else np.zeros(0, np.uint32)
    col_off = np.concatenate([[0], np.cumsum([len(m) for m in parts])]).astype(np.int64)
    return dict(left=left, right=right, reverse=np.zeros((n_iv, 2), np.int8), col_off=col_off, cols=cols)


def _masks(rng, n):
    m = rng.choice(np.array([1, 2, 3], np.uint32), n, p=[0.15, 0.15, 0.7])
    m[0] = 3
    return m


def _shifted(m):
    """genome 0's row one column later: a gap column at its front"""
    r0 = np.concatenate([[0], m & 1]).astype(np.uint32)
    r1 = np.concatenate([m & 2, [0]]).astype(np.uint32)
    s = r0 | r1
    return s[s != 0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 447, 448, 449, 897])
def test_score_block_and_word_boundaries(ctx, n):
    rng = np.random.default_rng(7000 + n)
    m = _masks(rng, n)
    A = _two([m])
    rec = _score(ctx, A, _two([_shifted(m)]), 2)
    if n > 1:
        assert rec[..., 1].sum() > 0 and rec[..., 4].sum() > 0         # fp_base and fn_base appear
    rec = _score(ctx, _two([_shifted(m)]), A, 2)
    cut = _two([m[:BLOCK], m[BLOCK:]])
    assert cut["col_off"].tolist() == [0, min(n, BLOCK), n]
    for T, Cc in ((A, cut), (cut, A)):
        rec = _score(ctx, T, Cc, 2)
        assert not rec[..., 1:5].any()                                  # the same pairs, cut differently: all correct
    rec = _score(ctx, A, A, 2)
    assert not rec[..., 1:5].any() and rec[0, 1, 0] == np.count_nonzero(m == 3)


@pytest.mark.parametrize("n", [512, 513])
def test_score_sample_distance(ctx, n):
    """genome 0 with exactly n residues: the last sample of the index sits on, or one behind, its last residue"""
    rng = np.random.default_rng(7100 + n)
    m = _masks(rng, 700)
    at = np.flatnonzero(m & 1)
    m = m[:at[n - 1] + 1]
    assert np.count_nonzero(m & 1) == n
    A, B = _two([m]), _two([_shifted(m)])
    assert A["right"][0, 0] == n
    _score(ctx, A, B, 2)
    _score(ctx, B, A, 2)


def test_score_single_column_intervals_and_empty_alignments(ctx):
    rng = np.random.default_rng(7200)
    m = _masks(rng, 130)
    A = _two([m])
    single = _two([m[i:i + 1] for i in range(len(m))])
    assert single["left"].shape == (130, 2)
    rec = _score(ctx, single, A, 2)
    assert not rec[..., 1:5].any()
    _score(ctx, single, _two([_shifted(m)]), 2)
    _score(ctx, A, single, 2)
    none = _two([])
    assert none["left"].shape == (0, 2) and none["col_off"].tolist() == [0]
    rec = _score(ctx, A, none, 2)                                       # a C with no interval: everything is fn_unaligned / tn
    assert rec[..., 3].sum() == 2 * np.count_nonzero(m == 3) and rec[..., 5].sum() == np.count_nonzero(m != 3) and not rec[..., [0, 1, 2, 4]].any()
    rec = _score(ctx, none, A, 2)                                       # a T with no interval: zeros
    assert not rec.any()
    rec = _score(ctx, _two([np.zeros(0, np.uint32)]), A, 2)             # ... with an interval without columns
    assert not rec.any()


# ---- 4. width ----
def _perturbed(rng, a, N):
    """a copy with a random 5 % of one genome's residues of one interval moved into columns of their own"""
    left, col_off, cols = a["left"], a["col_off"], a["cols"]
    cnt = np.where(left != 0, a["right"] - left + 1, 0)
    shared = [(int(cnt[i, g]), i, g) for i in range(left.shape[0]) for g in range(N) if np.count_nonzero(left[i]) > 1]
    _, i, g = max(shared)
    bit = np.uint32(1 << g)
    parts, lens = [], []
    for k in range(left.shape[0]):
        m = cols[col_off[k]:col_off[k + 1]]
        if k == i:
            out = []
            for c in m:
                if c & bit and c != bit and rng.random() < 0.05:
                    out += [c & ~bit, bit]
                else:
                    out.append(c)
            m = np.array(out, np.uint32)
        parts.append(m)
        lens.append(len(m))
    b = {k: a[k].copy() for k in KEYS}
    b["cols"] = np.concatenate(parts)
    b["col_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return b


@pytest.mark.parametrize("N", [2, 5, 17, 32])
def test_score_random_wide_alignments(ctx, N):
    rng = np.random.default_rng(7300 + N)
    A, B = _disjoint_alignment(rng, N, 6, 3), _disjoint_alignment(rng, N, 6, 3)
    rec = _score(ctx, A, B, N)                                          # positions need not mean anything
    assert rec.shape == (N, N, 8)
    P = _perturbed(rng, A, N)
    assert len(P["cols"]) > len(A["cols"])
    rec = _score(ctx, A, P, N)
    s = _slots(rec)
    assert s[0] > s[1:5].sum() and s[2] > 0, s                          # tp dominates; a moved residue is a gap in C where T has a base ...
    s2 = _slots(_score(ctx, P, A, N))                                   # ... and a base in C where T has none
    assert s2[0] == s[0] and s2[4] == s[2], (s, s2)


# ---- 5. state ----
def test_score_state_and_errors(ctx):
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(7400)
    m = _masks(rng, 300)
    A, B = _two([m]), _two([_shifted(m)])
    fresh = _lib.Context(0)
    try:
        with pytest.raises(RuntimeError, match=r"mauve_score_alignment failed \(-5\).*no correct alignment"):
            fresh.score_alignment()
        fresh.score_truth(A)                                            # no genomes set, no index
        with pytest.raises(RuntimeError, match=r"mauve_score_alignment failed \(-5\).*no index"):
            fresh.score_alignment()
        _index(fresh, B)
        want = SR.score_records(A, B, 2)
        assert np.array_equal(fresh.score_alignment(), want)
        # an index over another number of genomes
        W = _disjoint_alignment(rng, 3, 2, 2)
        _index(fresh, W)
        with pytest.raises(RuntimeError, match=r"mauve_score_alignment failed \(-5\).*2 genomes.*3"):
            fresh.score_alignment()
        _index(fresh, B)                                                # coord_index* leaves the truth usable
        assert np.array_equal(fresh.score_alignment(), want)
        # a refused truth: overlapping intervals, inconsistent columns (the earlier truth is gone: a state error, not stale counts)
        over = _two([m[:100], m[100:]])
        over["left"][1, 0] -= 1
        over["right"][1, 0] -= 1
        with pytest.raises(RuntimeError, match=r"mauve_score_truth failed \(-1\): score_truth: intervals 0 and 1 overlap in genome 0"):
            fresh.score_truth(over)
        with pytest.raises(RuntimeError, match=r"mauve_score_alignment failed \(-5\).*no correct alignment"):
            fresh.score_alignment()
        short = _two([m])
        short["right"][0, 1] += 1
        with pytest.raises(RuntimeError, match=r"mauve_score_truth failed \(-1\): score_truth: the columns of interval 0"):
            fresh.score_truth(short)
        assert fresh.coord_index_size() == (2, 1, len(B["cols"]))      # the index in force stayed
        fresh.score_truth(B)
        assert np.array_equal(fresh.score_alignment(), SR.score_records(B, B, 2))
        fresh.score_truth(A)                                            # a second truth replaces the first
        assert np.array_equal(fresh.score_alignment(), want)
    finally:
        fresh.close()


def test_score_truth_leaves_index_and_selection(ctx):
    from mauvealigner_amd import _lib
    gs = synth.star_genomes(3, 3000, 0.05, 5)
    ctx.set_genomes(gs)
    r = ctx.align(_lib.default_params())
    ctx.coord_index()
    n_sel = ctx.extract_select(require=7)
    rows0 = ctx.extract_fetch()[0].copy()
    other = O.align(gs, O.default_params(seed_weight=9, recursive=0))["aln"]
    ctx.score_truth(other)
    assert ctx.coord_index_size() == (3, r["n_iv"], r["n_cols"])
    rows1 = ctx.extract_fetch()[0]                                      # the selection made before the truth is still usable
    assert rows1.shape == (3, n_sel) and np.array_equal(rows0, rows1)
    want = SR.score_records(other, r, 3)
    rec = ctx.score_alignment()
    assert np.array_equal(rec, want)
    # an upload and another alignment: the truth stays, the new index is scored
    ctx.set_genomes(gs)
    ctx.align(_lib.default_params(seed_weight=9, recursive=0), fetch=False)
    ctx.coord_index()
    rec2 = ctx.score_alignment()
    assert np.array_equal(rec2, SR.score_records(other, other, 3)) and not rec2[..., 1:5].any()
    # page-locked and pageable records, twice: identical bytes
    pin = _lib.pinned_empty((3, 3, 8), np.int64)
    pin[:] = -1
    got = ctx.score_alignment(out=pin)
    assert got is pin and np.array_equal(pin, rec2)
    page = np.full((3, 3, 8), -1, np.int64)
    assert ctx.score_alignment(out=page) is page and page.tobytes() == pin.tobytes() == ctx.score_alignment().tobytes()
    with pytest.raises(ValueError):
        ctx.score_alignment(out=np.zeros((3, 3, 6), np.int64))
