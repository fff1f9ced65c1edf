"""GPU parity tests of the backbone / island stage (mauve_backbone, mauve_backbone_alignment) against the
CPU oracle's column-by-column restatement.  Integer work: every segment, genome set, column range and coordinate must
match exactly."""
import functools

import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O
from tests.backbone_cases import GAPS, random_case, random_alignment as _random_alignment  # noqa: F401 (tests/test_gpu_coord.py takes the generator from here)

pytestmark = pytest.mark.gpu
KEYS = ("seg_iv", "seg_col", "seg_len", "seg_mask", "seg_left", "seg_right", "islands")


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _same(r, e):
    for k in KEYS:
        assert r[k].shape == e[k].shape, (k, r[k].shape, e[k].shape)
        assert np.array_equal(r[k], e[k]), k


def test_backbone_hand_case(ctx):
    """genome 1 lacks five columns the other two share: with island_gap 3 they are an island of 0 and of 2 against 1,
    the backbone is {0,1,2} / {0,2} / {0,1,2}; with island_gap 5 the gap is small and one segment covers everything"""
    cols = np.array([7] * 10 + [5] * 5 + [7] * 5, np.uint32)
    left, right, rev = np.array([[1, 101, 201]]), np.array([[20, 115, 220]]), np.array([[0, 0, 1]], np.int8)
    r = ctx.backbone_alignment(left, right, rev, [0, 20], cols, island_gap=3)
    assert r["seg_mask"].tolist() == [7, 5, 7] and r["seg_col"].tolist() == [0, 10, 15] and r["seg_len"].tolist() == [10, 5, 5]
    assert r["seg_left"].tolist() == [[1, 101, -211], [11, 0, -206], [16, 111, -201]]
    assert r["seg_right"].tolist() == [[10, 110, -220], [15, 0, -210], [20, 115, -205]]
    assert r["islands"].tolist() == [[0, 0, 1, 0, 10, 14, 11, 15], [0, 1, 2, 2, 10, 14, -206, -210]]
    _same(r, O.backbone(left, right, rev, [0, 20], cols, island_gap=3))
    r = ctx.backbone_alignment(left, right, rev, [0, 20], cols, island_gap=5)
    assert r["seg_mask"].tolist() == [7] and r["seg_len"].tolist() == [20] and len(r["islands"]) == 0
    # nothing to do: single-genome intervals only, and no interval at all
    r = ctx.backbone_alignment(np.array([[1, 0]]), np.array([[5, 0]]), np.zeros((1, 2), np.int8), [0, 5], np.full(5, 1, np.uint32))
    assert len(r["seg_iv"]) == 0 and len(r["islands"]) == 0
    r = ctx.backbone_alignment(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int8), [0], np.zeros(0, np.uint32))
    assert len(r["seg_iv"]) == 0


@pytest.mark.parametrize("seed", range(6))
def test_backbone_random_alignments(ctx, seed):
    left, right, rev, col_off, cols = random_case(seed)
    for gap in GAPS:
        r = ctx.backbone_alignment(left, right, rev, col_off, cols, island_gap=gap)
        e = O.backbone(left, right, rev, col_off, cols, island_gap=gap)
        _same(r, e)
    assert len(e["seg_iv"]) > 0


def test_backbone_record_list_regrows(ctx):
    """more open regions than the record list holds at first: the launch is repeated with room"""
    rng = np.random.default_rng(5)
    n = 400000
    cols = np.where(np.arange(n) % 3 == 0, 3, np.where(np.arange(n) % 3 == 1, 1, 3)).astype(np.uint32)     # an island of one every third column
    left, right, rev = np.array([[1, 1]]), np.array([[n, int(np.count_nonzero(cols & 2))]]), np.zeros((1, 2), np.int8)
    r = ctx.backbone_alignment(left, right, rev, [0, n], cols, island_gap=0)
    e = O.backbone(left, right, rev, [0, n], cols, island_gap=0)
    assert len(e["islands"]) > 100000
    _same(r, e)
    del rng


def _partition_checks(r, a, N):
    """every genome's segments lie inside their interval and do not overlap one another"""
    for g in range(N):
        rows = np.flatnonzero(r["seg_mask"] >> np.uint32(g) & 1)
        lo = np.abs(r["seg_left"][rows, g])
        hi = np.abs(r["seg_right"][rows, g])
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
        iv = r["seg_iv"][rows]
        assert np.all(lo >= a["left"][iv, g]) and np.all(hi <= a["right"][iv, g])
        o = np.argsort(lo)
        assert np.all(lo[o][1:] > hi[o][:-1])


def test_backbone_of_the_resident_alignment(ctx):
    """mauve_backbone on the columns the alignment left in HBM (device tail) and on a host-assembled result
    (progressive path) = the oracle on the fetched alignment"""
    from mauvealigner_amd import _lib
    import os
    gs = synth.make_config("C3", scale=0.03)
    N = len(gs)
    ctx.set_genomes(gs)
    old = os.environ.get("MAUVE_CANON_DEVICE_MIN")
    os.environ["MAUVE_CANON_DEVICE_MIN"] = "1"               # small lists take the device tail as well
    try:
        sz = ctx.align(_lib.default_params(), fetch=False)
        r = ctx.backbone(island_gap=20)                      # before any fetch: the columns are only in HBM
        a = ctx.align(_lib.default_params())
    finally:
        if old is None:
            del os.environ["MAUVE_CANON_DEVICE_MIN"]
        else:
            os.environ["MAUVE_CANON_DEVICE_MIN"] = old
    assert sz["n_iv"] == a["n_iv"]
    e = O.backbone(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], island_gap=20)
    _same(r, e)
    assert len(r["seg_iv"]) >= a["n_lcb"] and np.any(r["seg_mask"] == (1 << N) - 1)
    _partition_checks(r, a, N)
    _same(ctx.backbone(island_gap=20), e)                    # after the fetch as well
    # the progressive path assembles on the host: the columns are uploaded
    gs4 = synth.make_config("C4", scale=0.02)
    ctx.set_genomes(gs4)
    p = ctx.progressive_align(_lib.default_params())
    r = ctx.backbone(island_gap=20)
    e = O.backbone(p["left"], p["right"], p["reverse"], p["col_off"], p["cols"], island_gap=20)
    _same(r, e)
    assert len(set(r["seg_mask"].tolist())) > 1              # clade-specific backbone next to the all-genome one
    _partition_checks(r, p, len(gs4))
    # an alignment that kept nothing (no LCB reaches the weight, leftovers not listed) has an empty backbone
    ctx.set_genomes(gs)
    z = ctx.align(_lib.default_params(lcb_weight=10 ** 9, add_unaligned=0))
    assert z["n_iv"] == 0
    r = ctx.backbone()
    assert len(r["seg_iv"]) == 0 and len(r["islands"]) == 0
    # error behaviour: nothing aligned yet in a fresh context, gap out of range
    c2 = _lib.Context(0)
    with pytest.raises(RuntimeError):
        c2.backbone()
    c2.close()
    with pytest.raises(RuntimeError):
        ctx.backbone(island_gap=-1)


def test_inconsistent_columns_are_refused(ctx):
    """A caller's alignment whose columns do not hold the residues its ends announce (the homology pass would turn the surplus into
    base addresses outside the interval -- below 0 on the reverse strand) is refused with MAUVE_ERR_ARG by both _alignment entry
    points, before any kernel reads a genome through it; the consistent array goes through and equals the oracle's."""
    gs = synth.star_genomes(3, 20_000, 0.05, 7)
    ctx.set_genomes(gs)
    e = O.align(gs, O.default_params())["aln"]
    left, right, rev, off, cols = e["left"], e["right"], e["reverse"], e["col_off"], e["cols"]
    nz = np.count_nonzero(left, axis=1)
    assert (nz >= 2).any() and (nz == 1).any()           # the cases below need an interval of each kind
    noff, ncols, moved = ctx.apply_homology_alignment(left, right, rev, off, cols)
    eoff, ecols, emoved = O.homology_apply(gs, left, right, rev, off, cols)
    assert moved == emoved and np.array_equal(noff, eoff) and np.array_equal(ncols, ecols)
    multi = int(np.argmax(np.count_nonzero(left, axis=1) >= 2))
    # (1) one more residue of genome 0 than its ends allow; (2) a residue of a genome the interval does not have; (3) a bit above nseq;
    # (4) a reverse-strand interval that starts at base 1 with surplus residues: the unguarded address would be negative
    bad = []
    c1 = cols.copy(); k = off[multi] + int(np.argmax((c1[off[multi]:off[multi + 1]] & 1) == 0)); c1[k] |= 1; bad.append((left, right, rev, c1))
    single = int(np.argmax(np.count_nonzero(left, axis=1) == 1))
    other = int(np.argmax(left[single] == 0))
    c2 = cols.copy(); c2[off[single]] |= np.uint32(1 << other); bad.append((left, right, rev, c2))
    c3 = cols.copy(); c3[off[multi]] |= np.uint32(1 << 7); bad.append((left, right, rev, c3))
    l4, r4, v4 = left.copy(), right.copy(), rev.copy()
    n0 = int(right[multi, 0] - left[multi, 0] + 1)
    l4[multi, 0], r4[multi, 0], v4[multi, 0] = 1, n0 - 5, 1
    bad.append((l4, r4, v4, cols))
    for l, r, v, c in bad:
        assert not (np.array_equal(l, left) and np.array_equal(c, cols))
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.apply_homology_alignment(l, r, v, off, c)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.backbone_alignment(l, r, v, off, c)
    _same(ctx.backbone_alignment(left, right, rev, off, cols), O.backbone(left, right, rev, off, cols, island_gap=20))


def test_homology_refusals_of_a_foreign_alignment_keep_their_order(ctx):
    """mauve_apply_homology_alignment on an alignment over 2 genomes in a context of 3: the offsets are looked at first (MAUVE_ERR_ARG),
    then the genome count (MAUVE_ERR_STATE) -- before the columns are counted and before the scores are looked at, so inconsistent
    columns or positive transition scores on top of the wrong count do not change the answer"""
    ctx.set_genomes(synth.star_genomes(3, 20_000, 0.05, 7))
    left, right, rev = np.array([[1, 1]]), np.array([[4, 4]]), np.zeros((1, 2), np.int8)
    good, short, high = np.array([3, 3, 3, 3], np.uint32), np.array([3, 3, 3, 1], np.uint32), np.array([3, 3, 3, 7], np.uint32)
    for cols in (good, short, high):
        with pytest.raises(RuntimeError, match=r"\(-5\).*does not belong to the genomes"):
            ctx.apply_homology_alignment(left, right, rev, [0, 4], cols)
        with pytest.raises(RuntimeError, match=r"\(-5\).*does not belong to the genomes"):
            ctx.apply_homology_alignment(left, right, rev, [0, 4], cols, ctx.hmm_params(go_homologous=1))
        with pytest.raises(RuntimeError, match=r"\(-1\).*apply_homology: col_off must ascend from 0"):
            ctx.apply_homology_alignment(left, right, rev, [1, 4], cols)


@functools.lru_cache(maxsize=None)
def _sequence_reference():
    """the star genomes of test_inconsistent_columns_are_refused, the oracle's alignment of them and, under two HMM schemes, the oracle's
    homology pass on it: the frozen default, which moves nothing here (the columns stay where they are), and `zero`, under which 1328
    residues move (the re-split columns replace them).  Computed once, shared, never changed"""
    from tests import homology_cases as HC
    gs = synth.star_genomes(3, 20_000, 0.05, 7)
    e = O.align(gs, O.default_params())["aln"]
    hom = {}
    for scheme in ("default", "zero"):
        m, x, g, gh, gu = HC.SCHEMES[scheme]
        hom[scheme] = O.homology_apply(gs, e["left"], e["right"], e["reverse"], e["col_off"], e["cols"],
                                       O.hmm_params(match=m, mismatch=x, gap=g, go_homologous=gh, go_unrelated=gu))
    assert hom["default"][2] == 0 and hom["zero"][2] > 1000
    return gs, e, hom


@pytest.mark.parametrize("scheme", ["default", "zero"])
@pytest.mark.parametrize("resident", [True, False])
def test_stages_in_sequence_on_one_result(ctx, resident, scheme):
    """mauve_backbone -> mauve_apply_homology -> mauve_backbone -> mauve_coord_index on one result of this context, each step against the
    oracle on the fetched arrays.  resident: nothing is fetched in between, the columns are only in HBM (after a homology pass that
    moves residues: its re-split ones); else the result was fetched first and every stage that finds the columns on the host uploads
    them.  The four entry points take the result in through one front end (aln_from_context): each must get the columns the step
    before left, wherever they are.  After the fetched run the genomes are uploaded again under the host-side result: the stages that
    read no bases still take it, the homology pass refuses it."""
    from mauvealigner_amd import _lib
    from tests import homology_cases as HC
    from tests.coord_ref import CoordRef
    gs, e, hom = _sequence_reference()
    left, right, rev = e["left"], e["right"], e["reverse"]
    hoff, hcols, hmoved = hom[scheme]
    m, x, g, gh, gu = HC.SCHEMES[scheme]
    ctx.set_genomes(gs)
    a = ctx.align(_lib.default_params(), fetch=not resident)
    if not resident:
        assert np.array_equal(a["cols"], e["cols"]) and np.array_equal(a["col_off"], e["col_off"]) and np.array_equal(a["left"], left)
    _same(ctx.backbone(island_gap=20), O.backbone(left, right, rev, e["col_off"], e["cols"], island_gap=20))
    h = ctx.apply_homology(ctx.hmm_params(match=m, mismatch=x, gap=g, go_homologous=gh, go_unrelated=gu), fetch=not resident)
    assert h["n_moved"] == hmoved and h["n_cols"] == len(hcols) and h["n_iv"] == len(left)
    if not resident:
        assert np.array_equal(h["cols"], hcols) and np.array_equal(h["col_off"], hoff)
    _same(ctx.backbone(island_gap=20), O.backbone(left, right, rev, hoff, hcols, island_gap=20))
    ctx.coord_index()
    assert ctx.coord_index_size() == (3, len(left), len(hcols))
    R = CoordRef(left, right, rev, hoff, hcols)
    iv = np.repeat(np.arange(len(left), dtype=np.int64), np.diff(hoff))
    col = np.arange(len(hcols), dtype=np.int64) - hoff[iv]
    p, d = ctx.column_positions(iv, col)
    ep, ed = R.column_positions(iv, col)
    assert np.array_equal(p, ep) and np.array_equal(d, ed) and np.array_equal(d, hcols)
    seq = np.concatenate([np.full(len(g), k, np.int32) for k, g in enumerate(gs)])
    pos = np.concatenate([np.arange(1, len(g) + 1, dtype=np.int64) for g in gs])
    qi, qc = ctx.seqpos_to_column(seq, pos)
    ei, ec = R.seqpos_to_column(seq, pos)
    assert np.array_equal(qi, ei) and np.array_equal(qc, ec)
    if not resident:                                         # the same genomes again: the result, wholly on the host, stays, but its genomes count as replaced
        ctx.set_genomes(gs)
        _same(ctx.backbone(island_gap=20), O.backbone(left, right, rev, hoff, hcols, island_gap=20))
        ctx.coord_index()
        assert ctx.coord_index_size() == (3, len(left), len(hcols))
        with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
            ctx.apply_homology(fetch=False)
