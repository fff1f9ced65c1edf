"""GPU tests of the pairwise column statistics (mauve_pair_stats) against the numpy restatement of tests/pairstats_ref.py
(pinned in tests/test_pairstats_cpu.py), hand-counted literals and the rows of mauve_write_xmfa of the same context.  Integer work: every
counter must be equal."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests import pairstats_ref as PR
from tests.extract_ref import ExtractRef, xmfa_matrix
from tests.test_extract_cpu import COUNTS, load
from tests.test_gpu_coord import _disjoint_alignment
from tests.test_gpu_extract import HAND, HAND_GENOMES, _codes, _index, _n_positions, _random_genomes, _ref
from tests.test_pairstats_cpu import check_invariants, some_ranges

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024                # columns per chunk of the counting kernel (PS_UNITS = 16 words of 64 columns, pairstat_dev.hip): where a
#                             workgroup's walk starts inside a range it looks back for the run state


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _both_modes(ctx, E, pairs=None, ranges=None):
    """totals and per-range records of the device against the restatement; -> the per-range records"""
    want = PR.pair_stats(E, pairs, ranges, per_range=True)
    per = ctx.pair_stats(pairs, ranges, per_range=True)
    assert per.shape == want.shape and per.dtype == np.int64
    assert np.array_equal(per, want), np.argwhere(per != want)[:5]
    tot = ctx.pair_stats(pairs, ranges)
    assert tot.shape == want.shape[1:] and np.array_equal(tot, want.sum(axis=0)), np.argwhere(tot != want.sum(axis=0))[:5]
    return per


def test_pair_stats_hand_case(ctx):
    """the alignment of test_extract_hand_case: rows ACGTACGTACGTACGTACGT / CCCCCGGGGG-----TTTTT / TTACGTACGTAAAACCCGGT"""
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    st = ctx.pair_stats()
    assert st.shape == (3, 32)
    s01, s02, s12 = st
    assert s01[:25].sum() == 15 and s01[PR.DIAG].sum() == 4 and s01[25:].tolist() == [5, 0, 1, 0, 0, 0, 0]
    assert s12[:25].sum() == 15 and s12[PR.DIAG].sum() == 3 and s12[25:].tolist() == [0, 5, 0, 1, 0, 0, 0]
    assert s02[:25].sum() == 20 and s02[25:].tolist() == [0] * 7
    assert s01[:25].reshape(5, 5)[:4, :4].tolist() == [[0, 2, 1, 1], [0, 1, 2, 1], [0, 1, 1, 1], [0, 1, 1, 2]]
    # the ordered pair (1, 0): the transposed table, the one-sided slots swapped
    s10 = ctx.pair_stats(([1], [0]))[0]
    assert np.array_equal(s10[:25].reshape(5, 5), s01[:25].reshape(5, 5).T) and s10[25:].tolist() == [0, 5, 0, 1, 0, 0, 0]
    # a window, and the gap run of genome 1 (columns 10..14) cut by a range boundary: each range opens a run of its own
    w = ctx.pair_stats(([0], [1]), ([0], [8], [6]))[0]
    assert w[:25].sum() == 2 and w[25:].tolist() == [4, 0, 1, 0, 0, 0, 0]
    per = ctx.pair_stats(([0], [1]), ([0, 0], [8, 12], [4, 6]), per_range=True)
    assert per[0, 0, 25:30].tolist() == [2, 0, 1, 0, 0] and per[1, 0, 25:30].tolist() == [3, 0, 1, 0, 0]
    assert ctx.pair_stats(([0], [1]), ([0, 0], [8, 12], [4, 6]))[0, 25:30].tolist() == [5, 0, 2, 0, 0]
    E = _ref(HAND, gs)
    _both_modes(ctx, E)
    _both_modes(ctx, E, ([2, 1, 0], [0, 2, 1]), ([0, 0, 0], [0, 19, 3], [20, 1, 0]))


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_pair_stats_golden_fixtures(ctx, name):
    """set_genomes + coord_index_alignment on the committed fixtures: all pairs over whole intervals, then 40 random ranges with empty
    and overlapping ones, then a chosen list of ordered pairs with a duplicate; totals and per-range"""
    a, gs = load(name)
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    per = _both_modes(ctx, E)
    up = PR.all_pairs(N)
    assert check_invariants(per, np.diff(a["col_off"]), up) == 0
    rng = np.random.default_rng(len(name))
    ranges = some_ranges(a, rng)
    _both_modes(ctx, E, None, ranges)
    chosen = ([N - 1, 0, 1, N - 1, 0], [0, N - 1, 0, 0, 1])
    per = _both_modes(ctx, E, chosen, ranges)
    assert np.array_equal(per[:, 0], per[:, 3])                                           # the duplicate
    assert check_invariants(per[:, [0, 1, 2, 4]], ranges[2], ([N - 1, 0, 1, 0], [0, N - 1, 0, 1])) == (4 if N > 2 else 2)
    if name == "g2x2k":
        s = ctx.pair_stats()[0]
        assert (int(s[:25].sum()), int(s[PR.DIAG].sum()), s[25:30].tolist()) == (1991, 1915, [10, 15, 5, 7, 0])


@pytest.mark.parametrize("run", ["c3_align", "c4_progressive", "c3_ambiguous"])
def test_pair_stats_of_the_resident_alignment(ctx, run):
    """mauve_align / mauve_progressive_align, mauve_coord_index, then the statistics equal the restatement, and the identity matrix equals
    the one counted in numpy on the rows of mauve_write_xmfa of the same context (the host writer: independent of the new code); over the
    backbone segments every genome is in, it is the backbone identity matrix"""
    from mauvealigner_amd import _lib
    inv = None
    if run == "c4_progressive":
        gs = synth.make_config("C4", scale=0.02)
        ctx.set_genomes(gs)
        a = ctx.progressive_align(_lib.default_progressive_params(), want_xmfa=True)
        assert np.any((np.count_nonzero(a["left"], axis=1) > 1) & (np.count_nonzero(a["left"], axis=1) < len(gs)))       # intervals with absent genomes
    else:
        gs = synth.make_config("C3", scale=0.01)
        if run == "c3_ambiguous":
            rng = np.random.default_rng(5)
            inv = [_n_positions(rng, len(g), 0.003) for g in gs]
            inv[2] = None
            ctx.set_genomes(gs, invalid=inv)
        else:
            ctx.set_genomes(gs)
        a = ctx.align(_lib.default_params(), want_xmfa=True)
    N = len(gs)
    ctx.coord_index()
    E = _ref(a, gs, inv)
    per = _both_modes(ctx, E)
    # the identity matrix from the text the host writer printed
    rows = xmfa_matrix(a["xmfa"], N)
    up = PR.all_pairs(N)
    rid = np.repeat(np.arange(len(a["left"]), dtype=np.int64), np.diff(a["col_off"]))
    from_text = PR.count_rows(PR.letter_codes(rows), rid, len(a["left"]), up)
    assert np.array_equal(per, from_text)
    ident = _lib.pair_stats_identity(ctx.pair_stats())
    x, y = PR.letter_codes(rows)[up[0]], PR.letter_codes(rows)[up[1]]
    both = (x != 5) & (y != 5)
    assert np.array_equal(ident, (both & (x == y)).sum(axis=1) / both.sum(axis=1)) and np.all((ident > 0) & (ident < 1))
    if inv is not None:
        # an ambiguous base shows as N on both strands: the fifth row of the letter table of (g, other) in forward and in reverse intervals
        seen = 0
        for g in range(N):
            rev = a["reverse"][:, g] != 0
            if inv[g] is None or not np.any(rev):
                continue
            n_rows = ctx.pair_stats(([g], [(g + 1) % N]), per_range=True)[:, 0, 20:25].sum(axis=1)
            assert np.any(n_rows[rev] > 0) and np.any(n_rows[~rev] > 0), g
            seen += 1
        assert seen > 0
        assert not np.any(ctx.pair_stats(([2], [0]))[0, 20:25])
    # backbone ranges: the segments every genome is in
    full = (1 << N) - 1
    b = ctx.backbone(island_gap=20)
    m = b["seg_mask"] == full
    assert np.any(m)
    ranges = (b["seg_iv"][m], b["seg_col"][m], b["seg_len"][m])
    ctx.coord_index()
    bb = ctx.pair_stats(ranges=ranges)
    assert np.array_equal(bb, PR.pair_stats(E, None, ranges))
    bb_ident = _lib.pair_stats_identity(bb)
    assert np.array_equal(bb_ident, PR.identity(bb)) and np.all((bb_ident > 0) & (bb_ident < 1))


@pytest.mark.parametrize("N", [2, 5, 17, 32])
def test_pair_stats_random_alignments(ctx, N):
    """random alignments with random genomes, 1 / 10 / 136 / 496 pairs (above 256 the pairs are strided over the workgroup); the ranges
    start and end on and around multiples of 64 (a record word), 448 (a block) and CHUNK"""
    rng = np.random.default_rng(6000 + N)
    n_iv, length = {2: (10, 24), 5: (5, 10), 17: (4, 8), 32: (4, 8)}[N]                  # ... of 9 000 to 21 000 columns
    a = _disjoint_alignment(rng, N, n_iv=n_iv, length=length)
    gs = _random_genomes(rng, a)
    inv = [_n_positions(rng, len(g), 0.02) if g_i % 2 else None for g_i, g in enumerate(gs)]
    ctx.set_genomes(gs, invalid=inv)
    _index(ctx, a)
    E = _ref(a, gs, inv)
    n_cols = len(a["cols"])
    assert 8 * CHUNK < n_cols < 22000
    per = _both_modes(ctx, E)
    assert per.shape[1] == N * (N - 1) // 2 and np.any(per[:, per.shape[1] // 2:, :25])
    edge = np.unique(np.concatenate([np.arange(0, n_cols, s)[:, None] + np.array([-1, 0, 1]) for s in (64, 448, CHUNK)], axis=None))
    edge = edge[(edge >= 0) & (edge < n_cols)]
    n_r = 300 if N <= 5 else 40
    x0 = rng.choice(edge, n_r)
    x1 = rng.choice(edge, n_r)
    x0, x1 = np.minimum(x0, x1), np.maximum(x0, x1) + 1
    iv = np.searchsorted(a["col_off"], x0, side="right") - 1
    x1 = np.minimum(x1, a["col_off"][iv + 1])                                             # a range stays inside its interval
    ranges = (iv, x0 - a["col_off"][iv], x1 - x0)
    assert np.any(ranges[2] > 2 * CHUNK)
    _both_modes(ctx, E, None, ranges)


def _runs_alignment():
    """one interval of 20 000 columns, three genomes, long gap runs and long stretches of empty columns -> (alignment, genomes)"""
    n = 20000
    cols = np.ones(n, np.uint32)                                                          # genome 0 everywhere
    cols[:100] |= 2
    cols[15000:] |= 2                                                                     # genome 1: absent from 100 to 14 999 ...
    cols[12000] |= 2                                                                      # ... but for one column
    cols[:50] |= 4
    cols[[2000, 9000, 12000, 14000]] |= 4                                                 # genome 2: four lone columns
    cnt = [int(np.count_nonzero(cols >> g & 1)) for g in range(3)]
    a = dict(left=np.array([[1, 1, 1]]), right=np.array([cnt]), reverse=np.array([[0, 1, 0]], np.int8), col_off=np.array([0, n]), cols=cols)
    rng = np.random.default_rng(77)
    return a, [rng.integers(0, 4, c + 3, dtype=np.uint8) for c in cnt]


def test_pair_stats_runs_across_chunks(ctx):
    """one interval of 20 000 columns, three genomes: gap runs that span many chunks of the counting kernel, columns of a run with chunks
    of empty columns between them, a column with two residues in between, and ranges that cut a run"""
    a, gs = _runs_alignment()
    n = 20000
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)

    def one(pair, col, ln):
        s = ctx.pair_stats(([pair[0]], [pair[1]]), ([0], [col], [ln]))[0]
        assert np.array_equal(s, PR.pair_stats(E, ([pair[0]], [pair[1]]), ([0], [col], [ln]))[0])
        return s[25:30].tolist()

    assert one((0, 1), 50, 11950) == [11900, 0, 1, 0, 0]                                  # one only_a run over eleven chunks
    assert one((1, 0), 50, 11950) == [0, 11900, 0, 1, 0]
    assert one((1, 2), 1500, 8500) == [0, 2, 0, 1, 8498]                                  # 2000 and 9000, chunks of `neither` between: one run
    assert one((2, 1), 1500, 8500) == [2, 0, 1, 0, 8498]
    assert one((1, 2), 8000, 6500) == [0, 2, 0, 2, 6497]                                  # 9000, both at 12000, 14000: two runs
    assert one((1, 2), 2001, 7499) == [0, 1, 0, 1, 7498]                                  # 9000 alone: its predecessor lies outside the range
    for cut in (6000, CHUNK * 5, CHUNK * 5 + 1, 6017):                                    # a range boundary inside the run opens a new run
        per = ctx.pair_stats(([0], [1]), ([0, 0], [50, cut], [cut - 50, 12000 - cut]), per_range=True)
        assert per[:, 0, 25:30].tolist() == [[cut - 100, 0, 1, 0, 0], [12000 - cut, 0, 1, 0, 0]]
        assert ctx.pair_stats(([0], [1]), ([0, 0], [50, cut], [cut - 50, 12000 - cut]))[0, 25:30].tolist() == [11900, 0, 2, 0, 0]
    ranges = ([0] * 6, [0, 50, 1500, 8000, 2001, 13999], [n, 11950, 8500, 6500, 7499, 3])
    per = _both_modes(ctx, E, ([0, 1, 2, 0, 1, 2], [1, 2, 0, 2, 0, 1]), ranges)
    assert per[0, 0, 25:30].tolist() == [14899, 0, 2, 0, 0]


def test_pair_stats_many_short_ranges(ctx):
    """3000 ranges of 0 to 3 columns, overlapping and in arbitrary order: many ranges fall into one 64-column word; per-range records, and
    their sum is the totals call"""
    a, gs = load("g4x6k_repeat")
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    rng = np.random.default_rng(31)
    lens = np.diff(a["col_off"])
    r_iv = rng.integers(0, len(lens), 3000)
    r_len = np.minimum(rng.integers(0, 4, 3000), lens[r_iv])
    r_col = (rng.random(3000) * (lens[r_iv] - r_len + 1)).astype(np.int64)
    per = _both_modes(ctx, E, None, (r_iv, r_col, r_len))
    assert np.array_equal(per.sum(axis=0), ctx.pair_stats(ranges=(r_iv, r_col, r_len)))
    assert np.array_equal(per[..., :27].sum(axis=-1) + per[..., 29], np.broadcast_to(r_len[:, None], per.shape[:2]))
    assert np.any(r_len == 0) and np.any(per[..., 27] > 0)


MAX_SPANS = 1024            # PS_MAX_SPANS: the counting kernel has at most that many workgroups; above PS_MAX_SPANS * PS_UNITS units of work
UNITS = CHUNK // 64         # (PS_UNITS units = 64-column words of one range per chunk) a workgroup walks a span of several chunks


@pytest.mark.parametrize("which", ["runs", "random"])
def test_pair_stats_spans_of_several_chunks(ctx, which):
    """more than PS_MAX_SPANS * PS_UNITS units with at most 256 pairs: every workgroup takes a span of two or three chunks, and a thread
    keeps its pair's counters, its current range and the run state from chunk to chunk, as every call of production size does.  Thousands
    of overlapping ranges of up to four words, so that ranges straddle the chunk boundaries inside a span, and among them long ranges that
    cover many chunks and spans with a gap run open (runs: the alignment of test_pair_stats_runs_across_chunks; random: five genomes with
    ambiguous bases); totals and per-range records"""
    if which == "runs":
        a, gs = _runs_alignment()
        inv = None
        n_short, pairs = 14000, ([0, 1, 2, 0, 1, 2], [1, 2, 0, 2, 0, 1])
        long_ranges = ([0] * 6, [0, 50, 1500, 8000, 2001, 13999], [20000, 11950, 8500, 6500, 7499, 3])
    else:
        rng = np.random.default_rng(6105)
        a = _disjoint_alignment(rng, 5, n_iv=5, length=10)
        gs = _random_genomes(rng, a)
        inv = [_n_positions(rng, len(g), 0.02) if g_i % 2 else None for g_i, g in enumerate(gs)]
        n_short, pairs = 9000, None
        lens = np.diff(a["col_off"])
        long_ranges = (np.arange(len(lens)), lens // 3, lens - lens // 3)
    assert len(a["cols"]) < 22000
    rng = np.random.default_rng(len(which))
    lens = np.diff(a["col_off"])
    r_iv = rng.integers(0, len(lens), n_short)
    r_len = np.minimum(rng.integers(0, 201, n_short), lens[r_iv])
    r_col = (rng.random(n_short) * (lens[r_iv] - r_len + 1)).astype(np.int64)
    at = np.sort(rng.integers(0, n_short, len(long_ranges[0])))                           # the long ranges somewhere among the short ones
    r_iv, r_col, r_len = (np.insert(s, at, np.asarray(l, np.int64)) for s, l in zip((r_iv, r_col, r_len), long_ranges))
    x0 = a["col_off"][r_iv] + r_col
    units = int(np.where(r_len > 0, (x0 + r_len - 1) // 64 - x0 // 64 + 1, 0).sum())
    assert units > (2 if which == "runs" else 1) * MAX_SPANS * UNITS                      # spans of three chunks, of two
    ctx.set_genomes(gs, invalid=inv)
    _index(ctx, a)
    E = _ref(a, gs, inv)
    per = _both_modes(ctx, E, pairs, (r_iv, r_col, r_len))
    assert np.any(per[..., 27] > 0) and np.any(per[..., 28] > 0) and np.any(r_len == 0)
    assert np.array_equal(per[..., :27].sum(axis=-1) + per[..., 29], np.broadcast_to(r_len[:, None], per.shape[:2]))
    if which == "runs":                                                                   # the literals of test_pair_stats_runs_across_chunks
        assert per[at[0], 0, 25:30].tolist() == [14899, 0, 2, 0, 0] and per[at[1] + 1, 0, 25:30].tolist() == [11900, 0, 1, 0, 0]
        assert per[at[2] + 2, 1, 25:30].tolist() == [0, 2, 0, 1, 8498] and per[at[3] + 3, 1, 25:30].tolist() == [0, 2, 0, 2, 6497]


def test_pair_stats_buffers_and_state(ctx):
    """page-locked results are copied directly, pageable ones through the staging; no range at all; two calls give the same bytes; the
    extract selection in force is neither needed nor disturbed"""
    from mauvealigner_amd import _lib
    a, gs = load("g5x3k_unique")
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    rng = np.random.default_rng(8)
    ranges = some_ranges(a, rng)
    for per_range in (False, True):
        want = PR.pair_stats(E, None, ranges, per_range=per_range)
        for pinned in (True, False):
            out = _lib.pinned_empty(want.shape, np.int64) if pinned else np.empty(want.shape, np.int64)
            out[...] = -1
            got = ctx.pair_stats(ranges=ranges, per_range=per_range, out=out)
            assert got is out and np.array_equal(got, want), (per_range, pinned)
        assert ctx.pair_stats(ranges=ranges, per_range=per_range).tobytes() == want.tobytes() == ctx.pair_stats(ranges=ranges, per_range=per_range).tobytes()
    none = (np.zeros(0, np.int64),) * 3
    z = ctx.pair_stats(ranges=none)
    assert z.shape == (N * (N - 1) // 2, 32) and not np.any(z)
    assert ctx.pair_stats(ranges=none, per_range=True).shape == (0, N * (N - 1) // 2, 32)
    assert not np.any(ctx.pair_stats(ranges=([0, 1], [3, 0], [0, 0]), per_range=True))
    # a selection made before the statistics is still there after them
    ns = ctx.extract_select(keep=[4, 1], polymorphic=True)
    want = E.extract(keep=[4, 1], polymorphic=True)
    assert ns == want[0].shape[1] > 0
    st = ctx.pair_stats(([4], [1]), ranges)
    assert np.array_equal(st, PR.pair_stats(E, ([4], [1]), ranges))
    got = ctx.extract_fetch()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_pair_stats_errors_and_state(ctx):
    """every refusal of S16, once each; none of them reaches a kernel with an index it could follow out of bounds; a refused call leaves
    the index usable"""
    from mauvealigner_amd import _lib
    gs = [_codes(s) for s in HAND_GENOMES]
    c2 = _lib.Context(0)
    try:
        st = np.zeros((3, 32), np.int64)
        assert c2.L.mauve_pair_stats(c2.h, C.c_int64(0), None, None, C.c_int64(0), None, None, None, 0, _lib._p(st, C.c_int64)) == -5       # no index
        c2.set_genomes(gs[:2])
        _index(c2, HAND)                                                                   # an index of 3 genomes, a context of 2
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.pair_stats()
        c2.set_genomes(gs)                                                                 # ... built before the last upload
        with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
            c2.pair_stats()
        assert c2.column_positions([0], [19])[0].tolist() == [[20, 115, -201]]
        _index(c2, HAND)
        assert c2.pair_stats()[0, 25] == 5
    finally:
        c2.close()
    ctx.set_genomes(gs)
    two = dict(left=np.array([[1, 101, 201], [21, 0, 221]]), right=np.array([[20, 115, 220], [22, 0, 222]]), reverse=np.array([[0, 0, 1], [0, 0, 0]], np.int8),
               col_off=np.array([0, 20, 22]), cols=np.concatenate([HAND["cols"], np.array([5, 5], np.uint32)]))
    _index(ctx, two)

    def still_there():
        assert ctx.column_positions([1], [1])[0].tolist() == [[22, 0, 222]]

    assert ctx.pair_stats(ranges=([1, 0], [0, 18], [2, 2]))[:, 25:30].tolist() == [[2, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 2, 0, 1, 0]]
    for ranges in (([2], [0], [1]), ([-1], [0], [1]), ([0], [-1], [1]), ([0], [0], [-1]), ([0], [0], [21]), ([0], [21], [0]), ([1], [1], [2]),
                   ([0, 1, 0], [0, 3, 0], [20, 0, 20])):
        for per_range in (False, True):
            with pytest.raises(RuntimeError, match=r"\(-1\)"):
                ctx.pair_stats(ranges=ranges, per_range=per_range)
        still_there()
    for pairs in (([1], [1]), ([0, 2], [1, 2]), ([3], [0]), ([0], [3]), ([-1], [0]), ([0], [-1]), ([], []), ([0] * 1025, [1] * 1025)):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.pair_stats(pairs)
        still_there()
    assert ctx.pair_stats(([0] * 1024, [1] * 1024)).shape == (1024, 32)
    # the record limit: 1024 pairs x 16 385 ranges
    many = (np.zeros(16385, np.int64), np.zeros(16385, np.int64), np.ones(16385, np.int64))
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        ctx.pair_stats(([0] * 1024, [1] * 1024), many, per_range=True)
    still_there()
    # with a result array passed, the library's refusal is still what the caller sees, not a word about the array's shape
    small = np.empty((1, 32), np.int64)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        ctx.pair_stats(([0] * 1024, [1] * 1024), many, per_range=True, out=small)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.pair_stats(([0] * 1025, [1] * 1025), out=small)
    with pytest.raises(ValueError):
        ctx.pair_stats(([0], [1]), out=np.empty((2, 32), np.int64))
    still_there()
    assert ctx.pair_stats(([0] * 1024, [1] * 1024), many)[1023, 1] == 16385                # the totals of the same request are 1024 records
    # an interval of the index that ends beyond the resident genome
    ctx.set_genomes([gs[0], gs[1][:114], gs[2]])
    _index(ctx, two)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.pair_stats()
    still_there()
    ctx.set_genomes(gs)
    _index(ctx, two)
    assert ctx.pair_stats().shape == (3, 32)


def test_pair_statistics_mirror():
    """mems::HipPairStatistics (include/libMems/PairStatistics.h) over IntervalLists read from committed golden XMFAs, with the genomes of
    the fixture: equal to the host mems::IdentityMatrix and to computeSPScore over every interval's rows (tests/cpp/pairstats_test.cpp)"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "pairstats_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pairstats_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        for name in ("g3x5k_inv", "g4x3k_tree"):
            a, gs = load(name)
            mfa = os.path.join(td, name + ".mfa")
            with open(mfa, "w") as f:
                for g, s in enumerate(gs):
                    f.write(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()))
            r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", name + ".xmfa"), mfa], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
