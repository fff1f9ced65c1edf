"""GPU tests of the excursions of the column scores (mauve_excursions_pairs, mauve_excursions_core, mauve_excursions_fetch)
against the restatement of tests/excursion_ref.py (pinned in tests/test_excursion_cpu.py).  Integer work: every array -- heights, end
columns, stream offsets, tails -- must be equal."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests import excursion_ref as XR
from tests.test_excursion_cpu import EXAMPLE, EXAMPLE_GENOMES, SIMPLE, scoring_of
from tests.test_extract_cpu import COUNTS, load
from tests.test_gpu_extract import HAND, HAND_GENOMES, _codes, _index, _n_positions, _ref
from tests.test_pairstats_cpu import some_ranges

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 512                    # MAUVE_EXCURSION_CHUNK: columns per chunk, counted from the 64-column word that holds a range's first column
MAX_GROUPS = 2048           # EXC_MAX_GROUPS (excursion_dev.hip): workgroups of a walk at the most; above it a workgroup takes several chunks
SKEW = [[5, -1, -2, -3], [-4, 6, -5, -6], [-7, -8, 7, -9], [-10, -11, -12, 8]]


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    assert _lib.EXCURSION_CHUNK == CH
    c = _lib.Context(0)
    yield c
    c.close()


def _default():
    from mauvealigner_amd import _lib
    d = _lib.default_scoring()
    return [list(r) for r in d.matrix], d.gap_open, d.gap_extend


def _same(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want.arrays())):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5])


def _pairs(ctx, E, pairs=None, ranges=None, sc=None):
    """the pair streams of the device against the restatement -> the restatement's result"""
    m, go, ge = _default() if sc is None else sc
    want = XR.excursions_pairs(E, m, go, ge, pairs, ranges)
    n = ctx.excursions_pairs(pairs, ranges, None if sc is None else scoring_of(*sc))
    assert n == len(want.height)
    _same(ctx.excursions_fetch(), want, "pairs")
    return want


def _core(ctx, E, groups=None, ranges=None, sc=None):
    m, go, ge = _default() if sc is None else sc
    want = XR.excursions_core(E, m, groups, ranges)
    n = ctx.excursions_core(groups, ranges, None if sc is None else scoring_of(*sc))
    assert n == len(want.height)
    _same(ctx.excursions_fetch(), want, "core")
    return want


def test_excursions_worked_example_and_hand_case(ctx):
    """the example of S18 -- mismatch, mismatch, match, mismatch, match under 2 / -1: one record of height 2 at column 4, the return to
    zero at column 2 ends nothing -- and the alignment of test_extract_hand_case, whose gap run a range boundary cuts"""
    ctx.set_genomes(EXAMPLE_GENOMES)
    _index(ctx, EXAMPLE)
    sc = scoring_of(*SIMPLE)
    assert ctx.excursions_pairs(scoring=sc) == 1
    h, e, off, tail = ctx.excursions_fetch()
    assert (h.tolist(), e.tolist(), off.tolist(), tail.tolist()) == ([2], [4], [0, 1], [[0, 0]])
    assert ctx.excursions_core(scoring=sc) == 1
    h, e, off, tail = ctx.excursions_fetch()
    assert (h.tolist(), e.tolist(), off.tolist(), tail.tolist()) == ([2], [4], [0, 1], [[0, 0]])
    assert ctx.excursions_pairs(ranges=([0], [0], [4]), scoring=sc) == 0                       # cut before the end: the tail holds it
    assert ctx.excursions_fetch()[3].tolist() == [[1, 2]]
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    E = _ref(HAND, gs)
    # rows ACGTACGTACGTACGTACGT / CCCCCGGGGG-----TTTTT: the run of columns 10..14 whole costs open + 4 extend, cut at 12 two opens
    go, ge = SIMPLE[1], SIMPLE[2]
    ctx.excursions_pairs(([0], [1]), ([0, 0, 0], [10, 10, 12], [5, 2, 3]), sc)
    assert ctx.excursions_fetch()[3].tolist() == [[-go - 4 * ge] * 2, [-go - ge] * 2, [-go - 2 * ge] * 2]
    for s in (None, SIMPLE, (SKEW, -17, -3)):
        _pairs(ctx, E, sc=s)
        _pairs(ctx, E, ([2, 1, 0, 1], [0, 2, 1, 0]), ([0, 0, 0, 0], [0, 19, 3, 8], [20, 1, 0, 6]), sc=s)
        _core(ctx, E, sc=s)
        _core(ctx, E, [7, 5, [1, 2]], ([0, 0, 0], [0, 12, 3], [20, 8, 0]), sc=s)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_excursions_golden_fixtures(ctx, name):
    """set_genomes + coord_index_alignment on the committed fixtures: all pairs, a chosen ordered pair list with a duplicate and a reversed
    pair, 40 random ranges with empty and overlapping ones, an asymmetric matrix; the groups {all}, {0, N-1} and one whose genome is absent
    from some interval"""
    a, gs = load(name)
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    whole = _pairs(ctx, E)
    assert len(whole.stream_off) == len(a["left"]) * N * (N - 1) // 2 + 1
    rng = np.random.default_rng(len(name))
    ranges = some_ranges(a, rng)
    _pairs(ctx, E, None, ranges)
    chosen = ([N - 1, 0, 1, N - 1, 0], [0, N - 1, 0, 0, 1])
    w = _pairs(ctx, E, chosen)
    hs = [[w.height[w.stream_off[r * 5 + k]:w.stream_off[r * 5 + k + 1]].tolist() for r in range(len(a["left"]))] for k in range(5)]
    assert hs[0] == hs[3] and hs[0] == hs[1]                  # the duplicate; the reversed pair under a symmetric matrix
    if N > 2:
        assert hs[2] == hs[4] and hs[2] != hs[0]
    _pairs(ctx, E, chosen, ranges, sc=(SKEW, -17, -3))
    _pairs(ctx, E, None, None, sc=(SKEW, -17, -3))
    absent = np.flatnonzero(np.any(a["left"] == 0, axis=0))
    g_abs = int(absent[0]) if len(absent) else N - 1
    groups = [(1 << N) - 1, [0, N - 1], sorted({g_abs, (g_abs + 1) % N})]
    _core(ctx, E)
    c = _core(ctx, E, groups)
    _core(ctx, E, groups, ranges, sc=(SKEW, -17, -3))
    if len(absent):                                           # absent from an interval: no stream there
        miss = np.flatnonzero(a["left"][:, g_abs] == 0)
        assert np.all(np.diff(c.stream_off)[miss * 3 + 2] == 0) and np.all(c.tail[miss * 3 + 2] == 0)


def _built(kinds, three):
    """an interval whose pair (0, 1) shows the given kinds, column by column -- M: A/A, X: A/C, Z: A/G, a: only genome 0, b: only genome 1,
    n: neither (genome 2 alone; three genomes only) -- -> (alignment, genomes); genome 2 has a residue in every column"""
    k = np.frombuffer(kinds.encode(), np.uint8)
    in0 = np.isin(k, np.frombuffer(b"MXZa", np.uint8))
    in1 = np.isin(k, np.frombuffer(b"MXZb", np.uint8))
    cols = in0.astype(np.uint32) | in1.astype(np.uint32) << 1
    if three:
        cols |= 4
    assert np.all(cols != 0)
    lut = np.zeros(256, np.uint8)
    lut[ord("X")], lut[ord("Z")] = 1, 2
    g0 = np.zeros(int(in0.sum()) + 2, np.uint8)
    g1 = np.concatenate([lut[k[in1]], np.zeros(2, np.uint8)])
    gs = [g0, g1] + ([np.random.default_rng(3).integers(0, 4, len(k) + 2, dtype=np.uint8)] if three else [])
    N = len(gs)
    cnt = [int(in0.sum()), int(in1.sum()), len(k)][:N]
    a = dict(left=np.ones((1, N), np.int64), right=np.array([cnt], np.int64), reverse=np.zeros((1, N), np.int8), col_off=np.array([0, len(k)]), cols=cols)
    return a, gs


# under BUILT a match is -2 for v, a mismatch A/C +1, A/G 0, a gap column +3 where it opens a run and +1 where it extends one
BUILT = ([[2, -1, 0, -5], [-3, 2, -4, -6], [1, -7, 2, -8], [-9, -2, -3, 2]], -3, -1)


def _designed(three):
    """the kinds of the chunk-edge interval; `three` puts `neither` columns where two genomes can have none"""
    n = "n" if three else "Z"
    s = "M" * 10 + "X" * 100 + "M" * 40 + "M" * 9 + "X" + "M"           # x = 100, then down to 1 at column 160, h = 100
    s += "Z" * (4 * CH - len(s))                                          # ... held through the chunks 1, 2, 3
    assert len(s) == 4 * CH
    s += "M"                                                              # the first column of chunk 4 ends it: (100, 4 CH)
    s += "Z" * (5 * CH - 3 - len(s)) + "XX" + "M"                         # x = 2, back to exactly 0 on the last column of chunk 4
    assert len(s) == 5 * CH
    s += "XXX" + "MM"                                                     # h carried over the return to zero: (3, 5 CH + 4)
    s += "Z" * (3000 - len(s)) + "a" * 8                                  # a run of genome 0 opens at 3000 ...
    s += n * (3136 - len(s))                                              # ... two whole words of `neither`, the chunk boundary 6 CH between them
    s += "a" * 5 + "b" * 3 + "X" * 21                                     # ... and goes on: extends, then a run of genome 1 opens
    s += n * (8 * CH + 100 - len(s))                                      # chunk 7 holds no stream column
    s += "M" * 30 + "Z" * 50 + "X" * 5                                    # the excursion ends behind it (the 21st match); the stream ends above zero
    return s


@pytest.mark.parametrize("three", [False, True])
def test_excursions_chunk_edges(ctx, three):
    """a built alignment of two / three genomes: an excursion that runs through three whole chunks without an emission and ends on the
    first column of a chunk (x and h both carried), an exact return to zero on a chunk's last column, a gap run across a chunk boundary
    with whole words of `neither` columns in between, a chunk without a stream column in mid-stream, a stream without a column; ranges that
    start off the multiples of 64 with 1, 63, 64, 65, CH - 1, CH, CH + 1 and 3 CH + 17 columns"""
    kinds = _designed(three)
    a, gs = _built(kinds, three)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    w = _pairs(ctx, E, ([0], [1]), sc=BUILT)
    assert w.height[:2].tolist() == [100, 3] and w.end_col[:2].tolist() == [4 * CH, 5 * CH + 4]
    if three:
        # the run of genome 0: open + 7 extends, then 5 extends behind the empty words; genome 1: open + 2 extends; 21 mismatches
        assert w.height[2] == 3 + 7 + 5 + 3 + 2 + 21 and w.end_col[2] == 8 * CH + 100 + 20 and len(w.height) == 3
    assert w.tail.tolist() == [[5, 5]]
    lens = [1, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 17]
    starts = [37, 100, 4 * CH - 70, 2700]
    r_col = [s for s in starts for _ in lens] + [7 * CH + 10, 0, 5 * CH - 5]
    r_len = [n for _ in starts for n in lens] + [300, len(kinds), 5]
    ranges = ([0] * len(r_col), r_col, r_len)
    w = _pairs(ctx, E, None, ranges, sc=BUILT)
    P = (w.stream_off.shape[0] - 1) // len(r_col)
    if three:
        k = (len(r_col) - 3) * P                                          # the range inside the empty chunk: pair (0, 1) has no column
        assert w.stream_off[k] == w.stream_off[k + 1] and w.tail[k].tolist() == [0, 0]
    _pairs(ctx, E, ([1, 0], [0, 1]), ranges)
    _core(ctx, E, None, ranges, sc=BUILT)
    _core(ctx, E, [3], None, sc=BUILT)


@pytest.mark.parametrize("N", [2, 3])
def test_excursions_random_built_alignments(ctx, N):
    """random kinds in random runs over about 20 000 columns, scored so that x rises and falls across many chunks; whole, and ranges of the
    edge lengths at random starts"""
    rng = np.random.default_rng(1800 + N)
    parts = []
    while sum(len(p) for p in parts) < 20000:
        kind = rng.choice(list("MXZab" + ("n" if N == 3 else "")), p=[.5, .3, .05, .075, .075] if N == 2 else [.46, .3, .05, .07, .07, .05])
        parts.append(kind * int(rng.choice([1, 2, 3, 5, 40, 70, 300], p=[.3, .2, .15, .15, .1, .07, .03])))
    kinds = "".join(parts)
    a, gs = _built(kinds, N == 3)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    w = _pairs(ctx, E, sc=BUILT)
    assert len(w.height) > 20 and w.height.max() > 100
    lens = np.array([1, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 17] * 6)
    r_col = rng.integers(0, len(kinds) - lens)
    ranges = (np.zeros(len(lens), np.int64), r_col, lens)
    assert np.any(r_col % 64 != 0)
    w = _pairs(ctx, E, None, ranges, sc=BUILT)
    assert np.any(w.tail[:, 0] > 0) and np.any(w.tail[:, 1] > w.tail[:, 0])
    _core(ctx, E, None, ranges, sc=BUILT)
    _pairs(ctx, E, None, ranges)


def test_excursions_more_chunks_than_workgroups(ctx):
    """250 overlapping ranges over the chunk-edge interval: more chunks than the walk's largest grid, so a workgroup takes several"""
    kinds = _designed(True)
    a, gs = _built(kinds, True)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    rng = np.random.default_rng(9)
    n_r = 250
    r_col = rng.integers(0, 200, n_r)
    r_len = len(kinds) - r_col - rng.integers(0, 100, n_r)
    assert int(np.sum((r_col + r_len - 1) // CH - r_col // CH + 1)) > MAX_GROUPS
    ranges = (np.zeros(n_r, np.int64), r_col, r_len)
    w = _pairs(ctx, E, None, ranges, sc=BUILT)
    assert len(w.height) > 3 * n_r
    _core(ctx, E, [3, 7, 6], ranges, sc=BUILT)


def test_excursions_ambiguous_bases(ctx):
    """N scores as A, on forward and on reverse intervals"""
    a, gs = load("g3x5k_inv")
    assert np.any(a["reverse"] != 0) and np.any(a["reverse"] == 0)
    rng = np.random.default_rng(18)
    inv = [_n_positions(rng, len(g), 0.05) for g in gs]
    inv[1] = None
    ctx.set_genomes(gs, invalid=inv)
    _index(ctx, a)
    E = _ref(a, gs, inv)
    plain = XR.excursions_pairs(_ref(a, gs), *_default())
    w = _pairs(ctx, E)
    assert not np.array_equal(w.height, plain.height)
    _pairs(ctx, E, sc=(SKEW, -17, -3))
    _core(ctx, E, [7, 5], sc=(SKEW, -17, -3))


@pytest.mark.parametrize("run", ["c3_align", "c4_progressive"])
def test_excursions_of_the_resident_alignment(ctx, run):
    """mauve_align of C3 at 0.01 / mauve_progressive_align of C4 at 0.02, mauve_coord_index, then both kinds of stream"""
    from mauvealigner_amd import _lib
    if run == "c4_progressive":
        gs = synth.make_config("C4", scale=0.02)
        ctx.set_genomes(gs)
        a = ctx.progressive_align(_lib.default_progressive_params())
    else:
        gs = synth.make_config("C3", scale=0.01)
        ctx.set_genomes(gs)
        a = ctx.align(_lib.default_params())
    N = len(gs)
    ctx.coord_index()
    E = _ref(a, gs)
    w = _pairs(ctx, E)
    assert len(w.height) > 0
    _core(ctx, E, [(1 << N) - 1, [0, N - 1]])
    thr, above = _lib.excursion_thresholds(ctx.excursions_fetch()[0])
    want = XR.thresholds(XR.excursions_core(E, _default()[0], [(1 << N) - 1, [0, N - 1]]).height)
    assert (thr.tolist(), above.tolist()) == want


def test_excursions_buffers_repeat_and_neighbours(ctx):
    """page-locked and pageable outputs, NULL outputs, two calls give identical bytes; pair_stats and an extract selection made before
    are unchanged after"""
    from mauvealigner_amd import _lib
    a, gs = load("g4x3k_tree")
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    st = ctx.pair_stats(per_range=True)
    n_sel = ctx.extract_select(keep=[2, 0], require=5)
    sel = ctx.extract_fetch()
    want = _pairs(ctx, E)
    ne, ns = len(want.height), len(want.stream_off) - 1
    first = [x.tobytes() for x in ctx.excursions_fetch()]
    for pinned in (True, False):
        new = _lib.pinned_empty if pinned else (lambda sh, dt: np.full(sh, 0x77, dt))
        out = (new(ne, np.int64), new(ne, np.int64), new(ns + 1, np.int64), new((ns, 2), np.int64))
        assert ctx.excursions_pairs() == ne
        got = ctx.excursions_fetch(out=out)
        assert got[0] is out[0] and got[3] is out[3]
        _same(got, want)
        assert [x.tobytes() for x in got] == first
    only = np.zeros(ne, np.int64)
    ctx._chk(ctx.L.mauve_excursions_fetch(ctx.h, None, _lib._p(only, C.c_int64), None, None), "mauve_excursions_fetch")
    assert np.array_equal(only, want.end_col)
    assert ctx.L.mauve_excursions_fetch(ctx.h, None, None, None, None) == 0
    h, e, off, tail = ctx.excursions_fetch(want=(True, False, False, True))
    assert e is None and off is None and np.array_equal(h, want.height) and np.array_equal(tail, want.tail)
    _core(ctx, E, [15, 3])
    # no range, empty ranges
    assert ctx.excursions_pairs(ranges=(np.zeros(0, np.int64),) * 3) == 0
    h, e, off, tail = ctx.excursions_fetch()
    assert h.shape == (0,) and off.tolist() == [0] and tail.shape == (0, 2)
    assert ctx.excursions_core(ranges=([0, 1], [3, 0], [0, 0])) == 0
    assert ctx.excursions_fetch()[2].tolist() == [0, 0, 0] and ctx.excursions_fetch()[3].tolist() == [[0, 0], [0, 0]]
    # the neighbours
    assert np.array_equal(ctx.pair_stats(per_range=True), st)
    again = ctx.extract_fetch()
    assert again[0].shape[1] == n_sel and all(np.array_equal(x, y) for x, y in zip(again, sel))


def test_excursions_errors_and_state(ctx):
    """every refusal of S18 by code and message; a refused call leaves no result and the index usable"""
    from mauvealigner_amd import _lib
    L = ctx.L
    n = C.c_int64(0)
    c2 = _lib.Context(0)
    try:
        assert L.mauve_excursions_pairs(c2.h, None, C.c_int64(0), None, None, C.c_int64(0), None, None, None, C.byref(n)) == -5          # no index
        assert b"no index" in L.mauve_last_error(c2.h)
        assert L.mauve_excursions_core(c2.h, None, C.c_int64(0), None, C.c_int64(0), None, None, None, C.byref(n)) == -5
        assert L.mauve_excursions_fetch(c2.h, None, None, None, None) == -5                                                               # no result
        assert b"no result" in L.mauve_last_error(c2.h)
        gs = [_codes(s) for s in HAND_GENOMES]
        c2.set_genomes(gs[:2])
        _index(c2, HAND)                                                                                                                 # an index of 3 genomes, a context of 2
        with pytest.raises(RuntimeError, match=r"\(-5\).*3 genomes"):
            c2.excursions_pairs()
        c2.set_genomes(gs)                                                                                                               # ... built before the last upload
        with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
            c2.excursions_core()
        _index(c2, HAND)
        assert c2.excursions_pairs() >= 0
        assert L.mauve_excursions_fetch(c2.h, None, None, None, None) == 0
    finally:
        c2.close()
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    ctx.excursions_pairs()
    for pairs in (([], []), ([0] * 1025, [1] * 1025), ([0], [0]), ([0], [3]), ([-1], [1])):
        with pytest.raises(RuntimeError, match=r"excursions_pairs failed \(-1\).*(n_pair|pair 0)"):
            ctx.excursions_pairs(pairs)
        with pytest.raises(RuntimeError, match=r"\(-5\).*no result"):         # a refused call leaves no result behind
            ctx.excursions_fetch()
    one = np.zeros(1, np.int32)
    assert L.mauve_excursions_pairs(ctx.h, None, C.c_int64(1), _lib._p(one, C.c_int32), None, C.c_int64(0), None, None, None, C.byref(n)) == -1       # pair_b missing
    for groups in ([], [3] * 1025, [1], [0], [8 | 1], [1 << 31 | 1]):
        with pytest.raises(RuntimeError, match=r"excursions_core failed \(-1\).*(n_group|group 0)"):
            ctx.excursions_core(groups)
    for ranges in (([1], [0], [1]), ([-1], [0], [1]), ([0], [-1], [1]), ([0], [0], [-1]), ([0], [0], [21]), ([0], [21], [0])):
        with pytest.raises(RuntimeError, match=r"\(-1\).*outside the alignment"):
            ctx.excursions_pairs(ranges=ranges)
        with pytest.raises(RuntimeError, match=r"\(-1\).*outside the alignment"):
            ctx.excursions_core(ranges=ranges)
    iv = np.zeros(1, np.int64)
    assert L.mauve_excursions_core(ctx.h, None, C.c_int64(0), None, C.c_int64(1), _lib._p(iv, C.c_int64), None, None, C.byref(n)) == -1                # missing range arrays
    assert b"missing range arrays" in L.mauve_last_error(ctx.h)
    z = np.zeros(16385, np.int64)                                             # 16 385 empty ranges x 1024 pairs: more than 2^24 streams
    with pytest.raises(RuntimeError, match=r"\(-4\).*2\^24 streams"):
        ctx.excursions_pairs(([0] * 1024, [1] * 1024), (z, z, z))
    with pytest.raises(RuntimeError, match=r"\(-4\).*2\^24 streams"):
        ctx.excursions_core([3] * 1024, (z, z, z))
    assert ctx.column_positions([0], [19])[0].tolist() == [[20, 115, -201]]   # the index is still there
    assert ctx.excursions_core() >= 0 and ctx.excursions_fetch()[2].shape == (2,)
    # a new index, a genome upload: each ends the result before
    _index(ctx, HAND)
    with pytest.raises(RuntimeError, match=r"\(-5\).*no result"):
        ctx.excursions_fetch()
    ctx.excursions_pairs()
    ctx.set_genomes(gs)
    with pytest.raises(RuntimeError, match=r"\(-5\).*no result"):
        ctx.excursions_fetch()
    with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
        ctx.excursions_pairs()
    # an interval of the index that ends beyond the resident genome
    ctx.set_genomes([gs[0], gs[1][:114], gs[2]])
    _index(ctx, HAND)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.excursions_pairs()
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    assert ctx.excursions_pairs() >= 0


def test_excursions_mirror_class():
    """mems::HipExcursions (include/libMems/Excursions.h) over IntervalLists read from committed golden XMFAs against the host loop over
    GetAlignment rows written out in tests/cpp/excursion_test.cpp"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "excursion_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "excursion_test.cpp"),
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
