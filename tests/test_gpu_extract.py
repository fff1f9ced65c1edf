"""GPU tests of the column extraction (mauve_extract_select, mauve_extract_fetch) against the numpy restatement of
tests/extract_ref.py, the committed XMFA texts and mauve_write_xmfa of the same context.  Character work: every cell must match."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests.extract_ref import ExtractRef, xmfa_matrix
from tests.test_extract_cpu import COUNTS, load
from tests.test_gpu_coord import _disjoint_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _codes(s):
    return np.array(["ACGT".index(ch) for ch in s], np.uint8)


def _text(row):
    return bytes(row).decode()


def _same(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(g, w), k


def _ref(a, gs, invalid=None):
    return ExtractRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], gs, invalid)


def _index(ctx, a):
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])


HAND = dict(left=np.array([[1, 101, 201]]), right=np.array([[20, 115, 220]]), reverse=np.array([[0, 0, 1]], np.int8), col_off=np.array([0, 20]),
            cols=np.array([7] * 10 + [5] * 5 + [7] * 5, np.uint32))
HAND_GENOMES = ["ACGTACGTACGTACGTACGT" + "GG", "A" * 100 + "CCCCCGGGGGTTTTT", "C" * 200 + "ACCGGGTTTTACGTACGTAA" + "TTT"]


def test_extract_hand_case(ctx):
    """the alignment of test_coord_hand_case: genome 1 lacks columns 10..14, genome 2 runs on the reverse strand (220 down to 201: the
    reverse complement of ACCGGGTTTTACGTACGTAA)"""
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    rows, siv, scol, roff = ctx.extract_columns()
    assert [_text(r) for r in rows] == ["ACGTACGTACGTACGTACGT", "CCCCCGGGGG-----TTTTT", "TTACGTACGTAAAACCCGGT"]
    assert siv.tolist() == [0] * 20 and scol.tolist() == list(range(20)) and roff.tolist() == [0, 20]
    rows, siv, scol, roff = ctx.extract_columns(require=7)                                  # the core columns
    assert [_text(r) for r in rows] == ["ACGTACGTACTACGT", "CCCCCGGGGGTTTTT", "TTACGTACGTCCGGT"]
    assert scol.tolist() == list(range(10)) + list(range(15, 20)) and roff.tolist() == [0, 15]
    rows, siv, scol, roff = ctx.extract_columns(keep=[2, 0], ranges=([0], [8], [6]))         # a projection of a window
    assert [_text(r) for r in rows] == ["GTAAAA", "ACGTAC"] and scol.tolist() == [8, 9, 10, 11, 12, 13]
    rows, siv, scol, roff = ctx.extract_columns(keep=[1], drop_empty=True)
    assert [_text(r) for r in rows] == ["CCCCCGGGGGTTTTT"]
    rows, siv, scol, roff = ctx.extract_columns(keep=[0, 1], polymorphic=True, ranges=([0, 0], [0, 9], [2, 8]))
    # columns 0, 1: A/C, C/C -> 0 only; columns 9..16: C/G, G/-, T/-, A/-, C/-, G/-, T/T, A/T -> 9 and 16
    assert [_text(r) for r in rows] == ["ACA", "CGT"] and scol.tolist() == [0, 9, 16] and roff.tolist() == [0, 1, 3]
    E = _ref(HAND, gs)
    for kw in (dict(), dict(require=7), dict(polymorphic=True), dict(keep=[2, 1], require=1, polymorphic=True, drop_empty=True)):
        _same(ctx.extract_columns(**kw), E.extract(**kw))


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_extract_golden_fixtures(ctx, name):
    """set_genomes + coord_index_alignment on the committed fixtures: the unconditioned rows are the rows of the committed XMFA text,
    every flag combination, projections and ranges equal the restatement, the core and polymorphic counts are the pinned ones"""
    a, gs = load(name)
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    with open(os.path.join(ROOT, "tests", "golden", name + ".xmfa")) as f:
        want = xmfa_matrix(f.read(), N)
    rows, siv, scol, roff = ctx.extract_columns()
    assert np.array_equal(rows, want) and np.array_equal(roff, a["col_off"])
    full = (1 << N) - 1
    n_cols, n_core, n_poly = COUNTS[name]
    assert ctx.extract_select(require=full) == n_core and ctx.extract_select(require=full, polymorphic=True) == n_poly
    rng = np.random.default_rng(len(name))
    n_iv = len(a["left"])
    lens = np.diff(a["col_off"])
    r_iv = rng.integers(0, n_iv, 40)
    r_col = (rng.random(40) * (lens[r_iv] + 1)).astype(np.int64)
    r_len = (rng.random(40) * (lens[r_iv] - r_col + 1)).astype(np.int64)
    r_len[::7] = 0
    keeps = [None, list(range(N - 1, -1, -1)), [N - 1], [1, 0]]
    for keep, require, drop_empty, polymorphic, ranges in itertools.product(keeps, (0, full, 2), (False, True), (False, True), (None, (r_iv, r_col, r_len))):
        kw = dict(keep=keep, require=require, drop_empty=drop_empty, polymorphic=polymorphic, ranges=ranges)
        _same(ctx.extract_columns(**kw), E.extract(**kw))


def _n_positions(rng, n, frac):
    return rng.random(n) < frac


@pytest.mark.parametrize("run", ["c3_align", "c4_progressive", "c3_ambiguous"])
def test_extract_of_the_resident_alignment(ctx, run):
    """mauve_align / mauve_progressive_align, mauve_coord_index, then the extraction equals the rows of mauve_write_xmfa of the same
    context (the host writer: independent of the new code) and the restatement; c3_ambiguous: genomes with ambiguous bases
    (mauve_set_genomes_contigs), which print N on both strands"""
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
    assert np.any(a["reverse"] != 0)
    ctx.coord_index()
    want = xmfa_matrix(a["xmfa"], N)
    got = ctx.extract_columns()
    assert np.array_equal(got[0], want) and np.array_equal(got[3], a["col_off"])
    E = _ref(a, gs, inv)
    _same(got, E.extract())
    if inv is not None:
        rev_cell = np.repeat(a["reverse"] != 0, np.diff(a["col_off"]), axis=0).T                                         # [N, n_cols]: the cell is on the reverse strand
        assert np.any(want[rev_cell] == ord("N")) and np.any(want[~rev_cell] == ord("N"))                                 # both strands
        assert not np.any(want[2] == ord("N"))
    full = (1 << N) - 1
    for kw in (dict(require=full), dict(require=full, polymorphic=True), dict(keep=[N - 1, 0], drop_empty=True), dict(keep=[1, 2], polymorphic=True)):
        _same(ctx.extract_columns(**kw), E.extract(**kw))
    # backbone ranges: the segments every genome is in, then the core columns in them (stripSubsetLCBs + stripGapColumns)
    b = ctx.backbone(island_gap=20)
    m = b["seg_mask"] == full
    assert np.any(m)
    ranges = (b["seg_iv"][m], b["seg_col"][m], b["seg_len"][m])
    ctx.coord_index()
    got = ctx.extract_columns(require=full, ranges=ranges)
    _same(got, E.extract(require=full, ranges=ranges))
    assert got[0].shape[1] > 0 and not np.any(got[0] == ord("-")) and len(got[3]) == int(m.sum()) + 1


def _random_genomes(rng, a):
    return [rng.integers(0, 4, int(a["right"][:, g].max(initial=0)) + 3, dtype=np.uint8) for g in range(a["left"].shape[1])]


@pytest.mark.parametrize("N", [2, 5, 17, 32])
def test_extract_random_alignments(ctx, N):
    """random alignments with random genomes; the ranges start and end on and around multiples of 64 (a record word) and 448 (a block)"""
    rng = np.random.default_rng(5000 + N)
    a = _disjoint_alignment(rng, N, n_iv=10, length=[24, 40][N % 2])
    gs = _random_genomes(rng, a)
    inv = [_n_positions(rng, len(g), 0.02) if g_i % 2 else None for g_i, g in enumerate(gs)]
    ctx.set_genomes(gs, invalid=inv)
    _index(ctx, a)
    E = _ref(a, gs, inv)
    n_cols = len(a["cols"])
    edge = np.unique(np.concatenate([np.arange(0, n_cols, s)[:, None] + np.array([-1, 0, 1]) for s in (64, 448)], axis=None))
    edge = edge[(edge >= 0) & (edge < n_cols)]
    x0 = rng.choice(edge, 300)
    x1 = rng.choice(edge, 300)
    x0, x1 = np.minimum(x0, x1), np.maximum(x0, x1) + 1
    iv = np.searchsorted(a["col_off"], x0, side="right") - 1
    x1 = np.minimum(x1, a["col_off"][iv + 1])                                             # a range stays inside its interval
    ranges = (iv, x0 - a["col_off"][iv], x1 - x0)
    full = (1 << N) - 1
    some = [int(g) for g in rng.permutation(N)[:max(1, N // 2)]]
    req = (1 << some[0]) | (1 << int(rng.integers(0, N)))
    for kw in (dict(), dict(ranges=ranges), dict(keep=some, ranges=ranges, drop_empty=True), dict(keep=some, require=req, ranges=ranges),
               dict(polymorphic=True, ranges=ranges), dict(keep=some, require=req, polymorphic=True, drop_empty=True), dict(require=full)):
        _same(ctx.extract_columns(**kw), E.extract(**kw))
    if N == 32:
        assert np.any(ctx.extract_columns(keep=[31], drop_empty=True)[0] != ord("-"))


def test_extract_composes_with_column_positions(ctx):
    """(sel_iv, sel_col) is what mauve_column_positions takes: the positions of the selected columns, read from the genomes in numpy,
    spell the fetched rows"""
    a, gs = load("g4x3k_tree")
    ctx.set_genomes(gs)
    _index(ctx, a)
    rows, siv, scol, _ = ctx.extract_columns(keep=[2, 0, 3], require=0b0101, polymorphic=True)
    assert rows.shape[1] > 50
    pos, _ = ctx.column_positions(siv, scol)
    for k, g in enumerate((2, 0, 3)):
        p = pos[:, g]
        b = gs[g][np.maximum(np.abs(p) - 1, 0)]
        spelled = np.where(p == 0, ord("-"), np.frombuffer(b"ACGT", np.uint8)[np.where(p < 0, 3 - b, b)])
        assert np.array_equal(spelled, rows[k]), g
    assert np.any(pos < 0) and np.any(pos == 0)


def test_extract_pinned_and_pageable_buffers(ctx):
    """page-locked outputs are copied directly, pageable ones through the staging; a row stride above n_sel leaves the padding
    untouched, an odd row stride is as good as any, one row"""
    from mauvealigner_amd import _lib
    a, gs = load("g5x3k_unique")
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    E = _ref(a, gs)
    for kw in (dict(require=(1 << N) - 1), dict(keep=[3]), dict(keep=[4, 1], polymorphic=True)):
        want = E.extract(**kw)
        nk, ns = want[0].shape
        assert ns > 100
        for stride in (ns, ns + 1 if (ns + 1) % 2 else ns + 2, ns + 37, ns + 64):
            for pinned in (True, False):
                new = _lib.pinned_empty if pinned else (lambda sh, dt: np.empty(sh, dt))
                wide = new((nk, stride), np.uint8)
                wide[...] = 0x77
                out = (wide[:, :ns], new(ns, np.int64), new(ns, np.int64), new(len(want[3]), np.int64))
                assert ctx.extract_select(**{k: v for k, v in kw.items()}) == ns
                got = ctx.extract_fetch(out=out)
                assert got[0] is out[0] and got[3] is out[3]
                _same(got, want)
                assert np.all(wide[:, ns:] == 0x77), (stride, pinned)
    # NULL outputs: the C-ABI takes any subset; a second fetch of the same selection gives the same
    ns = ctx.extract_select(keep=[0, 2], require=5)
    only = np.zeros(ns, np.int64)
    ctx._chk(ctx.L.mauve_extract_fetch(ctx.h, None, C.c_int64(0), None, _lib._p(only, C.c_int64), None), "mauve_extract_fetch")
    again = ctx.extract_fetch()
    assert np.array_equal(only, again[2])
    _same(again, E.extract(keep=[0, 2], require=5))
    # nothing selected, no range
    got = ctx.extract_columns(keep=[0], require=1, ranges=(np.zeros(0, np.int64),) * 3)
    assert got[0].shape == (1, 0) and got[3].tolist() == [0]
    got = ctx.extract_columns(ranges=([0, 1], [3, 0], [0, 0]))
    assert got[0].shape == (N, 0) and got[3].tolist() == [0, 0, 0]


def test_extract_errors_and_state(ctx):
    """every refusal of S15, once each; none of them reaches a kernel with an index it could follow out of bounds; a failed call leaves
    the index usable"""
    from mauvealigner_amd import _lib
    c2 = _lib.Context(0)
    try:
        p = _lib.ExtractParams()
        c2.L.mauve_default_extract_params.restype = None
        c2.L.mauve_default_extract_params(3, C.byref(p))
        assert (p.n_keep, list(p.keep)[:4], p.require, p.drop_empty, p.polymorphic) == (3, [0, 1, 2, 0], 0, 0, 0)
        n = C.c_int64(0)
        assert c2.L.mauve_extract_select(c2.h, C.byref(p), C.c_int64(0), None, None, None, C.byref(n)) == -5                 # no index
        assert c2.L.mauve_extract_fetch(c2.h, None, C.c_int64(0), None, None, None) == -5                                     # no selection
        gs = [_codes(s) for s in HAND_GENOMES]
        c2.set_genomes(gs[:2])
        _index(c2, HAND)                                                                                                     # an index of 3 genomes, a context of 2
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.extract_select()
        c2.set_genomes(gs)                                                                                                   # ... built before the last upload
        with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
            c2.extract_select()
        _index(c2, HAND)
        assert c2.extract_select() == 20
        assert c2.L.mauve_extract_fetch(c2.h, None, C.c_int64(0), None, None, None) == 0
    finally:
        c2.close()
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    two = dict(left=np.array([[1, 101, 201], [21, 0, 221]]), right=np.array([[20, 115, 220], [22, 0, 222]]), reverse=np.array([[0, 0, 1], [0, 0, 0]], np.int8),
               col_off=np.array([0, 20, 22]), cols=np.concatenate([HAND["cols"], np.array([5, 5], np.uint32)]))
    _index(ctx, two)
    assert ctx.extract_select(ranges=([1, 0], [0, 18], [2, 2])) == 4
    assert [_text(r) for r in ctx.extract_fetch()[0]] == ["GGGT", "--TT", "TTGT"]
    for ranges in (([2], [0], [1]), ([-1], [0], [1]), ([0], [-1], [1]), ([0], [0], [-1]), ([0], [0], [21]), ([0], [21], [0]), ([1], [1], [2]),
                   ([0, 1, 0], [0, 3, 0], [20, 0, 20])):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.extract_select(ranges=ranges)
        with pytest.raises(RuntimeError, match=r"\(-5\)"):                    # a refused select leaves no selection behind
            ctx.extract_fetch()
    for kw in (dict(keep=[]), dict(keep=[0, 1, 2, 0]), dict(keep=[3]), dict(keep=[-1]), dict(keep=[1, 1]), dict(require=8), dict(require=1 << 31)):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.extract_select(**kw)
    assert ctx.column_positions([1], [1])[0].tolist() == [[22, 0, 222]]        # the index is still there
    assert ctx.extract_select(keep=[2, 0]) == 22
    with pytest.raises(RuntimeError, match=r"\(-1\).*row_stride"):
        ctx._chk(ctx.L.mauve_extract_fetch(ctx.h, C.c_void_p(np.zeros(64, np.uint8).ctypes.data), C.c_int64(21), None, None, None), "mauve_extract_fetch")
    assert ctx.extract_fetch()[0].shape == (2, 22)                              # ... and so is the selection
    # a later select, a new index, a genome upload: each ends the selection before
    _index(ctx, two)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.extract_fetch()
    assert ctx.extract_select() == 22
    ctx.set_genomes(gs)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.extract_fetch()
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.extract_select()
    assert ctx.column_positions([0], [19])[0].tolist() == [[20, 115, -201]]     # the index outlives the upload (S14), only the extraction refuses it
    # an interval of the index that ends beyond the resident genome
    ctx.set_genomes([gs[0], gs[1][:114], gs[2]])
    _index(ctx, two)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.extract_select()
    ctx.set_genomes(gs)
    _index(ctx, two)
    assert ctx.extract_select(require=5) == 22


def test_one_range_list_through_both_front_end_callers(ctx):
    """extract_select and pair_stats share the range front end: the same range list through both, on the hand case.  Every column of a range
    is selected once (every genome kept, no rule) and is counted once for every pair (a letter pair, a one-sided column or an empty one);
    a range one column too long is refused by both, and the refused select leaves no selection; the records come out the same through the
    staging and straight into page-locked memory, right after the coordinate stage used the staging"""
    from mauvealigner_amd import _lib
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    # an empty range, one that starts inside a 64-column word, the whole interval, two ranges of the same interval (overlapping)
    iv, col, ln = [0, 0, 0, 0, 0], [7, 5, 0, 2, 9], [0, 9, 20, 3, 8]
    assert ctx.extract_select(ranges=(iv, col, ln)) == sum(ln)
    rows, siv, scol, roff = ctx.extract_fetch()
    st = ctx.pair_stats(ranges=(iv, col, ln), per_range=True)
    assert st.shape == (len(ln), 3, 32)
    for r in range(len(ln)):
        assert roff[r + 1] - roff[r] == ln[r]
        assert scol[roff[r]:roff[r + 1]].tolist() == list(range(col[r], col[r] + ln[r]))
        for p in range(3):
            assert st[r, p, :25].sum() + st[r, p, 25] + st[r, p, 26] + st[r, p, 29] == ln[r], (r, p)
    long = (iv + [0], col + [15], ln + [6])                   # columns 15 .. 20 of an interval of 20
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.extract_select(ranges=long)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.extract_fetch()
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.pair_stats(ranges=long, per_range=True)
    # one staging buffer: pageable and page-locked records straight after an index call and a query of the coordinate stage
    _index(ctx, HAND)
    assert ctx.column_positions([0], [19])[0].tolist() == [[20, 115, -201]]
    pageable = ctx.pair_stats(ranges=(iv, col, ln), per_range=True, out=np.empty((len(ln), 3, 32), np.int64))
    pinned = ctx.pair_stats(ranges=(iv, col, ln), per_range=True, out=_lib.pinned_empty((len(ln), 3, 32), np.int64))
    assert np.array_equal(pageable, pinned) and np.array_equal(pageable, st)


def test_extract_full_size_c3(ctx):
    """the C3 configuration of bench.py (5 x 5 Mbp) aligned once: all columns of all genomes, then the polymorphic core columns --
    both equal to the restatement, every byte"""
    import time
    from mauvealigner_amd import _lib
    gs = synth.make_config("C3", scale=1.0)
    N = len(gs)
    ctx.set_genomes(gs)
    a = ctx.align(_lib.default_params(seed_weight=15))
    ctx.coord_index()
    E = _ref(a, gs)
    full = (1 << N) - 1
    for kw in (dict(), dict(require=full, polymorphic=True)):
        t0 = time.perf_counter()
        got = ctx.extract_columns(**kw)
        dt = time.perf_counter() - t0
        want = E.extract(**kw)
        print("extract at C3 %s: %d of %d columns, %.1f ms" % (kw, got[0].shape[1], a["n_cols"], dt * 1e3))
        _same(got, want)
        assert got[0].shape[1] > 100_000


def test_alignment_extractor_mirror():
    """mems::HipAlignmentExtractor (include/libMems/AlignmentExtractor.h) over IntervalLists read from committed golden XMFAs, with the
    genomes of the fixture: equal to the host Interval::GetAlignment and to the stripGapColumns loop (tests/cpp/extract_test.cpp)"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "extract_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "extract_test.cpp"),
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
