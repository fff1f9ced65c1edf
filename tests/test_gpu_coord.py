"""GPU tests of the coordinate translation through the alignment (mauve_coord_index*, mauve_column_positions,
mauve_seqpos_to_column, mauve_translate_positions) against the numpy restatement of tests/coord_ref.py.  Integer work: every answer
must match exactly."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests.coord_ref import CoordRef
from tests.test_gpu_backbone import _random_alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _all_columns(a):
    iv = np.repeat(np.arange(len(a["left"]), dtype=np.int64), np.diff(a["col_off"]))
    return iv, np.arange(len(a["cols"]), dtype=np.int64) - np.asarray(a["col_off"], np.int64)[iv]


def _all_positions(a, lens=None):
    """every position of every genome: 1..len (lens given), else 1..last right end + 3"""
    N = a["left"].shape[1]
    top = [int(lens[g]) if lens is not None else int(a["right"][:, g].max(initial=0)) + 3 for g in range(N)]
    seq = np.concatenate([np.full(t, g, np.int32) for g, t in enumerate(top)])
    pos = np.concatenate([np.arange(1, t + 1, dtype=np.int64) for t in top])
    return seq, pos


def _check_everything(ctx, a, lens=None):
    """every (interval, column) through rule 1 in both modes, every position of every genome through rules 2 and 3 = the restatement
    on the same arrays.  -> (restatement, seq, pos, interval of every position)"""
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    iv, col = _all_columns(a)
    for nearest in (False, True):
        p, d = ctx.column_positions(iv, col, nearest=nearest)
        ep, ed = R.column_positions(iv, col, nearest=nearest)
        assert p.shape == ep.shape and np.array_equal(p, ep), nearest
        assert np.array_equal(d, ed), nearest
    seq, pos = _all_positions(a, lens)
    qi, qc = ctx.seqpos_to_column(seq, pos)
    ei, ec = R.seqpos_to_column(seq, pos)
    assert np.array_equal(qi, ei) and np.array_equal(qc, ec)
    for nearest in (False, True):
        t, d, ti = ctx.translate_positions(seq, pos, nearest=nearest)
        et, ed, eti = R.translate_positions(seq, pos, nearest=nearest)
        assert np.array_equal(t, et) and np.array_equal(d, ed) and np.array_equal(ti, eti), nearest
    hit = ei >= 0
    assert np.array_equal(np.abs(t[hit, seq[hit]]), pos[hit])              # the genome asked for: its own position, signed
    return R, seq, pos, ei


def test_coord_hand_case(ctx):
    """the alignment of test_backbone_hand_case: genome 1 lacks columns 10..14, genome 2 runs on the reverse strand (220 down to 201)"""
    cols = np.array([7] * 10 + [5] * 5 + [7] * 5, np.uint32)
    left, right, rev = np.array([[1, 101, 201]]), np.array([[20, 115, 220]]), np.array([[0, 0, 1]], np.int8)
    ctx.coord_index_alignment(left, right, rev, [0, 20], cols)
    p, d = ctx.column_positions([0, 0, 0, 0], [0, 12, 15, 19])
    assert p.tolist() == [[1, 101, -220], [13, 0, -208], [16, 111, -205], [20, 115, -201]] and d.tolist() == [7, 5, 7, 7]
    p, d = ctx.column_positions([0, 0], [12, 10], nearest=True)
    assert p.tolist() == [[13, 110, -208], [11, 110, -210]] and d.tolist() == [5, 5]
    iv, col = ctx.seqpos_to_column([2, 2, 2, 1, 1, 0, 0, 1], [206, 220, 201, 110, 111, 20, 21, 100])
    assert iv.tolist() == [0, 0, 0, 0, 0, 0, -1, -1] and col.tolist() == [14, 0, 19, 9, 15, 19, -1, -1]
    t, d, ti = ctx.translate_positions([2, 1, 0], [206, 111, 21])
    assert t.tolist() == [[15, 0, -206], [16, 111, -205], [0, 0, 0]] and d.tolist() == [5, 7, 0] and ti.tolist() == [0, 0, -1]
    t, d, ti = ctx.translate_positions([2], [206], nearest=True)
    assert t.tolist() == [[15, 110, -206]] and d.tolist() == [5]
    _check_everything(ctx, dict(left=left, right=right, reverse=rev, col_off=np.array([0, 20]), cols=cols))


@pytest.mark.parametrize("run", ["c3_align", "c4_align_no_unaligned", "c4_progressive"])
def test_coord_of_the_resident_alignment(ctx, run):
    """mauve_coord_index on the alignment the context holds -- on the columns the assembly left in HBM (before any fetch) and on a
    fetched / host-assembled result (uploaded) -- answers as the restatement does on the arrays the same context fetched"""
    from mauvealigner_amd import _lib
    if run == "c3_align":
        gs = synth.make_config("C3", scale=0.01)
        ctx.set_genomes(gs)
        old = os.environ.get("MAUVE_CANON_DEVICE_MIN")
        os.environ["MAUVE_CANON_DEVICE_MIN"] = "1"               # small lists take the device tail as well
        try:
            ctx.align(_lib.default_params(), fetch=False)
            ctx.coord_index()                                    # before any fetch: the columns are only in HBM
            a = ctx.align(_lib.default_params())                 # (the index is a snapshot: the second pass leaves it alone)
        finally:
            if old is None:
                del os.environ["MAUVE_CANON_DEVICE_MIN"]
            else:
                os.environ["MAUVE_CANON_DEVICE_MIN"] = old
    elif run == "c4_align_no_unaligned":
        gs = synth.make_config("C4", scale=0.02)
        ctx.set_genomes(gs)
        a = ctx.align(_lib.default_params(add_unaligned=0))
        ctx.coord_index()
    else:
        gs = synth.make_config("C4", scale=0.02)
        ctx.set_genomes(gs)
        a = ctx.progressive_align(_lib.default_progressive_params())
        ctx.coord_index()
    assert np.any(a["reverse"] != 0)                             # reverse-strand intervals are in every run
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    if run == "c4_align_no_unaligned":
        for g in range(len(gs)):
            cov = R.covered(g, len(gs[g]))
            assert cov.any() and not cov.all(), g                # ... and uncovered positions in this one
    _, seq, pos, ei = _check_everything(ctx, a, lens=[len(g) for g in gs])
    if run == "c4_align_no_unaligned":
        assert np.any(ei < 0) and np.any(ei >= 0)


def _disjoint_alignment(rng, N, n_iv, length):
    """_random_alignment of the backbone tests (`length` bounds the stretches per interval, a few hundred columns each on average; long
    runs: gap runs cross 64-column words, blocks and 4096-column tiles), with the
    intervals of each genome laid out one after another, random gaps between them, so that no base lies in two intervals; the last
    genome is kept in one interval only, and two intervals of a single column are appended"""
    left, right, rev, col_off, cols = _random_alignment(rng, N, n_iv, length, long_runs=True)
    keep = int(np.flatnonzero(left[:, N - 1])[0]) if np.any(left[:, N - 1]) else -1
    parts = []
    for i in range(n_iv):
        m = cols[col_off[i]:col_off[i + 1]].copy()
        if i != keep and left[i, N - 1]:
            m &= ~np.uint32(1 << (N - 1))
            left[i, N - 1] = right[i, N - 1] = rev[i, N - 1] = 0
            m = m[m != 0]
        parts.append(m)
    g1 = int(rng.integers(0, N - 1))
    parts += [np.array([1 << g1], np.uint32), np.array([(1 << g1) | (1 << int((g1 + 1) % (N - 1)))], np.uint32) if N > 2 else np.array([1], np.uint32)]
    n_iv += 2
    left = np.vstack([left, np.zeros((2, N), np.int64)]); right = np.vstack([right, np.zeros((2, N), np.int64)]); rev = np.vstack([rev, np.zeros((2, N), np.int8)])
    for i in (n_iv - 2, n_iv - 1):
        for g in range(N):
            if parts[i][0] >> g & 1:
                left[i, g] = 1
                rev[i, g] = int(rng.random() < 0.5)
    col_off = np.concatenate([[0], np.cumsum([len(m) for m in parts])]).astype(np.int64)
    cols = np.concatenate(parts)
    for g in range(N):
        at = 1
        for i in rng.permutation(n_iv):
            if not left[i, g]:
                continue
            cnt = int(np.count_nonzero(cols[col_off[i]:col_off[i + 1]] >> np.uint32(g) & 1))
            at += int(rng.integers(0, 40))
            left[i, g], right[i, g] = at, at + cnt - 1
            at += cnt
    return dict(left=left, right=right, reverse=rev.astype(np.int8), col_off=col_off, cols=cols)


@pytest.mark.parametrize("N", [2, 5, 8, 17, 32])
def test_coord_random_caller_alignments(ctx, N):
    rng = np.random.default_rng(4000 + N)
    a = _disjoint_alignment(rng, N, n_iv=10, length=[24, 40][N % 2])
    assert np.count_nonzero(a["left"][:, N - 1]) <= 1 and np.any(np.diff(a["col_off"]) == 1)
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    R, seq, pos, ei = _check_everything(ctx, a)
    assert np.any(ei < 0) and np.any(ei >= 0)
    if N == 32:
        _, d = ctx.column_positions(*_all_columns(a))
        assert np.any(d >> np.uint32(31))                        # bit 31 of the mask


def test_coord_boundaries(ctx):
    """first and last residue of every interval, the columns around every 64-column word, every block of the index (448 columns) and every
    512- and 4096-column boundary, the last column of the last interval -- for every genome of one case"""
    rng = np.random.default_rng(77)
    a = _disjoint_alignment(rng, 5, n_iv=8, length=40)
    N = 5
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    n_cols = len(a["cols"])
    x = np.unique(np.concatenate([np.arange(0, n_cols, s)[:, None] + np.array([-1, 0, 1]) for s in (64, 448, 512, 4096)] + [np.array([[0, n_cols - 1]])], axis=None))
    x = x[(x >= 0) & (x < n_cols)]
    iv = np.searchsorted(a["col_off"], x, side="right") - 1
    assert iv[-1] == len(a["left"]) - 1 and x[-1] == a["col_off"][-1] - 1
    col = x - a["col_off"][iv]
    for nearest in (False, True):
        p, d = ctx.column_positions(iv, col, nearest=nearest)
        ep, ed = R.column_positions(iv, col, nearest=nearest)
        assert np.array_equal(p, ep) and np.array_equal(d, ed)
    # the residues in those columns, and the two ends of every interval, back through rules 2 and 3
    seq = np.concatenate([np.repeat(np.arange(N), 2 * len(a["left"])), np.nonzero(ep)[1]]).astype(np.int32)
    pos = np.concatenate([np.concatenate([a["left"][:, g], a["right"][:, g]]) for g in range(N)] + [np.abs(ep[np.nonzero(ep)])])
    seq, pos = seq[pos > 0], pos[pos > 0]
    qi, qc = ctx.seqpos_to_column(seq, pos)
    ei, ec = R.seqpos_to_column(seq, pos)
    assert np.all(ei >= 0) and np.array_equal(qi, ei) and np.array_equal(qc, ec)
    t, d, ti = ctx.translate_positions(seq, pos, nearest=True)
    et, ed, eti = R.translate_positions(seq, pos, nearest=True)
    assert np.array_equal(t, et) and np.array_equal(d, ed) and np.array_equal(ti, eti)


def test_coord_index_is_a_snapshot(ctx):
    """the index has buffers of its own: a seed pass and an alignment of other genomes leave its answers as they were; after
    mauve_apply_homology the next mauve_coord_index follows the rewritten columns"""
    from mauvealigner_amd import _lib
    gs = synth.make_config("C3", scale=0.01)
    ctx.set_genomes(gs)
    a = ctx.align(_lib.default_params())
    ctx.coord_index()
    iv, col = _all_columns(a)
    seq, pos = _all_positions(a, [len(g) for g in gs])
    first = (ctx.column_positions(iv, col, nearest=True), ctx.seqpos_to_column(seq, pos), ctx.translate_positions(seq, pos))
    rng = np.random.default_rng(3)
    anc = rng.integers(0, 4, 30000, dtype=np.uint8)
    other = [np.ascontiguousarray(synth.mutate(anc, 0.05, rng, indel_frac=0.2)) for _ in range(3)]
    g1 = other[1].copy(); g1[12000:12600] = rng.integers(0, 4, 600, dtype=np.uint8); other[1] = g1      # unrelated sequence: the homology pass moves it
    ctx.set_genomes(other)
    ctx.seed_mums(_lib.get_seed(11, 0), fetch=False)
    b = ctx.align(_lib.default_params(seed_weight=11))
    assert b["n_cols"] != a["n_cols"]
    again = (ctx.column_positions(iv, col, nearest=True), ctx.seqpos_to_column(seq, pos), ctx.translate_positions(seq, pos))
    for x, y in zip(first, again):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    h = ctx.apply_homology()
    assert h["n_moved"] > 100 and h["n_cols"] > b["n_cols"]
    ctx.coord_index()
    _check_everything(ctx, h, lens=[len(g) for g in other])
    p, _ = ctx.column_positions(*_all_columns(h))
    assert not np.array_equal(p[:len(b["cols"])], CoordRef(b["left"], b["right"], b["reverse"], b["col_off"], b["cols"]).column_positions(*_all_columns(b))[0])


def test_coord_errors(ctx):
    """argument checks, once each: none of them reaches a kernel with an index it could follow out of bounds"""
    from mauvealigner_amd import _lib
    c2 = _lib.Context(0)
    try:
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.coord_index_size()
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.column_positions([0], [0])
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.seqpos_to_column([0], [1])
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.translate_positions([0], [1])
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            c2.coord_index()
        # the C entry points themselves (the binding above asks for the index's size first)
        import ctypes as C
        q, s, o = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(8, np.int64)
        assert c2.L.mauve_column_positions(c2.h, C.c_int64(1), _lib._p(q, C.c_int64), _lib._p(q, C.c_int64), 0, _lib._p(o, C.c_int64), None) == -5
        assert c2.L.mauve_seqpos_to_column(c2.h, C.c_int64(1), _lib._p(s, C.c_int32), _lib._p(q, C.c_int64), _lib._p(o, C.c_int64), None) == -5
        assert c2.L.mauve_translate_positions(c2.h, C.c_int64(1), _lib._p(s, C.c_int32), _lib._p(q, C.c_int64), 0, _lib._p(o, C.c_int64), None, None) == -5
        assert c2.L.mauve_column_positions(c2.h, C.c_int64(0), None, None, 0, None, None) == -5        # state comes before n = 0
    finally:
        c2.close()
    cols = np.array([7] * 10 + [5] * 5 + [7] * 5 + [3] * 4, np.uint32)
    left, right, rev = np.array([[1, 101, 201], [30, 120, 0]]), np.array([[20, 115, 220], [33, 123, 0]]), np.array([[0, 0, 1], [0, 1, 0]], np.int8)
    off = np.array([0, 20, 24])
    ctx.coord_index_alignment(left, right, rev, off, cols)
    assert ctx.coord_index_size() == (3, 2, 24)
    ok = ctx.column_positions([1], [3])
    assert ok[0].tolist() == [[33, -120, 0]]
    for iv, col in (([2], [0]), ([0], [20]), ([1], [4]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.column_positions(iv, col)
    for seq, pos in (([3], [1]), ([0], [0]), ([-1], [5]), ([0], [-7])):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.seqpos_to_column(seq, pos)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.translate_positions(seq, pos)
    assert ctx.column_positions([1], [3])[0].tolist() == [[33, -120, 0]]          # the index is still there
    # two intervals of genome 0 that share base 20
    l2 = left.copy(); r2 = right.copy(); l2[1, 0], r2[1, 0] = 20, 23
    with pytest.raises(RuntimeError, match=r"\(-1\).*intervals 0 and 1 overlap in genome 0"):
        ctx.coord_index_alignment(l2, r2, rev, off, cols)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):                             # a refused build leaves no index behind
        ctx.column_positions([1], [3])
    # one residue too many (as test_inconsistent_columns_are_refused does for the backbone), a genome the interval does not have, a bit above nseq
    c1 = cols.copy(); c1[12] |= 2
    c2_ = cols.copy(); c2_[21] |= 4
    c3 = cols.copy(); c3[0] |= np.uint32(1 << 7)
    for c in (c1, c2_, c3):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.coord_index_alignment(left, right, rev, off, c)
    ctx.coord_index_alignment(left, right, rev, off, cols)
    assert ctx.seqpos_to_column([1], [120])[1].tolist() == [3]


def test_coord_pinned_and_pageable_buffers(ctx):
    """page-locked query and answer arrays are copied directly, pageable ones through the context's staging: same answers; n = 0"""
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(9)
    a = _disjoint_alignment(rng, 8, n_iv=6, length=20)
    N = 8
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    iv, col = _all_columns(a)
    seq, pos = _all_positions(a)
    n, m = len(iv), len(seq)
    piv, pcol = _lib.pinned_empty(n, np.int64), _lib.pinned_empty(n, np.int64)
    pseq, ppos = _lib.pinned_empty(m, np.int32), _lib.pinned_empty(m, np.int64)
    piv[:], pcol[:], pseq[:], ppos[:] = iv, col, seq, pos
    o1 = (_lib.pinned_empty((n, N), np.int64), _lib.pinned_empty(n, np.uint32))
    o2 = (_lib.pinned_empty(m, np.int64), _lib.pinned_empty(m, np.int64))
    o3 = (_lib.pinned_empty((m, N), np.int64), _lib.pinned_empty(m, np.uint32), _lib.pinned_empty(m, np.int64))
    for x in o1 + o2 + o3:
        x[...] = 77
    r1, r2, r3 = ctx.column_positions(piv, pcol, nearest=True, out=o1), ctx.seqpos_to_column(pseq, ppos, out=o2), ctx.translate_positions(pseq, ppos, out=o3)
    assert r1[0] is o1[0] and r3[2] is o3[2]
    e1, e2, e3 = ctx.column_positions(iv, col, nearest=True), ctx.seqpos_to_column(seq, pos), ctx.translate_positions(seq, pos)
    m1, m2 = ctx.column_positions(piv, pcol, nearest=True), ctx.seqpos_to_column(seq, pos, out=o2)           # mixed: one side page-locked only
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    x1, x2, x3 = R.column_positions(iv, col, nearest=True), R.seqpos_to_column(seq, pos), R.translate_positions(seq, pos)
    for got in ((r1, r2, r3), (e1, e2, e3), (m1, m2, e3)):
        for u, v in zip(got, (x1, x2, x3)):
            for s, t in zip(u, v):
                assert np.array_equal(s, t)
    z = np.zeros(0, np.int64)
    p, d = ctx.column_positions(z, z)
    assert p.shape == (0, N) and d.shape == (0,)
    assert ctx.seqpos_to_column(z, z)[0].shape == (0,) and ctx.translate_positions(z, z)[0].shape == (0, N)
    # NULL outputs: the C-ABI takes any subset
    import ctypes as C
    only = np.zeros(3, np.int64)
    ctx._chk(ctx.L.mauve_seqpos_to_column(ctx.h, C.c_int64(3), _lib._p(seq[:3].copy(), C.c_int32), _lib._p(pos[:3].copy(), C.c_int64), None, _lib._p(only, C.c_int64)), "mauve_seqpos_to_column")
    assert np.array_equal(only, x2[1][:3])
    ctx._chk(ctx.L.mauve_translate_positions(ctx.h, C.c_int64(3), _lib._p(seq[:3].copy(), C.c_int32), _lib._p(pos[:3].copy(), C.c_int64), 0, None, None, None), "mauve_translate_positions")


def test_coord_large_batch(ctx):
    """one batch of 5 * 10^6 queries of each kind: more than one launch (the batches are split at 2^22 queries or 256 MiB)"""
    rng = np.random.default_rng(12)
    a = _disjoint_alignment(rng, 5, n_iv=10, length=40)
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    R = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    n = 5_000_000
    x = rng.integers(0, len(a["cols"]), n)
    iv = np.searchsorted(a["col_off"], x, side="right") - 1
    col = x - a["col_off"][iv]
    p, d = ctx.column_positions(iv, col, nearest=True)
    ep, ed = R.column_positions(iv, col, nearest=True)
    assert np.array_equal(p, ep) and np.array_equal(d, ed)
    seq = rng.integers(0, 5, n).astype(np.int32)
    pos = rng.integers(1, a["right"].max(axis=0)[seq] + 20)
    qi, qc = ctx.seqpos_to_column(seq, pos)
    ei, ec = R.seqpos_to_column(seq, pos)
    assert np.array_equal(qi, ei) and np.array_equal(qc, ec) and np.any(ei < 0)
    t, d, ti = ctx.translate_positions(seq, pos)
    et, ed, eti = R.translate_positions(seq, pos)
    assert np.array_equal(t, et) and np.array_equal(d, ed) and np.array_equal(ti, eti)


def test_coordinate_index_mirror():
    """mems::HipCoordinateIndex (include/libMems/CoordinateIndex.h) over IntervalLists read from committed golden XMFAs: every answer
    equals the host Interval::GetColumn and CompactGappedAlignment::SeqPosToColumn column walks (tests/cpp/coord_test.cpp)"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "coord_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "coord_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        for name in ("g3x5k_inv", "g4x3k_tree"):
            r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", name + ".xmfa")], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
