"""GPU tests of the projection onto a genome subset (mauve_project, mauve_project_fetch, mauve_project_index) against the
restatement of tests/project_ref.py (pinned in tests/test_project_cpu.py).  Integer work: every array -- interval ends, strands, column
offsets, columns, provenance -- must be equal."""
import ctypes as C
import itertools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests import excursion_ref as XR
from tests import project_ref as PR
from tests.extract_ref import ExtractRef
from tests.test_extract_cpu import load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("g3x5k_inv", "g4x3k_tree", "g5x3k_unique", "g4x6k_repeat")
COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "CG"):
    COMPLEMENT[ord(_a)], COMPLEMENT[ord(_b)] = ord(_b), ord(_a)


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _index(ctx, a):
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])


def _check(ctx, a, proj, drop_empty=True, compact=False):
    """one projection of the index in force (the alignment a) against the restatement -> the restatement's result"""
    want = PR.project(a, proj, drop_empty, compact)
    sz = ctx.project(proj, drop_empty)
    assert sz == dict(n_iv=len(want["left"]), n_cols=len(want["cols"]), n_src=len(want["src_iv"]), n_fill=want["n_fill"]), (proj, drop_empty)
    got = ctx.project_fetch(compact)
    assert PR.same(got, want) == [], (proj, drop_empty, compact, PR.same(got, want))
    return want


def test_project_hand_case(ctx):
    """the alignment of test_hand_case_every_array_written_out: a flipped interval, two that join once genome 2 is dropped with 3 and 0
    bases between them, one that lacks genome 1"""
    a = PR.HAND
    _index(ctx, a)
    assert ctx.project([0, 1]) == dict(n_iv=2, n_cols=15, n_src=3, n_fill=3)
    r = ctx.project_fetch()
    assert r["cols"].tolist() == [3, 3, 2, 1, 3,  3, 2, 1, 3,  1, 1, 1,  3, 3, 3] and r["col_off"].tolist() == [0, 5, 15]
    assert r["src_col"].tolist() == [5, 4, 2, 1, 0,  6, 7, 8, 9,  -1, -1, -1,  10, 11, 12]
    assert r["left"].tolist() == [[1, 1, 0], [6, 6, 0]] and r["right"].tolist() == [[4, 4, 0], [14, 11, 0]] and r["reverse"].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert (r["src_off"].tolist(), r["src_iv"].tolist(), r["src_flip"].tolist()) == ([0, 1, 3], [0, 1, 2], [1, 0, 0])
    for proj in ([0, 1], [1, 0], [2, 0], [0], [2], [1, 2], [0, 1, 2], [2, 1, 0]):
        for drop, compact in itertools.product((True, False), (False, True)):
            _check(ctx, a, proj, drop, compact)
    assert ctx.project() == ctx.project([0, 1, 2], True)                       # the defaults: every genome in order, drop_empty


@pytest.mark.parametrize("name", FIXTURES)
def test_project_golden_fixtures(ctx, name):
    """coord_index_alignment on the committed fixtures: all pairs and the full set, both drop_empty values, compact and wide"""
    a, gs = load(name)
    N = len(gs)
    _index(ctx, a)
    for P in list(itertools.combinations(range(N), 2)) + [tuple(range(N))]:
        for drop, compact in itertools.product((True, False), (False, True)):
            _check(ctx, a, P, drop, compact)
    _check(ctx, a, [N - 1, 0])
    _check(ctx, a, [N - 1])


GAPS = (0, 1, 1500, 0, 7, 1)
RUNS = (3, 1, 4, 2, 5)


def _built(N, seed):
    """a caller's alignment of N genomes made of runs of collinear pieces.  Piece lengths 1, 63, 64, 65, 447, 448, 449 and 3000 in a random
    order, then pieces that begin one column before, at and one column after a multiple of 64 and of 448.  Inside a run genome g runs
    forward or backward (s[g]); every second piece is stored in its inverted form (columns reversed, every strand toggled), so whatever
    proj[0] is, flipped and unflipped pieces alternate.  Between two pieces of a run a genome has 0, 1, 7 or 1500 bases.  With three or
    more genomes the one-piece runs lack the last genome.  -> (alignment, genome lengths)"""
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.permutation([1, 63, 64, 65, 447, 448, 449, 3000])]
    pad = -sum(lens) % 448
    lens += ([pad] if pad else []) + [63, 1, 1, 382, 1, 1, 62, 1, 1]
    nxt = np.ones(N, np.int64)                                                     # every genome's next free base
    left, right, rev, cols, off = [], [], [], [], [0]
    j = r = 0
    while j < len(lens):
        m = min(RUNS[r % len(RUNS)], len(lens) - j)
        s = rng.integers(0, 2, N).astype(bool)
        present = np.ones(N, bool)
        if N > 2 and m == 1:
            present[N - 1] = False
        bits = []
        for L in lens[j:j + m]:
            b = (rng.random((L, N)) < 0.75) & present
            b[rng.random(L) < 0.1] = False                                          # columns of no genome
            b[0] = present
            bits.append(b)
        n_res = np.array([b.sum(axis=0) for b in bits], np.int64)                   # [m, N]
        gap = np.array([[GAPS[(j + q + 2 * g) % len(GAPS)] for g in range(N)] for q in range(m - 1)], np.int64).reshape(m - 1, N)
        before = np.concatenate([np.zeros((1, N), np.int64), np.cumsum(n_res[:-1] + gap, axis=0)])   # bases of the run in front of piece q, run order
        total = n_res.sum(axis=0) + gap.sum(axis=0)
        for q in range(m):
            lo = np.where(s, nxt + total - before[q] - n_res[q], nxt + before[q])
            inv = (j + q) % 2 == 1
            left.append(np.where(present, lo, 0)), right.append(np.where(present, lo + n_res[q] - 1, 0)), rev.append((s ^ inv) & present)
            b = bits[q][::-1] if inv else bits[q]
            cols.append((b.astype(np.uint64) << np.arange(N, dtype=np.uint64)).sum(axis=1).astype(np.uint32))
            off.append(off[-1] + len(b))
        nxt = nxt + np.where(present, total + 5, 0)
        j += m
        r += 1
    a = dict(left=np.array(left, np.int64), right=np.array(right, np.int64), reverse=np.array(rev, np.int8), col_off=np.array(off, np.int64), cols=np.concatenate(cols))
    return a, nxt + 10


@pytest.mark.parametrize("N", [2, 5, 17, 32])
def test_project_built_alignments(ctx, N):
    """intervals that begin and end around multiples of 64 and 448 columns, alternating flips, fillers of 0, 1 and more than 1024 bases,
    runs of three and more pieces; n_proj = 1, 2 and N, lists that do not ascend"""
    a, _ = _built(N, 19 + N)
    starts = set((a["col_off"][:-1] % 448).tolist())
    assert {0, 1, 447, 63, 64, 65} <= starts and {1, 63, 64, 65, 447, 448, 449, 3000} <= set(np.diff(a["col_off"]).tolist())
    _index(ctx, a)
    lists = [[N - 1, 0], [N - 1], list(range(N)), list(range(N))[::-1], [N // 2, N - 1] if N > 2 else [1, 0], [0]]
    seen_long = seen_alt = seen_three = False
    for proj in lists:
        for drop in (True, False):
            w = _check(ctx, a, proj, drop)
        _check(ctx, a, proj, True, compact=True)
        fill = np.flatnonzero(w["src_col"] < 0)
        if len(fill):
            runs = np.diff(np.flatnonzero(np.concatenate([[True], (np.diff(fill) != 1) | (np.diff(w["cols"][fill]) != 0), [True]])))
            seen_long |= bool(np.any(runs > 1024))
        pieces = np.diff(w["src_off"])
        seen_three |= bool(np.any(pieces >= 3))
        for o in np.flatnonzero(pieces >= 2):
            f = w["src_flip"][w["src_off"][o]:w["src_off"][o + 1]]
            seen_alt |= bool(np.all(np.diff(f) != 0))
    assert seen_long and seen_alt and seen_three


def test_project_nothing_kept_and_an_empty_index(ctx):
    a = dict(left=np.array([[1, 0], [0, 1]]), right=np.array([[3, 0], [0, 2]]), reverse=np.zeros((2, 2), np.int8), col_off=np.array([0, 3, 5]), cols=np.array([1, 1, 1, 2, 2], np.uint32))
    _index(ctx, a)
    for drop, compact in itertools.product((True, False), (False, True)):
        w = _check(ctx, a, [0, 1], drop, compact)
        assert len(w["left"]) == 0 and w["col_off"].tolist() == [0]
    assert _check(ctx, a, [1])["cols"].tolist() == [2, 2]
    ctx.set_genomes([np.zeros(8, np.uint8)] * 2)
    _index(ctx, a)
    ctx.project([1, 0])
    ctx.project_index()                                                             # an index of no intervals is legal ...
    assert ctx.coord_index_size() == (2, 0, 0)
    assert ctx.project([0, 1]) == dict(n_iv=0, n_cols=0, n_src=0, n_fill=0)       # ... and so is its projection
    assert ctx.project_fetch()["src_off"].tolist() == [0]


def _compose(ctx, a, gs, proj):
    """the projection made the index in force: S14, S15 and S18 on it, and the round trip through mauve_coord_index_alignment"""
    N = len(gs)
    P = list(proj)
    n_src = len(a["cols"])
    siv = np.repeat(np.arange(len(a["left"]), dtype=np.int64), np.diff(a["col_off"]))
    _index(ctx, a)
    spos, sdef = ctx.column_positions(siv, np.arange(n_src, dtype=np.int64) - a["col_off"][siv])
    srows = ctx.extract_columns(keep=P)[0]
    assert srows.shape == (len(P), n_src)
    w = _check(ctx, a, P)
    ctx.project_index()
    assert ctx.coord_index_size() == (N, len(w["left"]), len(w["cols"]))
    assert PR.same(ctx.project_fetch(), w) == []                                    # the projection stays fetchable
    oiv = np.repeat(np.arange(len(w["left"]), dtype=np.int64), np.diff(w["col_off"]))
    pos, dfn = ctx.column_positions(oiv, np.arange(len(w["cols"]), dtype=np.int64) - w["col_off"][oiv])
    assert np.array_equal(dfn, w["cols"])
    src = w["src_col"] >= 0
    x = w["src_col"][src]
    flipped = np.zeros(len(a["left"]), bool)
    flipped[w["src_iv"]] = w["src_flip"] != 0
    fl = flipped[siv[x]]
    keep = np.zeros(N, bool)
    keep[P] = True
    assert np.array_equal(pos[src], np.where(keep[None, :], np.where(fl[:, None], -spos[x], spos[x]), 0))
    rows = ctx.extract_columns(keep=P)[0]
    assert np.array_equal(rows[:, src], np.where(fl[None, :], COMPLEMENT[srows[:, x]], srows[:, x]))
    fill_rows = rows[:, ~src]                                                      # a filler column: one letter, the others '-'
    assert np.all((fill_rows != ord("-")).sum(axis=0) == 1)
    E = ExtractRef(w["left"], w["right"], w["reverse"], w["col_off"], w["cols"], gs)
    assert np.array_equal(rows, E.extract(keep=P)[0])
    if len(P) >= 2:                                                                 # the multiEVD step: the core excursions of the group P
        from mauvealigner_amd import _lib
        d = _lib.default_scoring()
        want = XR.excursions_core(E, [list(r) for r in d.matrix], [P])
        assert ctx.excursions_core([P]) == len(want.height)
        for g, e in zip(ctx.excursions_fetch(), want.arrays()):
            assert np.array_equal(g, e)
    got = ctx.project_fetch()
    _index(ctx, got)                                                                # check_columns accepts it
    assert ctx.coord_index_size() == (N, len(w["left"]), len(w["cols"]))
    pos2, dfn2 = ctx.column_positions(oiv, np.arange(len(w["cols"]), dtype=np.int64) - w["col_off"][oiv])
    assert np.array_equal(pos2, pos) and np.array_equal(dfn2, dfn)


def test_project_index_composition(ctx):
    a, gs = load("g4x3k_tree")
    ctx.set_genomes(gs)
    _compose(ctx, a, gs, [0, 1])
    _compose(ctx, a, gs, [3, 2])
    a, lens = _built(5, 3)
    rng = np.random.default_rng(7)
    gs = [rng.integers(0, 4, int(n), dtype=np.uint8) for n in lens]
    ctx.set_genomes(gs)
    _compose(ctx, a, gs, [4, 0])
    _compose(ctx, a, gs, [2, 1, 3])


def test_project_of_a_resident_progressive_alignment(ctx):
    """mauve_progressive_align, mauve_coord_index: genomes are absent from some intervals; onto a pair"""
    from mauvealigner_amd import _lib
    gs = synth.make_config("C4", scale=0.02)
    ctx.set_genomes(gs)
    a = ctx.progressive_align(_lib.default_progressive_params())
    k = np.count_nonzero(a["left"], axis=1)
    assert np.any((k > 1) & (k < len(gs)))
    ctx.coord_index()
    for P in ([0, 1], [len(gs) - 1, 1]):
        w = _check(ctx, a, P)
        assert 0 < len(w["src_iv"]) < len(a["left"])
        _check(ctx, a, P, False, True)
    _compose(ctx, a, gs, [0, len(gs) - 1])


def test_project_buffers_and_state(ctx):
    from mauvealigner_amd import _lib
    a, gs = load("g4x3k_tree")
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    want = _check(ctx, a, [0, 2])
    # two calls return identical bytes; page-locked against pageable destinations; NULL outputs
    first = ctx.project_fetch()
    ctx.project([0, 2])
    assert all(first[k].tobytes() == v.tobytes() for k, v in ctx.project_fetch().items())
    pinned = {k: _lib.pinned_empty(want[k].shape, want[k].dtype) for k in PR.ARRAYS}
    for v in pinned.values():
        v[...] = 0x55
    got = ctx.project_fetch(out=pinned)
    assert got["cols"] is pinned["cols"] and PR.same(got, want) == []
    part = ctx.project_fetch(want=("cols", "src_off"))
    assert part["left"] is None and part["src_col"] is None and PR.same(part, want, ("cols", "src_off")) == []
    assert ctx.L.mauve_project_fetch(ctx.h, 1, *([None] * 9)) == 0
    # refusals: the index stays usable, the earlier projection is gone
    for proj, text in (([], "n_proj"), (list(range(N)) + [0], "n_proj"), ([0, 0], "repeated"), ([N], "outside"), ([-1, 0], "outside")):
        ctx.project([0, 1])
        with pytest.raises(RuntimeError, match=r"mauve_project failed \(-1\).*" + text):
            ctx.project(proj)
        with pytest.raises(RuntimeError, match=r"\(-5\).*no projection"):
            ctx.project_fetch()
        with pytest.raises(RuntimeError, match=r"\(-5\).*no projection"):
            ctx.project_index()
    assert ctx.coord_index_size() == (N, len(a["left"]), len(a["cols"]))
    assert np.array_equal(ctx.column_positions([0], [0])[1], a["cols"][:1])
    _check(ctx, a, [1, 3])
    # a genome upload after the index: the projection is still made and fetched, it cannot become the index
    ctx.set_genomes(gs)
    _check(ctx, a, [1, 3])
    with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
        ctx.project_index()
    assert PR.same(ctx.project_fetch(), PR.project(a, [1, 3])) == []               # a refused call leaves the projection and the index
    assert ctx.coord_index_size()[1] == len(a["left"])
    ctx.set_genomes(gs[:2])
    _index(ctx, a)
    ctx.project([0, 1])
    with pytest.raises(RuntimeError, match=r"\(-5\).*4 genomes, the context holds 2"):
        ctx.project_index()
    c2 = _lib.Context(0)
    try:
        with pytest.raises(RuntimeError, match=r"\(-5\).*no index"):
            c2.project([0])
        assert c2.L.mauve_project(c2.h, C.byref(_lib.default_project_params(1)), None) == -5 and b"project: no index" in c2.L.mauve_last_error(c2.h)
        with pytest.raises(RuntimeError, match=r"\(-5\).*no projection"):
            c2.project_fetch()
        with pytest.raises(RuntimeError, match=r"\(-5\).*no projection"):
            c2.project_index()
    finally:
        c2.close()
    # src_col is made by the first fetch that asks for it: here after the source index is gone
    ctx.set_genomes(gs)
    _index(ctx, a)
    ctx.project([3, 0])
    assert PR.same(ctx.project_fetch(want=("cols",)), PR.project(a, [3, 0]), ("cols",)) == []
    ctx.project_index()
    _index(ctx, PR.HAND)
    assert PR.same(ctx.project_fetch(), PR.project(a, [3, 0])) == []
    assert PR.same(ctx.project_fetch(compact=True), PR.project(a, [3, 0], compact=True)) == []
    # the projection of a projection: the second index is the first result
    ctx.set_genomes(gs)
    _index(ctx, a)
    w1 = _check(ctx, a, [0, 1, 2])
    ctx.project_index()
    assert ctx.extract_select() == len(w1["cols"])
    ctx.project_index()                                                             # again: the same index, the selection ended
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.extract_fetch()
    _check(ctx, w1, [2, 0])


def test_projection_mirror():
    """mems::HipProjection (include/libMems/Projection.h) over IntervalLists read from committed golden XMFAs against the mirror's host
    projectIntervalList: the same groups, ends, strands and -- without the filler -- columns; the projection made the index in force
    answers with the source's positions (tests/cpp/project_test.cpp)"""
    from tests.test_project_cpu import _build_project_test, parse_groups
    with tempfile.TemporaryDirectory() as td:
        exe = _build_project_test(td)
        for name, lists in (("g3x5k_inv", ([2, 0], [0, 1])), ("g4x3k_tree", ([0, 1], [3, 1, 0], [2]))):
            a, gs = load(name)
            mfa = os.path.join(td, name + ".mfa")
            with open(mfa, "w") as f:
                for g, s in enumerate(gs):
                    f.write(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()))
            for P in lists:
                r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", name + ".xmfa"), "--device", mfa] + [str(g) for g in P], capture_output=True, text=True)
                assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
                w = PR.project(a, P, drop_empty=False)
                assert len(parse_groups(r.stdout)) == len(w["left"])
                assert "%d intervals, %d columns, %d filler columns, %d inverted pieces" % (len(w["left"]), len(w["cols"]), w["n_fill"], int(w["src_flip"].sum())) in r.stdout
