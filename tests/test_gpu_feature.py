"""GPU tests of the range map and the interval-overlap join (mauve_map_ranges, mauve_map_ranges_fetch,
mauve_range_overlaps) against the restatement of tests/feature_ref.py (pinned in tests/test_feature_cpu.py).  Integer work: every array
must be equal."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests import feature_cases as FC
from tests import feature_ref as FR
from tests import pairstats_ref as PS
from tests.extract_ref import ExtractRef
from tests.test_extract_cpu import load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ("g3x5k_inv", "g4x3k_tree", "g5x3k_unique", "g4x6k_repeat")


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built5():
    """the built alignment of five genomes, its queries and the restatement's answer: made once, left unchanged"""
    a, lens = FC.built(5, 3)
    q = FC.built_queries(a, lens)
    return a, lens, q, FR.map_ranges(FC.ref_of(a), *q)


def _index(ctx, a):
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])


def _check(ctx, R, q, want=None):
    """one range map on the index in force against the restatement -> the restatement's result"""
    want = FR.map_ranges(R, *q) if want is None else want
    assert ctx.map_ranges(*q) == dict(n_query=len(q[0]), n_piece=len(want["piece_iv"]))
    got = ctx.map_ranges_fetch()
    assert FR.same(got, want) == [], FR.same(got, want)
    return want


def _check_join(ctx, tab, q):
    want = FR.range_overlaps(tab, q)
    got = ctx.range_overlaps(tab, q)
    for name, g, w in zip(("n_hit", "best", "overlap"), got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (name, np.flatnonzero(g != w)[:10])
    assert all(g.tobytes() == h.tobytes() for g, h in zip(got, ctx.range_overlaps(tab, q)))      # two calls give identical bytes
    return want


def test_map_hand_case(ctx):
    """every array written out: a flipped interval, an interval that lacks genome 1; one base, an interval exactly, one base beyond each
    end, all intervals of genome 0, a range between two intervals"""
    _index(ctx, FC.HAND)
    assert ctx.map_ranges(*FC.HAND_QUERIES) == dict(n_query=8, n_piece=12)
    got = ctx.map_ranges_fetch()
    for k in FR.ARRAYS:
        assert got[k].tolist() == FC.HAND_WANT[k], k
    _check(ctx, FC.ref_of(FC.HAND), FC.HAND_QUERIES)


def test_map_best_ties(ctx):
    """pieces of equal clipped length: the greater interval id wins whether it lies second or first in the genome's order"""
    _index(ctx, FC.TIES)
    w = _check(ctx, FC.ref_of(FC.TIES), FC.TIES_QUERIES)
    assert w["piece_iv"][w["best"]].tolist() == FC.TIES_BEST_IV
    assert ctx.map_ranges_fetch(want=("best", "piece_iv"))["piece_iv"][w["best"]].tolist() == FC.TIES_BEST_IV


@pytest.mark.parametrize("name", FIXTURES)
def test_map_golden_fixtures(ctx, name):
    a, _ = load(name)
    _index(ctx, a)
    w = _check(ctx, FC.ref_of(a), FC.random_queries(a, 11))
    assert (len(a["left"]) == 1 or np.any(np.diff(w["piece_off"]) > 1)) and np.any(np.diff(w["piece_off"]) == 0)


def test_map_built_alignment(ctx, built5):
    """intervals of 1, 63, 64, 65, 447, 448, 449 and 3000 columns, reversed rows, an absent genome, a row of only gaps in part of an
    interval; clipped ends on columns 0, 63, 64, 65, 447, 448, 449 of a block, on the residue ordinals around the samples of co_find, on the
    first and the last residue of a row"""
    a, lens, q, want = built5
    assert {1, 63, 64, 65, 447, 448, 449, 3000} <= set(np.diff(a["col_off"]).tolist()) and np.any(a["reverse"] != 0) and np.any(a["left"] == 0)
    _, kinds = FC.edge_residues(FC.ref_of(a))
    assert {"col0", "col1", "col63", "col64", "col65", "col447", "rank511", "rank512", "rank513"} <= kinds
    _index(ctx, a)
    _check(ctx, None, q, want)
    s = want["n_res"][-4:, 1].tolist()                                            # the stretch: genome 1 without a residue, with its only one in the last / first column
    assert s == [0, 1, 1, 1] and want["ext_left"][-4, 1] == 0 and want["ext_left"][-3, 1] == want["ext_right"][-2, 1] != 0
    assert np.any(np.diff(want["piece_off"]) >= len(FC.LENS) - 1)                  # a whole genome: every interval it is present in


@pytest.mark.parametrize("N", [2, 17, 32])
def test_map_built_alignment_other_genome_counts(ctx, N):
    """64 / N pieces share a wave: 32, 3 (with idle lanes) and 2"""
    a, lens = FC.built(N, 40 + N)
    q = FC.built_queries(a, lens)
    _index(ctx, a)
    _check(ctx, FC.ref_of(a), tuple(v[::7] for v in q))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_map_query_counts(ctx, built5, n):
    a, lens, q, want = built5
    k = np.arange(n) * 3 % len(q[0])
    _index(ctx, a)
    w = _check(ctx, FC.ref_of(a), tuple(v[k] for v in q))
    assert n == 1 or len(w["piece_iv"]) > n


def test_map_no_pieces_and_no_queries(ctx, built5):
    a, lens, _, _ = built5
    _index(ctx, a)
    w = _check(ctx, FC.ref_of(a), FC.no_piece_queries(a, lens, 300))
    assert len(w["piece_iv"]) == 0 and np.all(w["best"] == -1) and not np.any(w["covered"])
    e = (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert ctx.map_ranges(*e) == dict(n_query=0, n_piece=0)
    assert ctx.map_ranges_fetch()["piece_off"].tolist() == [0]
    empty = dict(left=np.zeros((0, 2), np.int64), right=np.zeros((0, 2), np.int64), reverse=np.zeros((0, 2), np.int8), col_off=np.zeros(1, np.int64), cols=np.zeros(0, np.uint32))
    _index(ctx, empty)                                                             # an index of no intervals: no pieces
    assert ctx.map_ranges([0, 1], [1, 5], [9, 5]) == dict(n_query=2, n_piece=0)
    assert ctx.map_ranges_fetch()["piece_off"].tolist() == [0, 0, 0]


def test_map_composition_with_extract_and_pair_stats(ctx):
    """the pieces are ranges: extract_select with require = all genomes and pair_stats(per_range) take them as they are"""
    a, gs = load("g4x3k_tree")
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    q = tuple(v[::9] for v in FC.random_queries(a, 5))
    w = _check(ctx, FC.ref_of(a), q)
    ranges = (w["piece_iv"], w["piece_col"], w["piece_len"])
    E = ExtractRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], gs)
    full = (1 << N) - 1
    got = ctx.extract_columns(require=full, ranges=ranges)
    for g, e in zip(got, E.extract(require=full, ranges=ranges)):
        assert np.array_equal(g, e)
    assert np.array_equal(ctx.pair_stats(ranges=ranges, per_range=True), PS.pair_stats(E, ranges=ranges, per_range=True))
    assert FR.same(ctx.map_ranges_fetch(), w) == []                                # neither call disturbed the range map


def test_join_planted(ctx):
    got = ctx.range_overlaps(FC.JOIN_TAB, FC.JOIN_QUERIES)
    for k, g in zip(("n_hit", "best", "overlap"), got):
        assert g.tolist() == FC.JOIN_WANT[k], k
    got = ctx.range_overlaps(FC.JOIN_TIES_TAB, FC.JOIN_TIES_QUERIES)
    for k, g in zip(("n_hit", "best", "overlap"), got):
        assert g.tolist() == FC.JOIN_TIES_WANT[k], k
    _check_join(ctx, FC.JOIN_TAB, FC.JOIN_QUERIES)
    e3 = (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert [v.tolist() for v in ctx.range_overlaps(e3, FC.JOIN_QUERIES)] == [[0] * 34, [-1] * 34, [0] * 34]       # m = 0
    assert [len(v) for v in ctx.range_overlaps(FC.JOIN_TAB, e3)] == [0, 0, 0]                                    # n = 0
    assert [len(v) for v in ctx.range_overlaps(e3, e3)] == [0, 0, 0]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1025, 20000])
def test_join_shuffled_tables(ctx, m):
    tab = FC.shuffled_table(m, 100 + m)
    n_hit, _, _ = _check_join(ctx, tab, FC.shuffled_queries(tab, 400, m))
    assert np.any(n_hit > 0) and np.any(n_hit == 0) and (m < 1025 or np.any(n_hit > 3))


def test_join_chained_to_a_map(ctx):
    """the extents of a map call go into the join as they are: signed, zero where a genome is absent"""
    a, _ = load("g4x3k_tree")
    N = a["left"].shape[1]
    _index(ctx, a)
    w = _check(ctx, FC.ref_of(a), tuple(v[::5] for v in FC.random_queries(a, 6)))
    tab = FC.gene_table(a, 8)
    qs = np.tile(np.arange(N, dtype=np.int32), len(w["piece_iv"]))
    q = (qs, w["ext_left"].reshape(-1), w["ext_right"].reshape(-1))
    assert np.any(q[1] < 0) and np.any(q[1] == 0)
    n_hit, _, _ = _check_join(ctx, tab, q)
    assert np.any(n_hit > 1)


def test_errors_and_state(ctx):
    from mauvealigner_amd import _lib
    a, gs = load("g4x3k_tree")
    N = len(gs)
    R = FC.ref_of(a)
    ctx.set_genomes(gs)
    _index(ctx, a)
    n_sel = ctx.extract_select(require=(1 << N) - 1)
    rows = ctx.extract_fetch()[0]
    good = tuple(v[:50] for v in FC.random_queries(a, 2))
    w = _check(ctx, R, good)
    # determinism: two calls give identical bytes; page-locked against pageable arrays; NULL outputs
    first = ctx.map_ranges_fetch()
    ctx.map_ranges(*good)
    assert all(first[k].tobytes() == v.tobytes() for k, v in ctx.map_ranges_fetch().items())
    pin_q = tuple(_lib.pinned_empty(v.shape, v.dtype) for v in good)
    for p, v in zip(pin_q, good):
        p[...] = v
    ctx.map_ranges(*pin_q)
    pinned = {k: _lib.pinned_empty(w[k].shape, np.int64) for k in FR.ARRAYS}
    for v in pinned.values():
        v[...] = 0x55
    got = ctx.map_ranges_fetch(out=pinned)
    assert got["n_res"] is pinned["n_res"] and FR.same(got, w) == []
    part = ctx.map_ranges_fetch(want=("best", "ext_left"))
    assert part["piece_off"] is None and FR.same(part, w, ("best", "ext_left")) == []
    assert ctx.L.mauve_map_ranges_fetch(ctx.h, *([None] * 12)) == 0
    # refused calls: MAUVE_ERR_ARG for the whole call, MAUVE_ERR_LIMIT for a position of 2^31 or more; the earlier result is gone
    for bad, code in (((N, 1, 5), -1), ((-1, 1, 5), -1), ((0, 0, 5), -1), ((0, -3, 5), -1), ((0, 6, 5), -1), ((0, 1, 1 << 31), -4), ((0, 1 << 31, 1 << 32), -4)):
        ctx.map_ranges(*good)
        q = tuple(np.concatenate([v, [b]]).astype(v.dtype) for v, b in zip(good, bad))
        with pytest.raises(RuntimeError, match=r"mauve_map_ranges failed \(%d\)" % code):
            ctx.map_ranges(*q)
        with pytest.raises(RuntimeError, match=r"\(-5\).*no range map"):
            ctx.map_ranges_fetch()
    # ... the index and the extract selection made before are still usable
    assert ctx.coord_index_size() == (N, len(a["left"]), len(a["cols"]))
    assert np.array_equal(ctx.extract_fetch()[0], rows) and rows.shape[1] == n_sel
    _check(ctx, R, good)
    # the join's refusals
    tab = FC.gene_table(a, 8)
    jq = (np.array([0, 1], np.int32), np.array([5, -7], np.int64), np.array([9, -9], np.int64))
    _check_join(ctx, tab, jq)
    for k, (s, lo, hi) in enumerate(((32, 1, 5), (-1, 1, 5), (0, 0, 5), (0, 6, 5), (0, -1, 5))):
        t = tuple(np.concatenate([v, [b]]).astype(v.dtype) for v, b in zip(tab, (s, lo, hi)))
        with pytest.raises(RuntimeError, match=r"mauve_range_overlaps failed \(-1\)"):
            ctx.range_overlaps(t, jq)
    for s, lo, hi in ((32, 1, 5), (-1, 1, 5), (0, 0, 5), (0, 5, 0), (0, -5, 9), (0, 5, -9), (0, 9, 5), (0, -9, -5)):
        q = tuple(np.concatenate([v, [b]]).astype(v.dtype) for v, b in zip(jq, (s, lo, hi)))
        with pytest.raises(RuntimeError, match=r"mauve_range_overlaps failed \(-1\)"):
            ctx.range_overlaps(tab, q)
    for t, q in (((np.array([0], np.int32), np.array([1], np.int64), np.array([1 << 31], np.int64)), jq),
                 (tab, (np.array([0], np.int32), np.array([1], np.int64), np.array([1 << 31], np.int64))),
                 (tab, (np.array([0], np.int32), np.array([-(1 << 62)], np.int64), np.array([-(1 << 62) - 1], np.int64)))):
        with pytest.raises(RuntimeError, match=r"mauve_range_overlaps failed \(-4\)"):
            ctx.range_overlaps(t, q)
    assert FR.same(ctx.map_ranges_fetch(), w) == []                                # the join neither needs nor disturbs the range map
    # more than 2^24 queries or table entries: refused by the count, before an array is read
    z4, z8, over = np.zeros(1, np.int32), np.zeros(1, np.int64), C.c_int64((1 << 24) + 1)
    p4, p8 = z4.ctypes.data_as(C.c_void_p), z8.ctypes.data_as(C.c_void_p)
    ctx.L.mauve_range_overlaps.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 6
    assert ctx.L.mauve_range_overlaps(ctx.h, over, p4, p8, p8, C.c_int64(1), p4, p8, p8, None, None, None) == -4
    assert ctx.L.mauve_range_overlaps(ctx.h, C.c_int64(1), p4, p8, p8, over, p4, p8, p8, None, None, None) == -4
    ctx.L.mauve_map_ranges.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    assert ctx.L.mauve_map_ranges(ctx.h, over, p4, p8, p8, None) == -4 and b"2^24" in ctx.L.mauve_last_error(ctx.h)
    _check(ctx, R, good)
    # the result ends at the next index call
    _index(ctx, a)
    with pytest.raises(RuntimeError, match=r"\(-5\).*no range map"):
        ctx.map_ranges_fetch()
    _check(ctx, R, good)
    ctx.project([0, 1])                                                             # a projection leaves it, mauve_project_index ends it
    assert FR.same(ctx.map_ranges_fetch(), w) == []
    ctx.project_index()
    with pytest.raises(RuntimeError, match=r"\(-5\).*no range map"):
        ctx.map_ranges_fetch()
    # no index: the map is refused, the join is not
    c2 = _lib.Context(0)
    try:
        with pytest.raises(RuntimeError, match=r"mauve_map_ranges failed \(-5\).*no index"):
            c2.map_ranges(*good)
        with pytest.raises(RuntimeError, match=r"\(-5\).*no range map"):
            c2.map_ranges_fetch()
        assert c2.L.mauve_map_ranges_fetch(c2.h, *([None] * 12)) == -5
        got = c2.range_overlaps(FC.JOIN_TIES_TAB, FC.JOIN_TIES_QUERIES)
        assert got[1].tolist() == FC.JOIN_TIES_WANT["best"]
    finally:
        c2.close()


def test_map_on_a_resident_alignment(ctx):
    """mauve_align, mauve_coord_index: the index of the alignment the context holds (the wide-index child runs this test, too)"""
    from mauvealigner_amd import _lib
    gs = synth.make_config("C3", scale=0.01)
    ctx.set_genomes(gs)
    a = ctx.align(_lib.default_params())
    ctx.coord_index()
    w = _check(ctx, FC.ref_of(a), tuple(v[::3] for v in FC.random_queries(a, 4, 60)))
    assert len(w["piece_iv"]) > 0


def test_map_under_a_forced_wide_index():
    env = dict(os.environ)
    env["MAUVE_WIDE_INDEX"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", "tests/test_gpu_feature.py::test_map_on_a_resident_alignment"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " passed" in r.stdout and " skipped" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


def test_ortholog_rows_mirror():
    """mems::HipFeatureMap (include/libMems/FeatureMap.h): getOrthologList's row for a planted gene table of g4x3k_tree -- best piece,
    counterpart feature and overlap in every genome, mean pairwise identity, the rearranged flag -- against the restatement composed the
    same way (tests/cpp/feature_map_test.cpp)"""
    from tests.test_feature_cpu import _build_feature_map_test, parse_rows
    a, gs = load("g4x3k_tree")
    N = len(gs)
    tab = FC.gene_table(a, 8)
    top = int(a["right"][:, 0].max())
    genes = tuple(np.concatenate([v[:58], np.array(x, v.dtype)]) for v, x in zip(tab, ([0, 0], [top + 60, top + 500], [top + 90, top + 501])))      # two genes in no interval
    E = ExtractRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], gs)
    want = FR.ortholog_rows(FC.ref_of(a), genes, tab, lambda ranges: PS.pair_stats(E, ranges=ranges, per_range=True))
    assert np.any(want["rearranged"] != 0) and np.any(want["piece_iv"] < 0) and np.any(want["identity"] > 0)
    with tempfile.TemporaryDirectory() as td:
        exe = _build_feature_map_test(td)
        mfa, genes_txt, tab_txt = (os.path.join(td, f) for f in ("g.mfa", "genes.txt", "features.txt"))
        with open(mfa, "w") as f:
            for g, s in enumerate(gs):
                f.write(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()))
        for path, t in ((genes_txt, genes), (tab_txt, tab)):
            np.savetxt(path, np.stack([np.asarray(v, np.int64) for v in t], axis=1), fmt="%d")
        r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "g4x3k_tree.xmfa"), "--device", mfa, genes_txt, tab_txt], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
        got = parse_rows(r.stdout, N)
    for k in ("piece_iv", "ortholog", "overlap", "rearranged"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["identity"], want["identity"])                       # the same integer counts, the same divisions in the same order
