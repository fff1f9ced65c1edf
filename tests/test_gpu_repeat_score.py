"""A repeat map scored against a correct repeat alignment on the device (mauve_repeat_score) against the plain-Python
restatement tests/repeat_score_ref.py, every counter and every table word: the planted cases of tests/repeat_score_cases.py, the word and
block edges of the truth index, the tile edges of the extent table, 2, 5 and 32 rows, repeat maps made on the device and scored where they
lie and as a fetched list, empty inputs, every refusal, what the call leaves alone, and the mirror's HipRepeatScore."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, repeat_accuracy
from oracle import pyoracle as O
from tests import repeat_map_cases as MC
from tests import repeat_map_ref as MR
from tests import repeat_score_cases as RC
from tests import repeat_score_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib.C


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def same(got, want, what=""):
    assert got["totals"] == want["totals"], (what, got["totals"], want["totals"])
    for k in ("pair_records", "comp_hit", "pair_hit"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def check(ctx, case, what=""):
    ctx.score_truth(case["truth"])
    got = ctx.repeat_score(case["records"], case["row_offset"])
    want = SR.score(case["truth"], case["records"], case["row_offset"])
    same(got, want, what)
    return got


@pytest.mark.parametrize("name", list(RC.CASES))
def test_planted_cases(ctx, name):
    got = check(ctx, RC.CASES[name], name)
    assert got["totals"] == RC.CASES[name]["totals"]


def test_concatenated_form_gives_the_same_bytes(ctx):
    a, b = check(ctx, RC.CASES["hand3"]), check(ctx, RC.CASES["hand3_concat"])
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("pair_records", "comp_hit", "pair_hit")) and a["totals"] == b["totals"]


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 447, 448, 449, 897])
def test_word_and_block_edges_of_the_truth(ctx, ncols):
    got = check(ctx, RC.random_case(100 + ncols, 3, ncols, 8), ncols)
    assert got["totals"]["sp_possible"] > 0 or ncols == 1


def sized_map(M, seed):
    """a truth of 4 rows and 300 columns and a map of exactly M components: records of 2 components, one of 3 where M is odd"""
    c = RC.random_case(seed, 4, 300, 1)
    P = SR.truth_positions(c["truth"])[0]
    rev = c["truth"]["reverse"][0]
    rng = np.random.default_rng(seed)
    recs = []
    for k in range((M - 3) // 2 + 1 if M % 2 else M // 2):
        m = 3 if (M % 2 and k == 0) else 2
        rows = rng.permutation(4)[:m]
        a, ln = int(rng.integers(0, 290)), int(rng.integers(1, 10))
        st = []
        for g in rows:
            p = int(P[g][a]) or int(P[g][P[g] > 0][0])
            st.append((-1 if rev[g] else 1) * max(1, p - ln + 1 if rev[g] else p))
        recs.append((ln, tuple(st)))
    c["records"] = RC.csr(recs)
    assert len(c["records"][3]) == M
    return c


@pytest.mark.parametrize("M", [2, 3, 1023, 1024, 1025])
def test_tile_edges_of_the_extent_table(ctx, M):
    """(a record has 2 components or more: the smallest table has 2 entries, not 1)"""
    got = check(ctx, sized_map(M, 900 + M), M)
    assert got["totals"]["components"] == M and got["totals"]["sp_truepos"] > 0


@pytest.mark.parametrize("nrows", [2, 5, 32])
def test_row_counts(ctx, nrows):
    got = check(ctx, RC.random_case(300 + nrows, nrows, 150, 20), nrows)
    assert got["totals"]["sp_truepos"] > 0 and got["pair_records"].shape == (nrows, nrows, 4)


def resident_and_list(ctx, genome, truth, pattern, what):
    ctx.set_genomes([genome])
    records = ctx.repeat_matches(0, pattern)
    ctx.score_truth(truth)
    res = ctx.repeat_score()                                   # where the map lies: no list
    lst = ctx.repeat_score(records)
    same(res, lst, what)
    assert all(res[k].tobytes() == lst[k].tobytes() for k in ("pair_records", "comp_hit", "pair_hit"))
    same(res, SR.score(truth, records), what)
    return records, res


def test_device_made_maps_scored_both_ways(ctx):
    rng = np.random.default_rng(2210)
    found = diverged = 0
    for i in range(40):
        fams = [(int(rng.integers(40, 160)), int(rng.integers(2, 5)), float(rng.choice([0.0, 0.02, 0.06]))) for _ in range(int(rng.integers(1, 4)))]
        g, T = repeat_accuracy.planted_repeats(int(rng.integers(2500, 4000)), fams, 5000 + i)
        pat = O.get_seed(9 + i % 7, 0)
        records, res = resident_and_list(ctx, g, T, pat, i)
        t = res["totals"]
        found += t["sp_truepos"] > 0
        diverged += t["sp_exact"] < t["sp_truepos"]
    assert found == 40 and diverged >= 1                       # (liveness of the inputs: ungapped matches end at most indels, one bridges one)


def test_equal_start_groups_follow_the_fetch(ctx):
    """three records with the same start 0, multiplicities 2, 2 and 3: the per-record tables are in the order the fetch finishes"""
    pat = O.get_seed(15, 0)
    c = MC.order_ties(pat)
    L = 6 * O.seed_length(pat)
    want = c.reference(pat)
    a = [r for r in want if len(r[1]) == 3][0][1]
    tie = [r for r in want if r[1][0] == a[0]]
    assert [len(r[1]) for r in tie] == [2, 2, 3]
    T = RC.truth_of([{g: (int(a[g]), 0, "x" * L) for g in range(3)}], 3)
    records, res = resident_and_list(ctx, c.codes, T, pat, "ties")
    assert MR.from_csr(*records) == want
    k = want.index(tie[0])
    assert res["comp_hit"][k:k + 3].tolist() == [3, 3, 7] and res["totals"]["sp_exact"] == 3 * L


def test_empty_map_and_empty_truth(ctx):
    c = RC.CASES["hand3"]
    none = RC.csr([])
    ctx.score_truth(c["truth"])
    got = ctx.repeat_score(none)
    same(got, SR.score(c["truth"], none))
    assert got["totals"] == dict(zip(SR.TOTALS, (30, 0, 0, 0, 0, 0, 0, 0))) and got["comp_hit"].shape == (0,)
    empty = dict(left=np.zeros((0, 3), np.int64), right=np.zeros((0, 3), np.int64), reverse=np.zeros((0, 3), np.int8), col_off=np.zeros(1, np.int64),
                 cols=np.zeros(0, np.uint32))
    ctx.score_truth(empty)
    got = ctx.repeat_score(c["records"])
    same(got, SR.score(empty, c["records"]))
    assert got["totals"] == dict(zip(SR.TOTALS, (0, 0, 0, 3, 0, 3, 0, 0)))
    same(ctx.repeat_score(none), SR.score(empty, none))
    # the totals alone
    ctx.score_truth(c["truth"])
    got = ctx.repeat_score(c["records"], want=())
    assert got["totals"] == c["totals"] and got["pair_records"] is None and got["comp_hit"] is None and got["pair_hit"] is None


def test_refusals(ctx):
    c = RC.CASES["hand3"]
    length, mult, off, st = c["records"]
    fresh = _lib.Context(0)
    try:
        with pytest.raises(RuntimeError, match=r"mauve_repeat_score failed \(-5\): repeat_score: no correct alignment"):
            fresh.repeat_score(c["records"])
        fresh.score_truth(c["truth"])
        with pytest.raises(RuntimeError, match=r"mauve_repeat_score failed \(-5\): repeat_score: no repeat result in force"):
            fresh.repeat_score()
        assert fresh.repeat_score(c["records"])["totals"] == c["totals"]           # no genomes are needed
        g = MC.order_ties(O.get_seed(15, 0)).codes
        fresh.set_genomes([g])
        fresh.repeat_matches(0, O.get_seed(15, 0))
        assert fresh.repeat_score()["totals"]["components"] > 0
        fresh.set_genomes([g])                                                      # an upload ends the repeat result
        with pytest.raises(RuntimeError, match=r"\(-5\): repeat_score: no repeat result in force"):
            fresh.repeat_score()
    finally:
        fresh.close()
    ctx.score_truth(c["truth"])
    two = RC.csr([(10, (101, -201, 301)), (5, (11, 21))])

    def bad(records, code, text, row_offset=None):
        with pytest.raises(RuntimeError, match=r"mauve_repeat_score failed \(%d\): repeat_score: %s" % (code, text)):
            ctx.repeat_score(records, row_offset)

    for m in (1, 0, 33, -2):
        bad((two[0], np.array([3, m]), two[2], two[3]), -1, r"record 1 has multiplicity %d outside \[2, 32\]" % m)
    bad((two[0], two[1], np.array([0, 2, 5]), two[3]), -1, "record 1: start_off is not the prefix sum of mult")
    bad((two[0], two[1], np.array([1, 4, 5]), two[3]), -1, "record 0: start_off is not the prefix sum of mult")
    st0 = two[3].copy()
    st0[4] = 0
    bad((two[0], two[1], two[2], st0), -1, r"record 1 has a zero start \(component 1\)")
    bad((np.array([10, 0]), two[1], two[2], two[3]), -1, "record 1 has a length below 1")
    bad((np.array([-1, 5]), two[1], two[2], two[3]), -1, "record 0 has a length below 1")
    bad(two, -1, "row_offset of row 2 is negative", row_offset=[0, 0, -1])
    big = two[3].copy()
    big[3] = (1 << 31) - 4                                                       # 5 bases from there: the last is 2^31
    bad((two[0], two[1], two[2], big), -4, "a position of 2\\^31 or more")
    big[3] = -(1 << 31)
    bad((two[0], two[1], two[2], big), -4, "a position of 2\\^31 or more")
    bad(two, -4, "a position of 2\\^31 or more", row_offset=[0, 1 << 31, 0])
    bad(two, -4, "a position of 2\\^31 or more", row_offset=[0, 0, (1 << 31) - 305])          # row 2 reaches 2^31 with its offset
    assert ctx.repeat_score(two, [0, 0, (1 << 31) - 311])["totals"]["sp_possible"] == 30    # ... and stays below it
    n = (1 << 24) + 1
    bad((np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n + 1, np.int64), np.zeros(0, np.int64)), -4, "more than 2\\^24 records")
    # the boundary itself: NULL totals, a resident call with list arrays, a list without its arrays
    L, h = ctx.L, ctx.h
    tot = _lib.RepeatScoreTotals()
    p = [C.c_void_p(a.ctypes.data) for a in c["records"]]
    assert L.mauve_repeat_score(h, C.c_int64(1), *p, None, None, None, None, None) == -1
    assert L.mauve_repeat_score(h, C.c_int64(1), None, p[1], None, None, None, C.byref(tot), None, None, None) == -1
    assert L.mauve_repeat_score(h, C.c_int64(1), p[0], None, p[2], p[3], None, C.byref(tot), None, None, None) == -1
    assert L.mauve_repeat_score(h, C.c_int64(-1), *p, None, C.byref(tot), None, None, None) == -1
    assert L.mauve_repeat_score(h, C.c_int64(1), *p, None, C.byref(tot), None, None, None) == 0 and tot.sp_exact == 30
    assert ctx.repeat_score(c["records"])["totals"] == c["totals"]                  # a refusal leaves the truth usable


def test_the_call_leaves_other_results_alone(ctx):
    pat = O.get_seed(11, 0)
    g, T = repeat_accuracy.planted_repeats(4000, [(200, 3, 0.03), (120, 2, 0.0)], 31)
    aln = RC.CASES["absent_row"]["truth"]
    ctx.set_genomes([g])
    records = ctx.repeat_matches(0, pat)
    ctx.coord_index_alignment(aln["left"], aln["right"], aln["reverse"], aln["col_off"], aln["cols"])
    ctx.map_ranges([0, 1, 2], [101, 190, 1], [120, 520, 700])
    pieces = ctx.map_ranges_fetch()
    cols = ctx.seqpos_to_column([0, 1, 2], [105, 503, 603])
    ctx.score_truth(T)
    first = ctx.repeat_score()
    assert first["totals"]["sp_truepos"] > 0
    ctx.repeat_score(RC.CASES["walk_back"]["records"])
    # the repeat result, the index in force, the range map and the truth are what they were
    n = len(records[0])
    again = [np.zeros_like(a) for a in records]
    ctx._chk(ctx.L.mauve_repeat_fetch(ctx.h, *[a.ctypes.data_as(C.POINTER(C.c_int64)) for a in again]), "mauve_repeat_fetch")
    assert n > 0 and all(np.array_equal(a, b) for a, b in zip(again, records))
    assert ctx.coord_index_size() == (3, 2, len(aln["cols"]))
    assert all(np.array_equal(a, b) for a, b in zip(ctx.seqpos_to_column([0, 1, 2], [105, 503, 603]), cols))
    after = ctx.map_ranges_fetch()
    assert all(np.array_equal(after[k], pieces[k]) for k in pieces)
    ctx.coord_index_alignment(T["left"], T["right"], T["reverse"], T["col_off"], T["cols"])
    rec = ctx.score_alignment()                                # the truth against itself: no error of any kind
    assert rec[..., 0].sum() > 0 and not rec[..., 1:5].any()
    second = ctx.repeat_score()
    same(second, first)


def test_two_calls_and_both_kinds_of_memory_give_identical_bytes(ctx):
    c = RC.random_case(77, 6, 500, 60)
    ctx.score_truth(c["truth"])
    a = ctx.repeat_score(c["records"])
    b = ctx.repeat_score(c["records"])
    n, ns = len(c["records"][0]), len(c["records"][3])
    pin = dict(pair_records=_lib.pinned_empty((6, 6, 4), np.int64), comp_hit=_lib.pinned_empty((n,), np.uint32), pair_hit=_lib.pinned_empty((ns,), np.uint32))
    for v in pin.values():
        v[...] = 0x55
    plist = []
    for arr in c["records"]:
        q = _lib.pinned_empty(arr.shape, np.int64)
        q[...] = arr
        plist.append(q)
    d = ctx.repeat_score(tuple(plist), out=pin)
    assert a["totals"] == b["totals"] == d["totals"] and a["totals"]["sp_truepos"] > 0
    for k in ("pair_records", "comp_hit", "pair_hit"):
        assert d[k] is pin[k] and a[k].tobytes() == b[k].tobytes() == d[k].tobytes(), k
    same(a, SR.score(c["truth"], c["records"]))
    with pytest.raises(ValueError):
        ctx.repeat_score(c["records"], out=dict(comp_hit=np.zeros(n + 1, np.uint32)))


def test_repeat_score_mirror():
    """tests/cpp/repeat_score_test.cpp: HipRepeatScore on the hand case in both coordinate forms, a wrong strand, an empty list"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "repeat_score_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "repeat_score_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
