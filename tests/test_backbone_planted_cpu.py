"""The planted alignments of the backbone stage (tests/backbone_planted.py) without a GPU: the reference of
tests/backbone_ref.py is pinned by hand cases with their numbers written out and by the oracle on random alignments; every planted
case is shown, from the reference's facts alone, to be where it was aimed (the aim is the assert message); the oracle is held to the
reference on every case; and the families "components" and "coordinates" go through the stage's host steps (the stand-alone program of
tests/test_backbone_host_cpu.py).  Integers throughout: every comparison is exact, shapes and dtypes included."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import backbone_cases as BC, backbone_planted as P, backbone_ref as R
from tests.test_backbone_host_cpu import OFF, host_tables, program  # noqa: F401 (the fixture that builds the host-step program)


def same(r, e, what):
    diff = R.first_difference(r, e)
    assert diff is None, (what, diff)


@functools.lru_cache(maxsize=None)
def reference(name, gap):
    c = next(c for c in P.all_cases() if c["name"] == name)
    return R.backbone(*c["aln"], island_gap=gap)


def _cols_of(rows):
    """presence masks of alignment rows written as text ('-' is a gap)"""
    cols = np.zeros(len(rows[0]), np.uint32)
    for g, r in enumerate(rows):
        cols |= (np.frombuffer(r.encode(), np.uint8) != ord("-")).astype(np.uint32) << np.uint32(g)
    return cols


def test_reference_known_answers():
    """the six hand cases of the oracle's known-answer test (tests/test_oracle.py: test_backbone_oracle_known_answers), numbers written out,
    and two more"""
    aln = BC.hand_case()
    r = R.backbone(*aln, island_gap=3)
    assert r["seg_iv"].tolist() == [0, 0, 0] and r["seg_mask"].tolist() == [7, 5, 7] and r["seg_col"].tolist() == [0, 10, 15] and r["seg_len"].tolist() == [10, 5, 5]
    assert r["seg_left"].tolist() == [[1, 101, -211], [11, 0, -206], [16, 111, -201]]
    assert r["seg_right"].tolist() == [[10, 110, -220], [15, 0, -210], [20, 115, -205]]
    assert r["islands"].tolist() == [[0, 0, 1, 0, 10, 14, 11, 15], [0, 1, 2, 2, 10, 14, -206, -210]]
    r = R.backbone(*aln, island_gap=5)
    assert r["seg_mask"].tolist() == [7] and r["seg_col"].tolist() == [0] and r["seg_len"].tolist() == [20] and r["islands"].shape == (0, 8)
    assert r["seg_left"].tolist() == [[1, 101, -201]] and r["seg_right"].tolist() == [[20, 115, -220]]
    # ends: a pair is not joined before its first / after its last common column, however short the overhang
    cols = _cols_of(["xxxxxxxx--", "--xxxxxxxx"])
    r = R.backbone(np.array([[1, 1]]), np.array([[8, 8]]), np.zeros((1, 2), np.int8), [0, 10], cols, island_gap=20)
    assert r["seg_col"].tolist() == [2] and r["seg_len"].tolist() == [6] and r["seg_left"].tolist() == [[3, 1]] and r["seg_right"].tolist() == [[8, 6]]
    assert r["seg_mask"].tolist() == [3] and len(r["islands"]) == 0
    # two short one-sided runs of different genomes in a row are two runs, not one: no island at gap 3, both at gap 2
    cols = _cols_of(["xx" + "xxx" + "---" + "xx", "xx" + "---" + "xxx" + "xx"])
    lr = (np.array([[1, 1]]), np.array([[7, 7]]), np.zeros((1, 2), np.int8), [0, 10], cols)
    r = R.backbone(*lr, island_gap=3)
    assert r["seg_len"].tolist() == [10] and len(r["islands"]) == 0
    r = R.backbone(*lr, island_gap=2)
    assert r["seg_col"].tolist() == [0, 8] and r["islands"][:, 3:6].tolist() == [[0, 2, 4], [1, 5, 7]]
    # 0-1 share the first half, 1-2 the second, 0-2 never a column: two components, one after the other
    cols = _cols_of(["xxxx----", "xxxxxxxx", "----xxxx"])
    r = R.backbone(np.array([[1, 1, 1]]), np.array([[4, 8, 4]]), np.zeros((1, 3), np.int8), [0, 8], cols, island_gap=20)
    assert r["seg_mask"].tolist() == [3, 6] and r["seg_col"].tolist() == [0, 4]
    # columns neither genome of a pair has are skipped: the run of 0 against 1 is 4 + 4 columns around genome 2's insert
    cols = _cols_of(["xx" + "xxxx" + "---" + "xxxx" + "xx", "xx" + "----" + "---" + "----" + "xx", "xx" + "----" + "xxx" + "----" + "xx"])
    r = R.backbone(np.array([[1, 1, 1]]), np.array([[12, 4, 7]]), np.zeros((1, 3), np.int8), [0, 15], cols, island_gap=7)
    assert [row[1:6] for row in r["islands"].tolist() if row[1:3] == [0, 1]] == [[0, 1, 0, 2, 12]]
    assert [(x["first"], x["last"], x["n"]) for x in r["facts"][(0, 0, 1)]["runs"]] == [(2, 12, 8)]
    # one more, not among the oracle's: 0-1 and 1-2 joined, 0 and 2 never in one column, alternating
    left, right, rev = np.array([[1, 1, 1]]), np.array([[4, 8, 4]]), np.zeros((1, 3), np.int8)
    r = R.backbone(left, right, rev, [0, 8], np.array([3, 6, 3, 6, 3, 6, 3, 6], np.uint32), island_gap=3)
    # (column 0 is a leading region of 1-2, column 7 a trailing one of 0-1)
    assert r["seg_mask"].tolist() == [3, 7, 6] and r["seg_col"].tolist() == [0, 1, 7] and r["seg_len"].tolist() == [1, 6, 1]
    assert r["seg_left"].tolist() == [[1, 1, 0], [2, 2, 1], [0, 8, 4]] and r["seg_right"].tolist() == [[1, 1, 0], [4, 7, 3], [0, 8, 4]] and len(r["islands"]) == 0
    # an interval of one genome, and no interval
    r = R.backbone(np.array([[1, 0]]), np.array([[5, 0]]), np.zeros((1, 2), np.int8), [0, 5], np.full(5, 1, np.uint32))
    assert r["seg_iv"].shape == (0,) and r["seg_left"].shape == (0, 2) and r["islands"].shape == (0, 8)


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_equals_oracle_on_random_alignments(seed):
    aln = BC.random_case(seed)
    for gap in (0, 3, 20):
        e = O.backbone(*aln, island_gap=gap)
        same(R.backbone(*aln, island_gap=gap), e, (seed, gap))
    assert len(e["seg_iv"]) > 0 and len(e["islands"]) > 0


def check(c, gap, chk, r):
    """one aim of a case, from the reference's facts and tables"""
    kind, why = chk[0], (c["name"], gap, chk[-1])
    off = c["aln"][3]
    if kind == "run":
        _, iv, a, b, first, last, n, island, _ = chk
        got = [x for x in r["facts"][(iv, a, b)]["runs"] if x["first"] == first]
        assert len(got) == 1 and (got[0]["last"], got[0]["n"], got[0]["island"]) == (last, n, island), why + (got,)
    elif kind == "region":
        _, iv, a, b, first, last, is_open, reasons, _ = chk
        got = [x for x in r["facts"][(iv, a, b)]["regions"] if x["first"] == first]
        assert len(got) == 1 and (got[0]["last"], got[0]["open"], got[0]["why"]) == (last, is_open, tuple(sorted(reasons))), why + (got,)
        rows = r["islands"][(r["islands"][:, 0] == iv) & (r["islands"][:, 1] == a) & (r["islands"][:, 2] == b)]
        assert ("island" in reasons) == bool(np.any((rows[:, 4] >= first) & (rows[:, 5] <= last))), why
    elif kind == "regions":
        _, iv, a, b, count, _ = chk
        assert len(r["facts"][(iv, a, b)]["regions"]) == count, why
    elif kind == "chunks":
        _, iv, a, b, first, span, _ = chk
        got = [x for x in r["facts"][(iv, a, b)]["regions"] if x["first"] == first]
        assert len(got) == 1 and got[0]["last"] // P.CHUNK - first // P.CHUNK + 1 == span, why
    elif kind == "masks":
        _, iv, col, masks, _ = chk
        assert R.masks_at(r, iv, col) == sorted(masks), why + (R.masks_at(r, iv, col),)
    elif kind == "pair_islands":
        _, iv, a, b, count, _ = chk
        rows = r["islands"]
        assert int(np.count_nonzero((rows[:, 0] == iv) & (rows[:, 1] == a) & (rows[:, 2] == b))) == count, why
        assert sum(x["island"] for x in r["facts"][(iv, a, b)]["runs"]) == count, why
    elif kind == "islands":
        assert len(r["islands"]) == chk[1], why + (len(r["islands"]),)
    elif kind == "segments":
        assert len(r["seg_iv"]) == chk[1], why + (len(r["seg_iv"]),)
    elif kind == "edge":
        _, what, end, col, _ = chk
        if what == "seg":
            first = off[r["seg_iv"]] + r["seg_col"]
            ends = first if end == "first" else first + r["seg_len"] - 1
        else:
            ends = off[r["islands"][:, 0]] + r["islands"][:, 4 if end == "first" else 5]
        assert col in ends.tolist(), why
    else:
        raise AssertionError(("unknown check", chk))


@pytest.mark.parametrize("fam", P.FAMILIES)
def test_every_case_is_where_it_was_aimed(fam):
    cases = P.family(fam)
    assert cases
    for c in cases:
        assert c["gaps"] and all(c["aim"][g] for g in c["gaps"]), c["name"]
        assert c.get("sequence") in (None, c["gaps"]), (c["name"], "island_gap g and then g + 1, in this order")
        assert (c.get("sequence") is not None) == c["name"].startswith(("limit_word_", "limit_border_", "limit_holes_")), c["name"]
        for gap in c["gaps"]:
            r = reference(c["name"], gap)
            for chk in c["aim"][gap]:
                check(c, gap, chk, r)


def test_the_cases_cover_what_they_are_for():
    """the geometry the families are built around: every island limit at every placement, the borders, the look-back distances"""
    names = {c["name"] for c in P.all_cases()}
    for g in P.LIMITS:
        assert {"limit_border_g%d" % g, "limit_holes_g%d" % g} <= names and ("limit_word_g%d" % g in names) == (g <= 61) and ("limit_two_runs_g%d" % g in names) == (g > 0)
    for k in (1, 63, 64, 65):
        c = next(c for c in P.all_cases() if c["name"] == "start_back_%d_one_one" % k)
        m = c["aln"][4]
        assert not np.any(m[P.CHUNK:(k + 1) * P.CHUNK] & 3) and m[(k + 1) * P.CHUNK] & 3 == 1 and np.any(m[:P.CHUNK] & 3), (k, "chunks without a column of the pair")
    big = max(len(c["aln"][4]) for c in P.all_cases())
    assert 66 * P.CHUNK < big < 68 * P.CHUNK                 # the largest case: 65 empty chunks between two others
    for c in P.family("coordinates"):
        assert len(c["aln"][4]) % P.CHUNK == 0 and c["aln"][3][1] % P.CHUNK in (1, 4095, 0), c["name"]
    assert {tuple(c["aln"][2][1].tolist()) for c in P.family("coordinates")} == {(0, 0), (1, 0), (0, 1), (1, 1)}


@pytest.mark.parametrize("fam", P.FAMILIES)
def test_oracle_equals_reference_on_every_case(fam):
    for c in P.family(fam):
        for gap in c["gaps"]:
            same(O.backbone(*c["aln"], island_gap=gap), reference(c["name"], gap), (c["name"], gap))


@pytest.mark.parametrize("fam", ["components", "coordinates"])
def test_host_steps_on_the_planted_cases(program, tmp_path, fam):  # noqa: F811
    """what the kernels would hand the host, made by the program's plain column walk, through bb_sort_records, bb_sweep, bb_query_slots and
    bb_tables: the tables are the reference's"""
    for c in P.family(fam):
        for gap in c["gaps"]:
            t, slots, made = host_tables(program, tmp_path, c["aln"], gap, OFF)
            same(t, reference(c["name"], gap), (c["name"], gap))
            assert made == slots
