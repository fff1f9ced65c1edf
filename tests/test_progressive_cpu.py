"""The progressive path's plain reference (tests/progressive_ref.py) held to the CPU oracle on every planted case of
tests/progressive_cases.py, the planted-anchor guarantee of the refinement sets, and the liveness of the cases: a deliberately wrong
variant of the rule a case aims at must give another answer on it.  No GPU."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import progressive_cases as Cs
from tests import progressive_ref as R

TREES = {c["name"]: c for c in Cs.tree_sets()}
BPS = {c["name"]: c for c in Cs.bp_sets()}
WALKS = {c["name"]: c for c in Cs.walk_sets()}
REFSETS = {c["name"]: c for c in Cs.refinement_sets()}


def same_tree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_planted_seed_is_the_table_s():
    assert O.get_seed(11, 0) == Cs.P11 and O.seed_length(Cs.P11) == Cs.SPAN and O.seed_weight(Cs.SOLID11) == 11


# ------------------------------------------------------------------------------------------------------------- guide tree (S9)
@pytest.mark.parametrize("name", list(TREES))
def test_guide_tree_reference_equals_oracle(name):
    c = TREES[name]
    gs, N = c["genomes"], len(c["genomes"])
    rec = R.pair_records(gs, c["pattern"])
    dist = R.distances(gs, rec)
    tree = R.upgma(dist)
    odist, oleft, oright = O.guide_tree(gs, c["pattern"])
    assert np.array_equal(dist, odist) and same_tree(tree, (oleft, oright))
    if c["merges"] is not None:
        assert same_tree(tree, Cs.tree_of(N, c["merges"]))
    wrong = {"ties_high": lambda: R.upgma(dist, "ties_high"), "round": lambda: R.upgma(dist, "round"),
             "longer": lambda: R.upgma(R.distances(gs, rec, "longer"))}
    for v in c["moved_by"]:
        assert not same_tree(tree, wrong[v]()), (name, v)
    if name == "identical4":
        assert not dist.any()
    if name == "unrelated":
        assert np.all(dist[2:, :2] == 1000000) and dist[2, 3] == 1000000 and 0 < dist[0, 1] < 1000000
    if name == "fractions5":
        for (a, b), d in c["dist"].items():
            assert dist[a, b] == d, (a, b, int(dist[a, b]))
        assert any(num % den for num, den in R.upgma_means(dist))
    if name == "lengths_2k_20k":
        assert not np.array_equal(dist, R.distances(gs, rec, "longer")) and sorted(len(g) for g in gs) == [2000, 20000, 20000]
    if name == "thirty_two":
        assert N == 32 and dist[28, 26] == 0 and np.all(dist[31, :31] == 1000000)


def test_node_factor_by_hand():
    """S11b / S11c on a three-leaf tree ((0,1),2): c = floor((300001 + 500000) / 2) = 400000, factor = 10^6 - floor(0.5 * 400000) = 800000;
    b = floor((10^6 + 333333) / 2) = 666666, f2 = 10^6 - 333333 = 666667, product floor(800000 * 666667 / 10^6) = 533333"""
    dist = np.array([[0, 100000, 300001], [100000, 0, 500000], [300001, 500000, 0]])
    bpd = R.bp_distance(np.array([[0, 0, 3], [0, 0, 1], [3, 1, 0]]))
    assert bpd[0, 2] == 1000000 and bpd[1, 2] == 333333
    assert R.node_factor(Cs.TREE3, 4, dist, None, 500000) == 800000
    assert R.node_factor(Cs.TREE3, 4, dist, bpd, 500000, 500000) == 533333
    assert R.node_factor(Cs.TREE3, 3, dist, bpd, 500000, 500000) == 950000
    assert R.node_factor(Cs.TREE3, 4, dist * 3, None, 1000000) == 0          # (clamped at 0)
    assert R.scaled_weight(99, 533333) == 52 and R.scaled_weight(99, 0, 7) == 7
    assert not R.bp_distance(np.zeros((3, 3), np.int64)).any()


# ------------------------------------------------------------------------------------------------------ breakpoint counts (S11c)
@pytest.mark.parametrize("name", list(BPS))
def test_breakpoint_reference_equals_oracle(name):
    c = BPS[name]
    gs, N = c["genomes"], len(c["genomes"])
    rec = R.pair_records(gs, c["pattern"])
    moved = set()
    for min_len, want in c["runs"]:
        bp = R.breakpoint_counts(rec, N, min_len)
        assert np.array_equal(bp, O.breakpoint_counts(gs, c["pattern"], min_len)), (name, min_len)
        for (a, b), v in want.items():
            assert bp[a, b] == v and bp[b, a] == v, (name, min_len, a, b, int(bp[a, b]))
        for v in c["moved_by"]:
            if not np.array_equal(bp, R.breakpoint_counts(rec, N, min_len, v)):
                moved.add(v)
        if "counted" in c:
            for (a, b), k in c["counted"].items():
                assert len(R.bp_sorted(rec, a, b, min_len)) == k, (name, a, b)
        if "counted_by_floor" in c:
            assert len(R.bp_sorted(rec, 0, 1, min_len)) == c["counted_by_floor"][min_len]
        if c.get("all_reverse"):
            s = R.bp_sorted(rec, 0, 1, min_len)
            assert len(s) == 12 and all(x[2] == 1 for x in s)
        if "past" in c:
            assert max(x[0] for x in R.bp_sorted(rec, 0, 1, min_len)) > 4000 and max(len(g) for g in gs) in (4095, 4096)
    assert moved == set(c["moved_by"]) and moved, (name, moved)


def test_breakpoint_sweep_with_duplications():
    """small pairs with duplicated, mutated segments: records overlap, and at Cs.DUP_SEED two counted records start at the same base of the
    lower genome, so the order along it is settled by (position in b, strand in b)"""
    assert Cs.DUP_SEED is not None and Cs.same_start_in_a(Cs.dup_pair(Cs.DUP_SEED), 22)
    for seed in range(Cs.DUP_SEED, Cs.DUP_SEED + 24):
        gs = Cs.dup_pair(seed)
        rec = R.pair_records(gs, Cs.P11)
        for min_len in (0, 22):
            assert np.array_equal(R.breakpoint_counts(rec, 2, min_len), O.breakpoint_counts(gs, Cs.P11, min_len)), (seed, min_len)


# ------------------------------------------------------------------------------------------------------------ refinement (S13)
def all_stretches():
    out = []
    for c in Cs.refinement_sets():
        out += [(c["name"], i, st) for i, st in enumerate(c["stretches"])]
    cl = Cs.clade_set()
    out += [("clade_root", i, st) for i, st in enumerate(cl["rst"])] + [("clade_node", i, st) for i, st in enumerate(cl["cst"])]
    return out


def test_refine_interval_equals_oracle():
    """every planted stretch at every number of rounds: columns, DP score and the objective of every rotation"""
    for name, i, st in all_stretches():
        k = sum(1 for s in st if len(s))
        if k < 2:
            continue
        for rounds in (0,) + Cs.ROUNDS:
            cols, score, win, obj = Cs.refined(st, rounds)
            ocols, oscore, _ = O.align_interval_refined(st, rounds)
            assert np.array_equal(cols, ocols) and score == oscore, (name, i, rounds)
            assert O.sp_score_cols(st, cols) == obj[win] == max(obj)
            assert len(obj) == 1 + (min(rounds, k - 1) if k >= 3 else 0)
        nz = [s for s in st if len(s)]
        for r in range(1, k if k >= 3 else 1):                                  # the objective of every rotation, on the rotated sequences
            rot = [nz[(j + r) % k] for j in range(k)]
            rc, _ = O.align_interval(rot)
            assert O.sp_score_cols(rot, rc) == Cs.refined(st, 9)[3][r], (name, i, r)


def test_the_planted_stretches_reach_their_rules():
    n3 = REFSETS["n3"]
    w = {r: Cs.expect_refinement(n3, r)["winners"] for r in Cs.ROUNDS}
    assert w[9][:6] == [0, 0, 1, None, 2, 0] and w[2][:6] == w[9][:6] and w[1][4] in (0, 1)     # rotation 2 wins only from two rounds on
    assert [sum(1 for s in st if len(s)) for st in n3["stretches"][:6]] == [3, 2, 3, 1, 3, 2]   # k = 2 and k = 1 between k = 3: cbase entries without candidates
    # the tie: the lowest rotation is kept, and the highest would give other columns
    tie = n3["stretches"][n3["tie"]]
    cols, _, win, obj = Cs.refined(tie, 9)
    best = [r for r, o in enumerate(obj) if o == max(obj)]
    assert len(best) >= 2 and win == best[0]
    assert not np.array_equal(cols, Cs.refined(tie, 9, "ties_high")[0])
    # the 64-column edges of the objective kernel, on the kept alignment at every number of rounds
    for (nm, seed, L, o, t, what), idx in zip(Cs.LAYOUTS, n3["layouts"]):
        for rounds in Cs.ROUNDS:
            p01, p02 = Cs.layout_of(n3["stretches"][idx], rounds)
            assert p01 == "B" * o + "b" * t + "B" * (L - o) and p02 == "B" * o + "." * t + "B" * (L - o), nm
    lay = {nm: (L, o, t) for nm, seed, L, o, t, what in Cs.LAYOUTS}
    assert lay["cross_63_64"][1] <= 63 and sum(lay["cross_63_64"][1:]) > 64 and lay["cross_63_64"][0] + lay["cross_63_64"][2] == 128
    assert lay["cross_127_128"][1] <= 127 and sum(lay["cross_127_128"][1:]) > 128
    assert lay["start_64"][1] == 64 and sum(lay["end_63"][1:]) == 64
    assert lay["cols_64"][0] + lay["cols_64"][2] == 64 and lay["cols_65"][0] + lay["cols_65"][2] == 65
    # four and five sequences: every rotation wins somewhere; slots {0,2,3} and {1,2,4}
    assert {x for x in Cs.expect_refinement(REFSETS["n4"], 9)["winners"] if x is not None} == {0, 1, 2, 3}
    n5 = REFSETS["n5"]
    assert Cs.expect_refinement(n5, 9)["winners"] == [1, 0, 2, None, 0, 4, 1, 2] and Cs.expect_refinement(n5, 2)["winners"][5] != 4
    slots = [tuple(g for g in range(5) if len(st[g])) for st in n5["stretches"]]
    assert slots.count((0, 2, 3)) == 2 and slots.count((1, 2, 4)) == 2


def progressive(case, **kw):
    p = dict(case["params"])
    p.update(kw)
    return O.progressive_align(case["genomes"], O.default_params(**p), tree=case["tree"])


def same_alignment(res, want):
    return all(np.array_equal(res[k], want[k]) for k in ("left", "right", "col_off", "cols", "dp_score")) and not np.any(res["reverse"][:len(want["left"])])


@pytest.mark.parametrize("name", list(REFSETS))
def test_refinement_sets_against_oracle(name):
    c = REFSETS[name]
    e = O.align(c["genomes"], O.default_params(seed_weight=11, recursive=0, extend_lcbs=0))["aln"]     # the root is the Aligner::align path (S9)
    assert [(int(l), tuple(int(x) for x in s)) for l, s in zip(e["anchor_length"], e["anchor_start"])] == c["anchors"]
    for rounds in Cs.ROUNDS:
        r = progressive(c, refine_rounds=rounds)
        assert same_alignment(r["aln"], Cs.expect_refinement(c, rounds)), (name, rounds)
        R.check_walk(c["genomes"], r["tree"], r["aln"])
    if c.get("tie") is not None:
        assert not np.array_equal(Cs.expect_refinement(c, 9)["cols"], Cs.expect_refinement(c, 9, "ties_high")["cols"])


def test_clade_set_against_oracle():
    c = Cs.clade_set()
    e = O.align(c["genomes"], O.default_params(seed_weight=11, recursive=0, extend_lcbs=0))["aln"]
    assert [int(l) for l in e["anchor_length"]] == [len(b) for b in c["rb"]]
    for rounds in Cs.ROUNDS:
        r = progressive(c, refine_rounds=rounds)
        want = Cs.expect_clade(c, rounds)
        assert same_alignment(r["aln"], want), rounds
        R.check_walk(c["genomes"], c["tree"], r["aln"])
    assert Cs.expect_clade(c, 9)["winners"] == [1, 2, 2, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- the walk (S9)
@pytest.mark.parametrize("name", list(WALKS))
def test_walk_sets_against_oracle(name):
    c = WALKS[name]
    r = progressive(c)
    R.check_walk(c["genomes"], r["tree"], r["aln"])
    table = R.interval_table(r["aln"], multi_only=False)
    if c["table"] is not None:
        assert table == c["table"], table
        for v, t in c["wrong"].items():
            assert t != c["table"], (name, v)
    if "root_anchors" in c:                      # the stretch between the planted anchors is as long as the case says
        p = dict(c["params"], extend_lcbs=0)
        assert O.align(c["genomes"], O.default_params(**p))["aln"]["anchor_length"].tolist() == c["root_anchors"]
    if name == "thirty_two_balanced":
        sets = [t[0] for t in table]
        assert tuple(range(16, 32)) in sets and tuple(range(32)) in sets
        assert int(r["aln"]["cols"].max()) >> 31 == 1 and r["aln"]["n_gap_dp"] >= 17
        assert r["aln"]["dp_score"][sets.index(tuple(range(16, 32)))] != 0                    # sixteen-sequence stretches were aligned at that node


def test_check_walk_notices():
    """check_walk on a correct result passes (above); each rule it states trips on a result broken in that one way"""
    c = WALKS["chain_cut"]
    good = progressive(c)["aln"]
    tree = c["tree"]

    def broken(**kw):
        a = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, f in kw.items():
            f(a[k])
        return a

    for bad in (broken(right=lambda x: x.__setitem__((0, 0), x[0, 0] - 1)),                       # a base in no interval, bits and extent differ
                broken(left=lambda x: x.__setitem__((3, 0), x[3, 0] - 1)),                        # a base in two intervals
                broken(cols=lambda x: x.__setitem__(0, 3))):                                      # a column bit too few
        with pytest.raises(AssertionError):
            R.check_walk(c["genomes"], tree, bad)
    order = [3, 0, 1, 2, 4]                                                                       # a child's interval in front of the root's
    a = dict(good)
    a["left"], a["right"] = good["left"][order], good["right"][order]
    sizes = np.diff(good["col_off"])[order]
    a["col_off"] = np.concatenate(([0], np.cumsum(sizes)))
    a["cols"] = np.concatenate([good["cols"][good["col_off"][i]:good["col_off"][i + 1]] for i in order])
    with pytest.raises(AssertionError, match="pre-order"):
        R.check_walk(c["genomes"], tree, a)
    with pytest.raises(AssertionError, match="no node"):                                          # (0, 1) is no node of ((0, 2), 1)
        R.check_walk(c["genomes"], Cs.tree_of(3, [(0, 2), (1, 3)]), good)
