"""The chain stage's planted cases (tests/chain_cases.py) without a GPU: the oracle (orc_eliminate_overlaps, orc_compute_lcbs) and
the host chain (mauve_eliminate_overlaps, mauve_lcb_chain: chain_host.cpp, what the device chain falls back to) are held to the
restatement of DESIGN.md S5 in tests/chain_ref.py on every case, and every case is shown to be where it was aimed: a cluster
over the tile edge, a cluster of exactly 48 or 49, a workgroup that outgrows its LDS pool, a tie that decides.  The liveness
assertions read chain_ref.input_facts and the reference's own result -- never a cluster size, a pass count or an order reported by
the product.  tests/test_gpu_chains.py runs the same cases through chain_dev.hip."""
import numpy as np
import pytest

from mauvealigner_amd import _lib
from oracle import pyoracle as O
from tests import chain_cases as C
from tests import chain_ref as R

FAMILIES = C.FAMILY_NAMES
_elim = {}
_facts = {}


def elim(case):
    if case["name"] not in _elim:
        _elim[case["name"]] = R.eliminate_overlaps(case["length"], case["start"])
    return _elim[case["name"]]


def facts(case):
    if case["name"] not in _facts:
        _facts[case["name"]] = R.input_facts(case["length"], case["start"])
    return _facts[case["name"]]


def _arr(x, N):
    return np.asarray(x, dtype=np.int64).reshape(len(x), N) if N else np.asarray(x, dtype=np.int64)


def test_the_host_chain_loads_without_a_gpu():
    ln, st = _lib.eliminate_overlaps([10, 10], [[100, 300], [105, 400]])
    assert ln.tolist() == [10, 5] and st.tolist() == [[100, 300], [110, 405]]


def test_canonical_order_is_by_the_signed_starts():
    """|start 0| first, then the SIGNED starts, then the length, then the index (canon_less, host_chain.hpp; match_cmp of the
    oracle): of two records with the same |start 0| the reverse one in genome 1 comes first"""
    ln, st = [5, 5, 7, 5], [[100, 300], [100, -900], [100, -900], [100, -900]]
    assert R.canonical_order(ln, st) == [1, 3, 2, 0]
    # the oracle leaves the survivors of an elimination in that order too
    ln, st = [4, 4, 4], [[300, 10], [200, -50], [100, 90]]
    ol, os_ = O.eliminate_overlaps(ln, st)
    assert os_.tolist() == [[100, 90], [200, -50], [300, 10]] == R.canonicalise(ln, st)[1]


def test_a_list_out_of_canonical_order_is_another_list_to_the_oracle():
    """Why tests/test_gpu_chain_upfront.py hands over canonicalised lists: the index that decides among equal left ends is the
    caller's order for the oracle and the canonical one for the product.  Two matches with the same genome-0 start: whichever comes
    later in the list dies."""
    a = ([10, 10], [[100, 300], [100, 500]])
    b = ([10, 10], [[100, 500], [100, 300]])
    assert O.eliminate_overlaps(*a)[1].tolist() == [[100, 300]] and O.eliminate_overlaps(*b)[1].tolist() == [[100, 500]]
    assert R.eliminate_overlaps(*R.canonicalise(*b))["start"] == [[100, 300]]


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_and_host_chain_equal_the_reference(family):
    for case in C.families()[family]:
        N, ln, st = case["N"], case["length"], case["start"]
        e = elim(case)
        want = (e["length"], e["start"])
        for who, f in (("oracle", O.eliminate_overlaps), ("host chain", _lib.eliminate_overlaps)):
            gl, gs = f(ln, _arr(st, N))
            assert gl.tolist() == want[0] and gs.tolist() == want[1], (case["name"], who, len(gl), len(want[0]))
        if not want[0]:
            continue
        for w, col in case["runs"]:
            lc = R.compute_lcbs(want[0], want[1], w, bool(col))
            for who, f in (("oracle", O.compute_lcbs), ("host chain", _lib.lcb_chain)):
                got = f(np.asarray(want[0], np.int64), _arr(want[1], N), w, bool(col))
                assert got["n_lcb"] == lc["n_lcb"], (case["name"], who, w, col)
                for k in ("match_lcb", "weight", "left_end", "right_end", "left_adj", "right_adj"):
                    assert np.asarray(got[k]).tolist() == lc[k], (case["name"], who, w, col, k)


def test_the_nodes_of_the_reference_are_its_lcbs_at_weight_zero():
    for case in C.families()["graph"]:
        nodes = R.lcb_nodes(case["length"], case["start"])
        lc = R.compute_lcbs(case["length"], case["start"], 0)
        assert [nd["weight"] for nd in nodes] == lc["weight"] and [nd["prev"] for nd in nodes] == lc["left_adj"]
        assert [nd["next"] for nd in nodes] == lc["right_adj"]
        assert [nd["orient"] for nd in nodes] == [sum(1 << g for g in range(case["N"]) if le[g] < 0) for le in lc["left_end"]]


# ---- liveness ---------------------------------------------------------------------------------------------------------------
def _left(case, i, g):
    return abs(case["start"][i][g])


def _right(case, i, g):
    return abs(case["start"][i][g]) + case["length"][i] - 1


def test_tile_cases_straddle_the_tile_edges():
    for case in C.families()["tile"][:-1]:
        f, aim, n = facts(case), case["aim"], len(case["length"])
        assert len({tuple(o) for o in f["order"]}) == case["N"]          # another permutation of the list for every genome
        for g, a, s in aim["spots"]:
            o = f["order"][g]
            if s is None:                                   # abuts: two clusters, right end = next left end - 1
                assert R.cluster_at(f, g, a)[0] == a and _right(case, o[a - 1], g) == _left(case, o[a], g) - 1, case["name"]
            else:
                assert R.cluster_at(f, g, a) == (a, s), (case["name"], g, a, s)
                assert all(_right(case, o[k], g) - _left(case, o[k + 1], g) + 1 == 1 for k in range(a, a + s - 1))
        for g in range(case["N"]):
            for b in aim["edges"]:                          # members at order positions b - 1 and b, or a cut exactly there
                a, s = R.cluster_at(f, g, b - 1)
                assert (a + s == b) if aim["kind"] == "abut" else (a + s > b), (case["name"], g, b)
            if aim["kind"] != "abut" or (g, n - 2, 2) in aim["spots"]:
                a, s = f["clusters"][g][-1]
                assert s >= 2 and a + s == n                # a cluster ends on the last entry of the list
        if any(s for _, _, s in aim["spots"]):
            assert elim(case)["cropped"], case["name"]
        assert max(s for g in range(case["N"]) for _, s in f["clusters"][g]) <= 3
    assert {len(c["length"]) for c in C.families()["tile"][:-1]} == {1023, 1024, 1025, 2047, 2048, 2049, 4097}


def test_the_long_match_has_its_cluster_start_two_tiles_back():
    case = C.families()["tile"][-1]
    f, g = facts(case), case["aim"]["genome"]
    a, s = R.cluster_at(f, g, case["aim"]["reach"])
    assert a == 0 and case["aim"]["reach"] >= 2 * C.TILE and a + s > 2 * C.TILE
    o = f["order"][g]
    tile_max = [max(_right(case, i, g) for i in o[t * C.TILE:(t + 1) * C.TILE]) for t in range(2)]
    assert tile_max[1] < tile_max[0]                        # tile 1's own maximum does not reach tile 2: tile 0's does
    assert tile_max[1] < _left(case, o[2 * C.TILE], g) <= tile_max[0]
    assert s > C.CL_MAX and not case["device"]


@pytest.mark.parametrize("family,limit", [("cluster", C.CL_MAX), ("cluster_cl5", 5)])
def test_cluster_cases_have_clusters_of_exactly_the_stated_sizes(family, limit):
    seen = set()
    for case in C.families()[family]:
        f, g = facts(case), case["aim"]["genome"]
        for a, s in case["aim"]["clusters"]:
            assert R.cluster_at(f, g, a) == (a, s), (case["name"], a, s)
            seen.add(s)
        for h in range(case["N"]):
            top = max(s for _, s in f["clusters"][h])
            if h != g:
                assert top <= 2, case["name"]               # only the aimed genome has them
        top = max(s for _, s in f["clusters"][g])
        assert top == max(s for _, s in case["aim"]["clusters"]) and case["device"] == (top <= limit), case["name"]
        assert elim(case)["dead"] and elim(case)["cropped"]
    assert {limit, limit + 1} <= seen and (limit != C.CL_MAX or limit - 1 in seen)


def test_pool_cases_outgrow_the_lds_pool_of_a_workgroup():
    for case in C.families()["pool"]:
        f, g = facts(case), case["aim"]["genome"]
        for a, s in case["aim"]["clusters"]:
            assert R.cluster_at(f, g, a) == (a, s)
        want = C.pool_demand(f, g)[0]                       # clusters 0 .. 255 of the genome: one workgroup
        assert sum(want) > C.POOL_WORDS and sum(want) // C.WORDS_PER_ENTRY > 1536, case["name"]
        # the first ones fit and take their slots in LDS, the ones behind them find the pool used up and take scratch -- whatever order
        # the threads arrive in, since all of them ask for the same amount
        assert len(set(want)) == 1 and want[0] <= C.POOL_WORDS < len(want) * want[0]
        assert max(s for h in range(case["N"]) for _, s in f["clusters"][h]) <= C.CL_MAX and case["device"]
        assert elim(case)["cropped"]
    assert C.POOL_WORDS % (C.WORDS_PER_ENTRY * 48) == 0     # 32 clusters of 48 fill the pool to the last word: the 32nd still fits


EXPECT_FORWARD = {          # survivors (length, start 0, start 1), worked out by hand from S5
    "tie0_equal_length": [(10, 100, 300)], "tie0_second_shorter": [(10, 100, 300)], "tie0_first_shorter": [(10, 100, 500)],
    "tie1_equal_length": [(10, 100, 300)], "tie1_first_shorter": [(12, 200, 300)], "duplicate": [(10, 100, 300)],
    "equal_length_overlap": [(10, 100, 300), (5, 110, 405)], "nested": [(20, 100, 300)],
    "both_sides_exact": [(10, 100, 300), (10, 110, 500)], "both_sides_one_left": [(10, 100, 300), (1, 110, 404), (10, 111, 500)],
    "hidden_overlap": [(30, 100, 900), (20, 500, 300), (15, 605, 320)],
}
EXPECT_REVERSE = {          # the same with genome 1 reverse: what leaves a match's first columns leaves its right end there
    "equal_length_overlap": [(10, 100, -300), (5, 110, -400)], "both_sides_one_left": [(10, 100, -300), (1, 110, -404), (10, 111, -500)],
    "hidden_overlap": [(30, 100, -900), (20, 500, -300), (15, 600, -320)],
}


def test_every_tie_family_decides_something():
    cases = {c["name"]: c for c in C.families()["ties"]}
    for name in C.TIE_NAMES:
        for tag, expect in (("fwd", EXPECT_FORWARD), ("rev", EXPECT_REVERSE)):
            case = cases["%s_%s" % (name, tag)]
            e = elim(case)
            assert e["dead"] or e["cropped"] or e["reordered"], case["name"]
            got = sorted((l,) + tuple(s) for l, s in zip(e["length"], e["start"]))
            if name in expect:
                assert got == sorted(expect[name]), (case["name"], got)
            if tag == "rev" and name in EXPECT_FORWARD:     # the left ends, and so who dies, do not depend on the strand
                assert len(got) == len(EXPECT_FORWARD[name]), case["name"]
        assert any(s < 0 for st in cases[name + "_rev"]["start"] for s in st)
    for tag in ("fwd", "rev"):
        assert elim(cases["three_passes_" + tag])["passes"][0] >= 3
        assert elim(cases["crossing_" + tag])["reordered"]
        assert 1 in elim(cases["both_sides_one_left_" + tag])["length"]
        ed = cases["exact_death_" + tag]                    # a match that dies of exactly its length must leave at once
        right = sorted((l, tuple(t)) for l, t in zip(elim(ed)["length"], elim(ed)["start"]))
        assert C.survivors_if_exact_deaths_lingered(ed["length"], ed["start"]) != right
        other = cases["nested_" + tag]                      # (and the wrong rule is the right one wherever nobody dies of exactly its length)
        assert C.survivors_if_exact_deaths_lingered(other["length"], other["start"]) == \
            sorted((l, tuple(t)) for l, t in zip(elim(other)["length"], elim(other)["start"]))
        lo = cases["hidden_overlap_" + tag]                 # the match genome 0 kills lies between the overlapping pair in genome 1's order
        f = facts(lo)
        dead0 = [i for i in elim(lo)["dead"]]
        o = f["order"][1]
        k = o.index(dead0[0])
        assert len(dead0) == 1 and 0 < k < len(o) - 1 and _right(lo, o[k - 1], 1) >= _left(lo, o[k + 1], 1)
        assert R.eliminate_overlaps(lo["length"], [[s[0], s[0]] for s in lo["start"]])["dead"] == dead0     # genome 0 alone kills it


def test_the_mixed_tie_lists_hold_every_family_around_the_tile_edge():
    cases = {c["name"]: c for c in C.families()["ties"]}
    for tag in ("fwd", "rev"):
        case = cases["ties_mixed_" + tag]
        aim, e = case["aim"], elim(case)
        assert len(case["length"]) == 1100 and aim["first_family"] < C.TILE < aim["first_family"] + aim["n_family"]
        alone = [elim(cases["%s_%s" % (name, tag)]) for name in C.TIE_NAMES]
        assert len(e["dead"]) == sum(len(a["dead"]) for a in alone) and len(e["cropped"]) == sum(len(a["cropped"]) for a in alone)
        for g in range(2):                                  # the families are entries 1000 .. of both orders
            members = set(facts(case)["order"][g][aim["first_family"]:aim["first_family"] + aim["n_family"]])
            assert set(e["dead"]) <= members
        assert e["reordered"] and e["passes"][0] >= 3


def test_graph_cases_have_the_planted_nodes_and_a_live_greedy_step():
    for case in C.families()["graph"]:
        assert 1100 <= len(case["length"]) <= 3100 or case["small"]
        assert sum(elim(case)["passes"]) == 0               # no overlaps: the graph alone is under test
        nodes = R.lcb_nodes(case["length"], case["start"])
        assert len(nodes) == case["aim"]["n_nodes"] and [nd["matches"][0] for nd in nodes] == case["aim"]["first"], case["name"]
        (w0, c0), (w, c1), (w2, c2) = case["runs"]
        assert (w0, c0, c1, w2, c2) == (0, 0, 0, 0, 1)
        lc = R.compute_lcbs(case["length"], case["start"], w)
        if len(nodes) > 1:
            assert lc["removed"] >= 1 and lc["merged"] >= 1 and lc["n_lcb"] >= 1, (case["name"], lc["removed"], lc["merged"])
            assert R.compute_lcbs(case["length"], case["start"], 0, True)["n_lcb"] == 1
    by = {c["name"]: c for c in C.families()["graph"]}
    assert by["graph_every_match_a_node"]["aim"]["n_nodes"] == len(by["graph_every_match_a_node"]["length"])
    assert by["graph_breaks_at_edges"]["aim"]["first"][1:3] == [C.TILE, 2 * C.TILE]
    assert by["graph_breaks_before_edges"]["aim"]["first"][1:3] == [C.TILE - 1, 2 * C.TILE - 1]
    assert by["graph_breaks_behind_edges"]["aim"]["first"][1:3] == [C.TILE + 1, 2 * C.TILE + 1]
    assert any(nd["orient"] for nd in R.lcb_nodes(by["graph_breaks_at_edges"]["length"], by["graph_breaks_at_edges"]["start"]))
    # equal-weight minima: the first in genome-0 order goes, the second merges with its neighbour and stays
    t = by["graph_tie_minima"]
    nodes = R.lcb_nodes(t["length"], t["start"])
    assert nodes[1]["weight"] == nodes[2]["weight"] == min(nd["weight"] for nd in nodes) < t["runs"][1][0]
    lc = R.compute_lcbs(t["length"], t["start"], t["runs"][1][0])
    assert lc["match_lcb"][nodes[1]["matches"][0]] == -1 and lc["match_lcb"][nodes[2]["matches"][0]] == 0 and lc["removed"] == 1


def test_wide_and_key_width_cases():
    wide = C.families()["wide"]
    assert [c["N"] for c in wide] == [5, 17, 32] and all(len(c["length"]) == 1100 for c in wide)
    assert elim(wide[1])["cropped"] and elim(wide[1])["dead"]
    for case, longest in zip(C.families()["key"], C.KEY_WIDTHS):
        assert max(case["glen"]) == case["glen"][1] == longest
        assert any(l == 1 and abs(s[1]) == longest for l, s in zip(case["length"], case["start"])), case["name"]
        assert elim(case)["cropped"]
    # 8-bit passes over pos_bits + 1 bits of key.  This restates chain_device_graph (chain_dev.hip: pos_bits = the bits of maxlen,
    # dead_key = 1 << pos_bits, sort_passes = (pos_bits + 1 + 7) / 8) with maxlen the longest genome (chain_device_core); if those
    # change, the widths of KEY_WIDTHS have to follow
    bits = [(g.bit_length() + 1 + 7) // 8 for g in C.KEY_WIDTHS]
    assert bits == [1, 2, 2, 3, 3, 4]


def test_dense_lists_keep_their_ties_and_have_work_to_do():
    dense = C.families()["dense"]
    assert len(dense) == 40 and all(900 <= len(c["length"]) <= 2300 for c in dense)
    assert any(len({s[0] for s in c["start"]}) < len(c["start"]) for c in dense)      # tied genome-0 starts are kept
    assert all(elim(c)["dead"] for c in dense)
    # at this density every one of them is a single cluster, or nearly: hand-back cases, all 40
    assert all(max(s for g in range(c["N"]) for _, s in facts(c)["clusters"][g]) > C.CL_MAX for c in dense)


def test_scaled_lists_reach_the_device_over_several_tiles():
    """the share that the docstring of chain_cases.random_scaled works out: four fifths of the span range give a mean depth of at
    most 1 and a largest cluster of about 15, so at least half of the lists must stay within the limit in every genome"""
    scaled = C.families()["dense_scaled"]
    top = [max(s for g in range(c["N"]) for _, s in facts(c)["clusters"][g]) for c in scaled]
    within = [c for c, t in zip(scaled, top) if t <= C.CL_MAX]
    assert len(scaled) == 24 and 2 * len(within) >= len(scaled)
    assert sum(len(c["length"]) > C.TILE for c in within) >= 8 and any(len(c["length"]) > 2 * C.TILE for c in within)
    for c in within:
        e = elim(c)
        assert e["dead"] and e["cropped"] and max(e["passes"]) >= 3
    assert any(len({s[0] for s in c["start"]}) < len(c["start"]) for c in within)     # ties among them
    assert {c["N"] for c in within} == {2, 3, 4} and min(top) >= 3
    assert any(s < 0 for c in within for st in c["start"] for s in st)
