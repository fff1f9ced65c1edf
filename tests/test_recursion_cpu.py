"""The planted recursion inputs of tests/recursion_cases.py without a GPU.  Every case is shown to be where it was aimed, from the
records of tests/recursion_ref.py (DESIGN.md S8 restated gap by gap) and the geometry stated in recursion_cases.py alone: a case
whose aim does not hold fails here.  The oracle's whole path is then held to the reference's anchors, LCB ids and LCB weights on
EVERY case it can take; the reference itself is pinned by a hand case and, on every case whose genomes have at most
recursion_cases.SMALL bases, by the brute force of tests/bruteforce.py over every gap searched.

(The oracle takes no ambiguity / contig tables on its whole path: the bitmap cases are held to the reference alone, and counted.)"""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import bruteforce as B
from tests import chain_ref as CH
from tests import recursion_cases as C
from tests import recursion_ref as R
from tests import seed_ref as S

NAMES = [c["name"] for c in C.all_cases() if c["entry"] != "progressive"]          # (the two progressive entries: their own test below)
CASE = {c["name"]: c for c in C.all_cases()}
N_BITMAP_CASES = 14
HAND_SEED = 14             # (a seed at which the random spacers of the hand case share no weight-5 mer by chance)


def test_seed_table_is_what_the_cases_assume():
    dont_care = {5: [2, 4], 7: [3, 5], 9: [2, 4, 8, 10]}
    for w, dc in dont_care.items():
        s = bin(C.pattern_of(w))[2:]
        assert len(s) == C.SPAN[w] == C.span_of(w) and s.count("1") == w
        assert [i for i, ch in enumerate(s) if ch == "0"] == dc, (w, s)
    assert C.span_of(6) == 9 and C.span_of(15) == 21


def test_default_weight_is_the_oracles():
    for n in list(range(0, 70)) + [180, 181, 182, 183, 511, 512, 513, 1447, 1448, 1449, 1450, 4095, 4096, 4097, 11585, 11586, 10 ** 6, 5 * 10 ** 6]:
        assert R.default_weight(n) == O.default_seed_weight(n), n
    assert [R.default_weight(n) for n in (181, 182, 1448, 1449, 11585, 11586)] == [5, 7, 7, 9, 9, 11]


def test_hand_case():
    """small enough to check by eye: two genomes, root weight 7, min_recursive_gap 10, one LCB of the anchors A = (30, [9, 9]) and
    B = (30, [69, 71]).  The gap: genome 0 bases 39 .. 68 (30), genome 1 bases 39 .. 70 (32), mean 31 -> weight 5 (span 7).
    genome 0's gap = x(12) P(8) y(10), genome 1's = x'(15) P(8) y'(9), P's flanks disagree over two bases: one match (8, [13, 16]) inside the gap,
    = (8, [51, 54]) in real coordinates.  Its left sub-gap (12 and 15 bases) wants weight 3: w<5; the right one (10 and 9) is short.  The same genomes with genome 1 reverse-complemented
    (length 108): A = (30, [9, -71]), B = (30, [69, -9]); the gap of genome 1 is 39 .. 70 read backwards, the match inside the gap is
    the same and its real start is -(70 - 15 - 8 + 1) = -48."""
    rng = np.random.default_rng(HAND_SEED)
    A, Bk, P, x, y, x1, y1 = (rng.integers(0, 4, n, dtype=np.uint8) for n in (30, 30, 8, 12, 10, 15, 9))
    one = lambda v: np.array(v, np.uint8)
    x[-1] = (P[0] + 1) % 4; x[0] = (A[-1] + 1) % 4; y[0] = (P[-1] + 1) % 4; y[-1] = (Bk[0] + 1) % 4
    x1[-1] = (P[0] + 2) % 4; x1[0] = (A[-1] + 2) % 4; y1[0] = (P[-1] + 2) % 4; y1[-1] = (Bk[0] + 2) % 4
    x[-2], y[1] = (x1[-2] + 1) % 4, (y1[1] + 1) % 4              # (two bases: one alone can stand on a don't-care offset)
    g0 = np.concatenate([one([0, 1, 2, 3] * 2), A, x, P, y, Bk, one([3, 2, 1, 0] * 2)])
    g1 = np.concatenate([one([3, 3, 2, 2, 1, 1, 0, 0]), A, x1, P, y1, Bk, one([0, 0, 1, 1, 2, 2, 3, 3])])
    span_of = lambda w: len(bin(C.pattern_of(w))) - 2
    for rev in (False, True):
        a, b = ((30, [9, -71]), (30, [69, -9])) if rev else ((30, [9, 9]), (30, [69, 71]))
        ref = R.recurse([g0, C.rc(g1) if rev else g1], [a, b], [0, 0], C.pattern_of, span_of, 7, 10)
        r0 = ref["records"][0]
        assert (r0["lo"], r0["lens"], r0["rev"]) == ([39, 39], [30, 32], [False, rev]) and (r0["raw"], r0["weight"]) == (5, 5)
        assert r0["matches"] == [(8, [13, 16])] and r0["non_forward"] == [] and r0["nodes"] == 1 and r0["deleted"] == []
        assert r0["survivors"] == [(8, [51, -48] if rev else [51, 54])]
        assert [(q["level"], q["why"]) for q in ref["records"][1:]] == [(2, "w<5"), (2, "short")]
        assert ref["anchor_length"] == [30, 8, 30] and ref["anchor_start"] == [a[1], r0["survivors"][0][1], b[1]] and ref["anchor_lcb"] == [0, 0, 0]
        assert list(ref["batches"]) == [(1, 5)] and R.virtual_layout(ref["batches"][(1, 5)]) == [{"seg": [0], "total": 30}, {"seg": [0], "total": 32}]
    assert R.recurse([g0, g1], [(30, [9, 9]), (30, [69, 71])], [0, 0], C.pattern_of, span_of, 7, 32)["records"][0]["why"] == "short"
    assert R.recurse([g0, g1], [(30, [9, 9]), (30, [69, 71])], [0, 0], C.pattern_of, span_of, 7, 31)["records"][0]["weight"] == 5
    assert R.recurse([g0, g1], [(30, [9, 9]), (30, [69, 71])], [0, 0], C.pattern_of, span_of, 6, 10)["records"][0]["why"] == "w<5"


def _asc(g):
    return "".join("ACGT"[int(c)] for c in g)


SMALL_NAMES = [c["name"] for c in C.all_cases() if max(len(g) for g in c["genomes"]) <= C.SMALL and c["family"] != "entries"]


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_reference_gaps_equal_bruteforce(name):
    case, ref = CASE[name], C.reference(CASE[name])
    N = case["N"]
    for r in ref["records"]:
        if not r["weight"]:
            continue
        subs = []
        for g in range(N):
            x = case["genomes"][g][r["lo"][g] - 1:r["lo"][g] - 1 + r["lens"][g]]
            subs.append(_asc(C.rc(x) if r["rev"][g] else x))
        got = B.brute_matches(subs, C.pattern_of(r["weight"]), mode="mem", mask=(1 << N) - 1, valid=r["valid"])
        assert got == {(l, tuple(s)) for l, s in r["matches"]}, (name, r["level"], r["index"])


def test_small_cases_exist_in_every_family_but_limits():
    fam = {CASE[n]["family"] for n in SMALL_NAMES}
    assert fam >= set(C.FAMILIES) - {"limits", "entries"}, fam


# ---- aims --------------------------------------------------------------------------------------------------------------------------
def _rec(ref, level, index):
    return next(r for r in ref["records"] if r["level"] == level and r["index"] == index)


def _local_name(case, rec, name):
    """the stretch as a match inside the gap, by its length and genome-0 start (genome 0 is forward in every LCB)"""
    s, n, _ = case["pos"][0][name]
    return n, s - rec["lo"][0] + 1


@pytest.mark.parametrize("name", NAMES)
def test_case_is_where_it_was_aimed(name):
    case, ref = CASE[name], C.reference(CASE[name])
    aim, N, recs = case["aim"], case["N"], ref["records"]
    tb = [x[:3] for x in C.trace_batches(ref)]
    final = list(zip(ref["anchor_length"], ref["anchor_start"]))
    root = set(zip(ref["mums"][0], map(tuple, ref["mums"][1])))
    if "blocks" in aim:
        assert len(ref["root"]["anchor_length"]) == aim["blocks"] and set(ref["root"]["anchor_length"]) <= {30, C.BLOCK}, ref["root"]["anchor_length"]
    if "records" in aim:
        assert len(recs) == aim["records"]
    for lv, i, lens in aim.get("lens", []):
        assert _rec(ref, lv, i)["lens"] == lens
    for lv, i, lo in aim.get("lo", []):
        assert _rec(ref, lv, i)["lo"] == lo and (lo[0] - 1) % C.WORD == (lo[0] - 1) - 320
    for lv, i, why in aim.get("why", []):
        assert _rec(ref, lv, i)["why"] == why and _rec(ref, lv, i)["weight"] == 0
    if "batches" in aim:
        assert tb == aim["batches"], tb
    if "level1" in aim:
        assert [x for x in tb if x[0] == 1] == aim["level1"], tb
    if "first_batch" in aim:
        assert tb[0] == aim["first_batch"], tb
    if "levels" in aim:
        assert [(lv, w) for lv, w, _ in tb] == [(k + 1, w) for k, w in enumerate(aim["levels"])], tb
        rest = [r["why"] for r in recs if r["level"] == len(aim["levels"]) + 1]
        assert rest and set(rest) <= {"short", aim["stops"]} and aim["stops"] in rest, rest
    if "raw" in aim:
        lv, i, raw = aim["raw"]
        assert _rec(ref, lv, i)["raw"] == raw and _rec(ref, lv, i)["weight"] == case["params"]["seed_weight"] - 2 < raw
    if aim.get("silent"):
        assert all(not r["matches"] for r in recs) and len(final) == len(ref["root"]["anchor_length"])
    for x, lv in aim.get("found", []):
        ln, st = C.planted(case, x)
        assert (ln, tuple(st)) not in root
        assert not any((ln, st) in r.get("matches_real", []) for r in recs if r["level"] < lv), (x, "seen too early")
        assert any((ln, st) in r.get("matches_real", []) for r in recs if r["level"] == lv), (x, lv)
        assert (ln, st) in final, (x, "not kept")
    for x in aim.get("absent", []):
        if all(x in case["pos"][g] for g in range(N)):
            assert C.planted(case, x) not in [(l, s) for l, s in final]
    for x, g in aim.get("negative", []):
        assert C.planted(case, x)[1][g] < 0 and C.planted(case, x) in final
    if "non_forward" in aim or "deleted" in aim or "tie" in aim:
        r = _rec(ref, 1, 0)
        for x in aim.get("non_forward", []):
            k = r["matches_real"].index(C.planted(case, x))
            assert r["matches"][k] in r["non_forward"] and r["matches"][k] not in r["forward"]
        gone = [[(r["elim"][i][0], r["elim"][i][1][0]) for i in d["matches"]] for d in r["deleted"]]
        for x in aim.get("deleted", []):
            assert C.planted(case, x) in r["matches_real"] and C.planted(case, x) not in r["survivors"] and [_local_name(case, r, x)] in gone, (x, gone)
        if "deleted_order" in aim:
            assert gone[:len(aim["deleted_order"])] == [[_local_name(case, r, x)] for x in aim["deleted_order"]], gone
        if "tie" in aim:
            assert gone[0] == [_local_name(case, r, aim["tie"])] and len(r["deleted"][0]["tied"]) >= 2 and r["deleted"][0]["tied"][0] == 0
    for lv, w, g, k, v in aim.get("seg", []):
        assert R.virtual_layout(ref["batches"][(lv, w)])[g]["seg"][k] == v
    for lv, w, g, T in aim.get("total", []):
        assert R.virtual_layout(ref["batches"][(lv, w)])[g]["total"] == T
    for x, g, border in aim.get("across", []):
        r = _rec(ref, 1, 0)
        ln, s = r["matches"][r["matches_real"].index(C.planted(case, x))]
        assert s[g] - 1 < border < s[g] - 1 + ln, (x, g, s)
    if "same_content" in aim:
        a, b = aim["same_content"]
        assert np.array_equal(case["genomes"][0][case["pos"][0][a][0] - 1:][:9], case["genomes"][0][case["pos"][0][b][0] - 1:][:9])
        assert not any(C.planted(case, a) in r.get("matches_real", []) and C.planted(case, b) in r["matches_real"] for r in recs)
    for lv, i, m in aim.get("local", []):
        assert m in _rec(ref, lv, i)["matches"] and m in _rec(ref, lv, i)["survivors_local"], (m, _rec(ref, lv, i)["matches"])
    if "local_all" in aim:
        lv, i, want = aim["local_all"]
        assert sorted(_rec(ref, lv, i)["forward"]) == sorted(want)
    if "cluster" in aim:
        g, n = aim["cluster"]
        fw = _rec(ref, 1, 0)["forward"]
        facts = CH.input_facts([l for l, _ in fw], [s for _, s in fw])
        assert max(sz for _, sz in facts["clusters"][g]) == n and max(sz for _, sz in facts["clusters"][0]) == 1
    if "cropped_to" in aim:
        x, ov, left = aim["cropped_to"]
        r = _rec(ref, 1, 0)
        k = r["matches_real"].index(C.planted(case, x))
        ln, st = r["matches"][k]
        assert ln == ov + left and r["cropped"] == [(ln, st)] and r["dead"] == []
        others = [m for m in r["forward"] if m != (ln, st)]
        assert [[max(s + l - t, 0) for s, t in zip(so, st)] for l, so in others] == [[0, ov, 0]]       # the overlap: in genome 1 only, all but `left` columns
        assert (left, [s + ov for s in st]) in r["elim"] and (left, [s + ov for s in st]) in r["survivors_local"]
        assert (left, [s + ov for s in C.planted(case, x)[1]]) in final
    if "extension" in aim:
        x, w = aim["extension"]
        assert [q for q in ref["ext_rounds"] if q[1]] == [(w, 1, True)], ref["ext_rounds"]
        assert C.planted(case, x) in list(zip(ref["root"]["anchor_length"], ref["root"]["anchor_start"])) and (C.planted(case, x)[0], tuple(C.planted(case, x)[1])) not in root
        assert len(ref["root"]["anchor_length"]) == 3 and ref["n_lcb"] == 1
        assert [r["a"] for r in recs if r["level"] == 1][0] == C.planted(case, x)          # the first gap begins behind E: it is there through the extension alone
    if "mask_bit" in aim:
        lv, i, x, bit = aim["mask_bit"]
        lay = R.virtual_layout(ref["batches"][(lv, 5)])
        s1 = case["pos"][1][x][0]
        flagged = int(np.flatnonzero(case["invalid"][1])[0]) + 1
        virtual = lambda real: lay[1]["seg"][i] + real - _rec(ref, lv, i)["lo"][1]
        assert virtual(s1) == C.MASK_WORD and virtual(flagged) == bit and bit in (C.MASK_WORD - 1, C.MASK_WORD)
    if "nodes" in aim:
        lv, i, n = aim["nodes"]
        r = _rec(ref, lv, i)
        assert r["nodes"] == n and len(r["deleted"]) == n - 1 and all(len(d["matches"]) == 1 for d in r["deleted"])
        assert r["survivors"] == [C.planted(case, aim["survivor"])]
        assert [d["matches"][0] for d in r["deleted"]] == list(range(n - 1))                 # ties: the first in genome-0 order goes, every time
        assert (n > C.GAP_KMAX or n * N > C.GAP_LINKS) == aim["beyond"]
    if "seam" in aim:
        h1, h2, merged, cropped = aim["seam"]
        batch = ref["batches"][(1, 5)]
        lay = R.virtual_layout(batch)
        free = S.find(R.virtual_genomes(case["genomes"], batch), C.pattern_of(5), S.MEM, (1 << N) - 1, True, None)       # WITHOUT the segment rule
        s1 = [case["pos"][g][h1][0] - batch[0]["lo"][g] + 1 for g in range(N)]                # H1 inside gap 0 = in the virtual genome
        assert (merged, s1) in list(zip(free["length"], free["start"])), "the seam case is not live"
        assert all(s1[g] - 1 + merged > lay[g]["seg"][1] for g in range(N))
        assert (8, s1) in batch[0]["matches"] and (cropped, [1, 2, 1]) in batch[1]["matches"]
        assert not any(l >= merged for r in batch for l, _ in r["matches"])
    if "straddle" in aim:
        batch = ref["batches"][(1, 5)]
        lay = R.virtual_layout(batch)
        free = S.find(R.virtual_genomes(case["genomes"], batch), C.pattern_of(5), S.MEM, (1 << N) - 1, True, None)
        assert any(all(s[g] - 1 < lay[g]["seg"][1] < s[g] - 1 + l for g in range(N)) for l, s in zip(free["length"], free["start"])), "the straddle case is not live"
        assert not any(s[0] + l - 1 == batch[0]["lens"][0] for l, s in batch[0]["matches"]) and not any(s[0] == 1 for l, s in batch[1]["matches"])
        assert len(final) == len(ref["root"]["anchor_length"]) or all(r["level"] == 1 for r in recs if r["weight"])


def test_live_cases_are_all_there():
    have = {k for c in C.all_cases() for k in c["aim"]}
    assert {"seam", "straddle", "same_content", "tie", "nodes", "cluster", "seg", "total", "across", "raw"} <= have
    assert sorted(c["aim"]["nodes"][2] for c in C.family("limits")) == [80, 81, 426, 427, 512, 513]
    assert sorted(c["aim"]["cluster"][1] for c in C.family("chain") if "cluster" in c["aim"]) == [2, 2, 3, 48, 49]
    assert sorted(c["aim"]["level1"][0][2] for c in C.family("count")) == [1, 2, 3, 4, 63, 64, 255, 256, 257, 1023, 1024]
    assert not CASE[C.NOTHING]["aim"].get("found") and CASE[C.NOTHING]["aim"]["silent"]


def _column_pairs(aln, g, h):
    """the (position in g, position in h) pairs that share a column of a result (left / right 1-based, `reverse` genomes run backwards)"""
    out = set()
    for i in range(aln["n_iv"]):
        if not (aln["right"][i][g] and aln["right"][i][h]):
            continue
        at = {q: int(aln["right"][i][q]) if aln["reverse"][i][q] else int(aln["left"][i][q]) for q in (g, h)}
        step = {q: -1 if aln["reverse"][i][q] else 1 for q in (g, h)}
        for c in aln["cols"][aln["col_off"][i]:aln["col_off"][i + 1]]:
            if (c >> g) & 1 and (c >> h) & 1:
                out.add((at[g], at[h]))
            for q in (g, h):
                if (c >> q) & 1:
                    at[q] += step[q]
    return out


PROGRESSIVE = [c["name"] for c in C.all_cases() if c["entry"] == "progressive"]


@pytest.mark.parametrize("name", PROGRESSIVE)
def test_progressive_oracle_equals_reference(name):
    """S9 has no restatement with the recursion in it, so the oracle's progressive path is held to the S8 reference where the two
    meet: the node over genomes {1, 2} has the chain A, B (the pairwise root search finds A, B, C and not P; C belongs to the root
    node), tests/recursion_ref.py recurses into the gap between them, and EVERY anchor it ends with -- A, B, P and what chance adds --
    must stand column by column in the oracle's result, on the strand the reference gives it.  The oracle's result changes
    with `recursive` (liveness)."""
    case, ref = CASE[name], C.pair_reference(CASE[name])
    rel = case["pos"][2]["A"][2]
    s1, s2 = case["pos"][1]["P"][0], case["pos"][2]["P"][0]
    r0 = ref["records"][0]
    assert (12, [s1, -s2 if rel else s2]) in r0["matches_real"] and (12, [s1, -s2 if rel else s2]) in r0["survivors"]
    assert r0["weight"] == 5 and r0["rev"] == [False, rel] and len(ref["anchor_length"]) >= 3

    def columns(l, st):
        return {(st[0] + k, (-st[1] + l - 1 - k) if st[1] < 0 else st[1] + k) for k in range(l)}
    on = O.progressive_align(case["genomes"], O.default_params(**case["params"]), tree=case["tree"])["aln"]
    off = O.progressive_align(case["genomes"], O.default_params(**dict(case["params"], recursive=0)), tree=case["tree"])["aln"]
    pairs = _column_pairs(on, 1, 2)
    for l, st in zip(ref["anchor_length"], ref["anchor_start"]):
        assert columns(l, st) <= pairs, (name, l, st)
    assert on["n_iv"] != off["n_iv"] or not np.array_equal(on["cols"], off["cols"])           # (the DP may well align P without its anchor; the walk differs)


# ---- the oracle against the reference ----------------------------------------------------------------------------------------------
ORACLE_NAMES = [c["name"] for c in C.all_cases() if c["oracle"] and c["entry"] != "progressive"]


@pytest.mark.parametrize("name", ORACLE_NAMES)
def test_oracle_equals_reference(name):
    case, ref = CASE[name], C.reference(CASE[name])
    e = O.align(case["genomes"], O.default_params(**case["params"]))
    a = e["aln"]
    assert a["anchor_length"].tolist() == ref["anchor_length"], name
    assert a["anchor_start"].tolist() == ref["anchor_start"], name
    assert a["anchor_lcb"].tolist() == ref["anchor_lcb"], name
    assert e["lcbs"]["n_lcb"] == ref["n_lcb"] and e["lcbs"]["weight"].tolist() == ref["lcb_weight"], name
    ml, ms = O.multiplicity_filter(e["mums"][0], e["mums"][1], case["N"])
    assert (ml.tolist(), ms.tolist()) == (list(ref["mums"][0]), [list(s) for s in ref["mums"][1]])


def test_every_case_but_the_bitmap_cases_is_compared():
    """the two tests above are parametrised over every case the oracle can take: whatever they leave out is a bitmap case"""
    left_out = [c for c in C.all_cases() if c["name"] not in ORACLE_NAMES + PROGRESSIVE]
    assert len(left_out) == N_BITMAP_CASES
    assert all(c["family"] == "bitmaps" and not c["oracle"] and (c["contigs"] is not None or c["invalid"] is not None) for c in left_out)
    assert all(c["oracle"] and c["contigs"] is None and c["invalid"] is None for c in C.all_cases() if c not in left_out)
