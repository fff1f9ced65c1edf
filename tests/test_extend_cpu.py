"""The planted LCB-extension inputs of tests/extend_cases.py without a GPU.  Every case is shown to be where it was aimed, from the
records of tests/extend_ref.py (DESIGN.md S10 restated at match level) and the geometry stated in extend_cases.py alone: a case
whose aim does not hold fails here.  The oracle's whole path (recursive = 0, gapped = 0) is then held to the reference's anchors,
LCB ids and weights on every case; the reference itself is pinned by a hand case and, on the piece cases, by the brute force of
tests/bruteforce.py over the pieces.

(The oracle takes no ambiguity / contig tables on its whole path: the four bitmap cases are held to the reference alone.)"""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import bruteforce as B
from tests import extend_cases as C
from tests import extend_ref as R
from tests import seed_ref as S


pattern_of = C.pattern_of


def _reference(name):
    return C.reference(CASE[name])


NAMES = [c["name"] for c in C.all_cases()]
CASE = {c["name"]: c for c in C.all_cases()}


def test_seed_table_is_what_the_cases_assume():
    for w, span in C.SPAN.items():
        s = bin(pattern_of(w))[2:]
        assert len(s) == span and s.count("1") == w
        assert all("1" in s[i:i + C.FLANK] for i in range(span - C.FLANK + 1)), w     # a care position in any 6 consecutive offsets
    assert tuple(C.SPAN[15 - 2 * (k + 1)] for k in range(4)) == C.ROUND_LEN


def test_hand_case():
    """small enough to check by eye: two genomes, seed weight 7 (span 9), one round at weight 5 (span 7).
    genome 0 = L(8) A(30) x(3) P(8) y(4) B(30) R(8), genome 1 = L'(8) A(30) x'(5) P(8) y'(2) rc(B)(30) R'(8); P's flanks disagree.
    Root: A and B, two LCBs.  Round 0: pieces of genome 0 are (1, 8), (39, 15), (84, 8), of genome 1 (1, 8), (39, 15), (84, 8); P
    (8 bases at 42 and at 44) is found, lies behind A in both genomes and joins its LCB: weight 60 -> 76."""
    rng = np.random.default_rng(5)
    A, Bk, P = (rng.integers(0, 4, n, dtype=np.uint8) for n in (30, 30, 8))
    one = lambda v: np.array(v, np.uint8)
    g0 = np.concatenate([one([0, 1, 2, 3, 0, 1, 2, 3]), A, one([(A[-1] + 1) % 4, 0, (P[0] + 1) % 4]), P, one([(P[-1] + 1) % 4, 1, 1, (Bk[0] + 1) % 4]), Bk, one([(Bk[-1] + 2) % 4, 3, 2, 1, 0, 3, 2, 1])])
    g1 = np.concatenate([one([3, 3, 2, 2, 1, 1, 0, 0]), A, one([(A[-1] + 2) % 4, 2, 2, 3, (P[0] + 2) % 4]), P, one([(P[-1] + 2) % 4, (3 - Bk[-1] + 1) % 4]), C.rc(Bk), one([(3 - Bk[0] + 1) % 4, 0, 0, 1, 1, 2, 2, 3])])
    root = S.find([g0, g1], pattern_of(7), S.MEM, 3)
    assert (root["length"], root["start"]) == ([30, 30], [[9, 9], [54, -54]])
    ref = R.extend([g0, g1], root["length"], root["start"], pattern_of, 7, 20, 4, False)
    assert len(ref["rounds"]) == 1 and ref["rounds"][0]["weight"] == 5 and ref["rounds"][0]["span"] == 7
    assert ref["rounds"][0]["pieces"] == [[(1, 8), (39, 15), (84, 8)], [(1, 8), (39, 15), (84, 8)]]
    assert ref["rounds"][0]["layout"][0] == {"vstart": [0, 9, 25], "sep": [8, 24], "total": 33}
    assert ref["rounds"][0]["new"] == [(8, [42, 44])] and ref["rounds"][0]["kept"]
    assert ref["rounds"][0]["fate"][0]["how"] == "joined" and ref["rounds"][0]["fate"][0]["old"] == [0]
    assert ref["anchor_length"] == [30, 8, 30] and ref["anchor_start"] == [[9, 9], [42, 44], [54, -54]] and ref["anchor_lcb"] == [0, 0, 1]
    assert ref["lcb_weight"] == [76, 60] and ref["lcb_left"] == [[9, 9], [54, -54]] and ref["lcb_right"] == [[49, 51], [83, -83]]
    assert R.rec_gaps(ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"], 4) == [(0, 5)]
    assert R.rec_gaps(ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"], 5) == []


def _asc(g):
    return "".join("ACGT"[int(c)] for c in g)


@pytest.mark.parametrize("name", [c["name"] for c in C.family("pieces") if len(c["genomes"][0]) <= 2500])
def test_reference_rounds_equal_bruteforce_over_the_pieces(name):
    case, ref = CASE[name], _reference(name)
    seqs = [_asc(g) for g in case["genomes"]]
    for r in ref["rounds"]:
        if r["starved"]:
            continue
        valid = [[(a, a + n - 1) for a, n in r["pieces"][g]] for g in range(case["N"])]
        got = B.brute_matches(seqs, r["pattern"], mode="mem", mask=(1 << case["N"]) - 1, valid=valid)
        assert got == {(l, tuple(s)) for l, s in r["new"]}, (name, r["round"])


# ---- aims --------------------------------------------------------------------------------------------------------------------------
def _piece_with(case, rec, g, name):
    s, n, _ = case["pos"][g][name]
    for k, (a, ln) in enumerate(rec["pieces"][g]):
        if a <= s and s + n <= a + ln:
            return k, a, ln
    return None


def _lcb_of_block(case, src, name):
    """the LCB of the anchor that holds the block's first base in genome 0, in a set of anchors (the root's, a round's, the final)"""
    s = case["pos"][0][name][0]
    for l, st, k in zip(src["anchor_length"], src["anchor_start"], src["anchor_lcb"]):
        if abs(st[0]) <= s < abs(st[0]) + l:
            return k
    return None


@pytest.mark.parametrize("name", NAMES)
def test_case_is_where_it_was_aimed(name):
    case, ref = CASE[name], _reference(name)
    aim, N, rounds = case["aim"], case["N"], ref["rounds"]
    root = set(zip(ref["mums"][0], map(tuple, ref["mums"][1])))
    assert ref["root"]["n_lcb"] >= 1
    if "lcbs_root" in aim:
        assert ref["root"]["n_lcb"] == aim["lcbs_root"]
    if "rounds" in aim:
        assert len(rounds) == aim["rounds"], [r["weight"] for r in rounds]
    if aim.get("round_weight"):
        k, w = aim["round_weight"]
        assert rounds[k]["weight"] == w and rounds[k]["span"] == C.SPAN[w]
    for f in aim.get("found", []):
        ln, st = C.planted(case, f["name"])
        assert (ln, tuple(st)) not in root
        for r in rounds[:f["round"]]:
            assert (ln, st) not in r["new"], (f, r["round"])
        r = rounds[f["round"]]
        assert (ln, st) in r["new"], (f, r["new"])
        fate = next(x for x in r["fate"] if x["found"] == (ln, st))
        if f["how"] is not None:
            assert fate["how"] == f["how"], (f, fate)
        assert (fate["how"] == "dropped") or r["kept"]
        if fate["how"] != "dropped":
            assert fate["length"] == ln                      # kept whole
            # outside every LCB extent of the round, in every genome (a stretch inside one is the recursion's business)
            for g in range(N):
                a = abs(st[g])
                assert all(not (e[g][0] <= a + ln - 1 and a <= e[g][1]) for e in r["extents"])
        if f.get("joins"):
            assert fate["old"] == [_lcb_of_block(case, r["anchors_before"], f["joins"])]
        if f.get("cropped") is not None:
            assert fate["length"] == f["cropped"]
    for nm in aim.get("absent", []):
        ln, st = C.planted(case, nm)
        assert (ln, tuple(st)) not in root
        for r in rounds:
            for l2, s2 in r["new"]:
                assert not (abs(s2[0]) <= abs(st[0]) + ln - 1 and abs(st[0]) <= abs(s2[0]) + l2 - 1), (nm, r["round"], l2, s2)
    for nm in aim.get("absent_new", []):
        ln, st = C.planted(case, nm)
        assert (ln, tuple(st)) not in root and all((ln, st) not in r["new"] for r in rounds)
    for g, k, nm, front, behind in aim.get("piece", []):
        _, a, pl = _piece_with(case, rounds[k], g, nm)
        s, n, _ = case["pos"][g][nm]
        if front is not None:
            assert s - a == front, (nm, s - a)
        assert (a + pl) - (s + n) == behind
        if front == 0 and behind == 0:
            assert pl == n                                   # the stretch fills the piece
    for g, k, nm in aim.get("no_piece", []):
        assert _piece_with(case, rounds[k], g, nm) is None
    for g, k, nm in aim.get("piece_starts_with", []):
        assert _piece_with(case, rounds[k], g, nm)[1] == case["pos"][g][nm][0]
    for g, k, at in aim.get("first_piece_at", []):
        first = rounds[k]["pieces"][g][0][0]
        assert first == 1 if at == 1 else first > 1
    for g, k, tail in aim.get("last_piece_ends", []):
        a, pl = rounds[k]["pieces"][g][-1]
        assert (a + pl - 1 == len(case["genomes"][g])) == tail
    for g, k, v in aim.get("sep", []):
        assert rounds[k]["layout"][g]["sep"][0] == v and rounds[k]["pieces"][g][0] == (1, v)
    for g, k, T in aim.get("total", []):
        lay = rounds[k]["layout"][g]
        assert lay["total"] == T == sum(n for _, n in rounds[k]["pieces"][g]) + len(lay["sep"])
        a, pl = rounds[k]["pieces"][g][-1]
        assert a + pl - 1 == len(case["genomes"][g])
    for k, counts in aim.get("npieces", []):
        assert [len(p) for p in rounds[k]["pieces"]] == counts and C.pieces_K(rounds[k]["pieces"]) == max(counts)
    for g, k, nm, idx in aim.get("in_piece", []):
        assert _piece_with(case, rounds[k], g, nm)[0] == idx
    for g, k, x, y in aim.get("adjacent_pieces", []):
        kx, ky = _piece_with(case, rounds[k], g, x)[0], _piece_with(case, rounds[k], g, y)[0]
        lay = rounds[k]["layout"][g]
        assert ky == kx + 1
        # virtual coordinates: X's last base, the separator, Y's first base
        vx = lay["vstart"][kx] + (case["pos"][g][x][0] - rounds[k]["pieces"][g][kx][0]) + case["pos"][g][x][1] - 1
        assert lay["sep"][kx] == vx + 1 and lay["vstart"][ky] == vx + 2
    for k in aim.get("windows_beyond_tiny", []):
        windows = sum(max(lay["total"] - rounds[k]["span"] + 1, 0) for lay in rounds[k]["layout"])
        assert windows > C.TINY_MAX and N <= 16, (k, windows)
    if "between" in aim:
        a, z, pp = (case["pos"][0][x][0] for x in aim["between"])
        assert a < z < pp                                     # in genome 0 the light neighbour stands between the LCB and the match
    if "adjacent_pieces" in aim:
        # THE SEPARATOR CARRIES THE RULE: over the virtual genomes that the text prescribes, a search that respects the separators
        # finds X and Y apart; the same search with the separators taken for ordinary bases finds ONE match X a Y of 2 L + 1 bases
        g, k, x, y = aim["adjacent_pieces"][0]
        r = rounds[k]
        virt, valid = [], []
        for h in range(N):
            parts, iv, at = [], [], 0
            for i, (a, n) in enumerate(r["pieces"][h]):
                parts.append(case["genomes"][h][a - 1:a - 1 + n])
                iv.append((at + 1, at + n))
                at += n
                if i + 1 < len(r["pieces"][h]):
                    parts.append(np.zeros(C.SEPARATORS, np.uint8))
                    at += C.SEPARATORS
            virt.append(np.concatenate(parts))
            valid.append(iv)
            assert at == r["layout"][h]["total"]
        L = case["pos"][0][x][1]
        kx = _piece_with(case, r, 0, x)[0]
        vx = r["layout"][0]["vstart"][kx] + case["pos"][0][x][0] - r["pieces"][0][kx][0] + 1      # X's 1-based virtual start in genome 0
        with_sep = S.find(virt, r["pattern"], S.MEM, (1 << N) - 1, True, valid)
        without = S.find(virt, r["pattern"], S.MEM, (1 << N) - 1, True, None)
        at0 = lambda f: sorted((l, st[0]) for l, st in zip(f["length"], f["start"]) if vx <= st[0] <= vx + L + 1)
        assert at0(with_sep) == [(L, vx), (L, vx + L + 1)] and at0(without) == [(2 * L + 1, vx)]
    for x, y, d in aim.get("same_diagonal", []):
        for g in range(N):
            sx, sy = case["pos"][g][x], case["pos"][g][y]
            if g == 0 and "adjacent_pieces" in aim:
                continue                                      # (genome 0 holds B2 between them: one diagonal in virtual coordinates only)
            assert abs(sy[0] - sx[0]) == d
    for g, nm, blk, side in aim.get("touch", []):
        s, n, _ = case["pos"][g][nm]
        bs, bn, _ = case["pos"][g][blk]
        assert (s + n == bs) if side == "front" else (bs + bn == s)
    for first, last, count, rev in aim.get("lcb_of", []):
        k = _lcb_of_block(case, ref["root"], first)
        assert k == _lcb_of_block(case, ref["root"], last) and ref["root"]["anchor_lcb"].count(k) == count
        i = ref["root"]["anchor_lcb"].index(k)
        assert (ref["root"]["anchor_start"][i][1] < 0) == bool(rev)
    if "starved" in aim:
        if aim["starved"] is None:
            assert all(not r["starved"] for r in rounds)
        else:
            k, g = aim["starved"]
            assert rounds[k]["starved"] == [g] and len(rounds) == k + 1
    for k, before, after in aim.get("lcbs", []):
        assert (rounds[k]["lcb_before"], rounds[k]["lcb_after"]) == (before, after), (k, rounds[k]["lcb_before"], rounds[k]["lcb_after"])
    for k, kept in aim.get("kept", {}).items():
        assert rounds[k]["kept"] == kept and rounds[k]["dropped"] == (not kept) and len(rounds[k]["new"]) > 0
    for nm, k, how in aim.get("refound", []):
        ln, st = C.planted(case, nm)
        assert next(x for x in rounds[k]["fate"] if x["found"] == (ln, st))["how"] == how
    if "ids_move" in aim:
        r = rounds[aim["ids_move"]]
        new_ids = sorted(f["lcb"] for f in r["fate"] if f["how"] == "new")
        assert new_ids and new_ids[0] < r["lcb_after"] - 1   # an LCB of new matches in front of old ones: their ids move
    if "weight_up" in aim:
        blk, up = aim["weight_up"]
        k0, k1 = _lcb_of_block(case, ref["root"], blk), _lcb_of_block(case, ref, blk)
        w0 = sum(l for l, k in zip(ref["root"]["anchor_length"], ref["root"]["anchor_lcb"]) if k == k0) * N
        assert ref["lcb_weight"][k1] == w0 + up
    if "overlap" in aim:
        x, y, ov, g = aim["overlap"]
        (lx, sx), (ly, sy) = C.planted(case, x), C.planted(case, y)
        # both found whole; they overlap by ov columns in genome g and nowhere else; whole, the shorter one met the weight
        for h in range(N):
            a, b = sorted([(abs(sx[h]), lx), (abs(sy[h]), ly)])
            assert (a[0] + a[1] - b[0] == ov) if h == g else (a[0] + a[1] <= b[0])
        assert ly < lx and (ly - ov) * N < case["params"]["lcb_weight"] <= ly * N
        assert (ly - ov, ) == tuple(m[0] for m in rounds[0]["new_elim"] if m[1][0] == sy[0])
    if "na" in aim:
        assert len(ref["root"]["anchor_length"]) == aim["na"]
        s0 = [s[0] for s in ref["root"]["anchor_start"]]
        assert s0 == sorted(s0)
        for nm, at in aim["insert"]:
            p = case["pos"][0][nm][0]
            assert sum(1 for s in s0 if s < p) == at, (nm, at)
        kept = sum(1 for r in rounds for f in r["fate"] if f["how"] != "dropped")
        assert kept == len(aim["insert"]) and len(ref["anchor_length"]) == aim["na"] + kept
    if "rec_gap" in aim:
        mg, plus, G = aim["rec_gap"]
        assert case["params"]["min_recursive_gap"] == mg and G == mg + plus
        gaps = R.rec_gaps(ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"], 0)
        assert max(x for _, x in gaps) == G
        assert len(R.rec_gaps(ref["anchor_length"], ref["anchor_start"], ref["anchor_lcb"], mg)) == plus
        assert len(R.rec_gaps(ref["root"]["anchor_length"], ref["root"]["anchor_start"], ref["root"]["anchor_lcb"], mg)) == 0
    if "old_died" in aim:
        r = rounds[aim["old_died"]]
        assert r["kept"] and r["old_died"] > 0
    if "cut" in aim:
        nm, where, kind, p0 = aim["cut"]
        ln, st = C.planted(case, nm)
        s = st[0]
        clean = C.clean_intervals(case)[0]
        if kind == "invalid":
            assert all(not (lo <= p0 + 1 <= hi) for lo, hi in clean)
        else:
            assert any(lo == p0 + 1 for lo, _ in clean)
        at = lambda r: [m for m in rounds[r]["new"] if s <= m[1][0] < s + ln]
        if where == "behind":
            assert p0 + 1 == s + ln and at(0) == [(ln, st)]
        else:
            left = p0 - (s - 1)                              # bases of the stretch in front of the cut: round 1 sees them, round 0 nothing
            assert left == 15 and ln - left <= 5 and at(0) == [] and at(1) == [(left, st)]
    if not case["device"]:
        assert case["params"]["collinear"] or case["params"]["lcb_scoring"] or case["contigs"] or case["invalid"]


PLAIN = [c["name"] for c in C.all_cases() if c["contigs"] is None and c["invalid"] is None]     # (the oracle's whole path takes no ambiguity / contig tables)


@pytest.mark.parametrize("name", PLAIN)
def test_oracle_equals_reference(name):
    case, ref = CASE[name], _reference(name)
    p = {k: v for k, v in case["params"].items()}
    e = O.align(case["genomes"], O.default_params(recursive=0, gapped=0, **{k: v for k, v in p.items() if k != "recursive"}))
    ml, ms = O.multiplicity_filter(e["mums"][0], e["mums"][1], case["N"])
    assert ml.tolist() == ref["mums"][0] and ms.tolist() == ref["mums"][1]
    a = e["aln"]
    assert a["anchor_length"].tolist() == ref["anchor_length"]
    assert a["anchor_start"].tolist() == ref["anchor_start"]
    assert a["anchor_lcb"].tolist() == ref["anchor_lcb"]
    assert e["lcbs"]["n_lcb"] == ref["n_lcb"]
    if case["params"]["lcb_scoring"] == 0:                   # (score-weighted LCBs carry scores, and are not extended: S10, S11)
        assert np.asarray(e["lcbs"]["weight"]).tolist() == ref["lcb_weight"]


def test_census():
    """what the families hold, so that a lost case shows"""
    fam = {f: len(C.family(f)) for f in C.FAMILIES}
    assert fam == {"pieces": 59, "rounds": 16, "weights": 12, "merge": 19, "width": 5, "host": 6}
    assert len(NAMES) == 117 and len(PLAIN) == 113 and sum(1 for c in C.all_cases() if c["device"]) == 111
    assert sum(1 for c in C.all_cases() if c["full"]) == 24 and all(c["full"] for c in C.family("merge"))
    assert sorted({c["aim"]["na"] for c in C.family("merge") if "na" in c["aim"]}) == [255, 256, 257, 511, 512, 513]


def test_no_new_match_bridges_two_old_lcbs():
    """two old LCBs that a match between them could join are adjacent and collinear in every genome, so they were one LCB: the
    reference would call such a match "bridged", and without `collinear` the LCB count never falls in a round"""
    for name in NAMES:
        for r in _reference(name)["rounds"]:
            assert all(f["how"] != "bridged" for f in r["fate"]), (name, r["round"])
            if not CASE[name]["params"]["collinear"]:
                assert r["lcb_rechained"] >= r["lcb_before"] and r["old_died"] == 0, (name, r["round"])
