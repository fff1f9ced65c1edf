"""The planted seed-pass inputs of tests/seed_cases.py without a GPU: the oracle's finder is held to the restatement of DESIGN.md
S3 / S4 in tests/seed_ref.py on every case (lengths and starts, canonical order), the restatement is pinned to the brute force of
tests/bruteforce.py on small inputs, and every case is shown to be where it was aimed -- from the reference's facts (key table,
hits, agreement arrays) and the geometry stated in seed_cases.py alone.  A case whose aim does not hold fails here."""
import numpy as np
import pytest

from oracle import pyoracle as O
from tests import bruteforce as B
from tests import seed_cases as C
from tests import seed_ref as R


def reference(case):
    return R.find(case["genomes"], case["pattern"], mode=case["mode"], mask=case["mask"], extend=case["extend"], valid=C.valid_intervals(case))


def oracle(case):
    valid = C.valid_intervals(case)
    if valid is None:
        return O.find_matches(case["genomes"], case["pattern"], mode=case["mode"], mask=case["mask"], extend=case["extend"])
    return O.find_matches_masked(case["genomes"], case["pattern"], valid, mode=case["mode"], mask=case["mask"], extend=case["extend"])


# ---- the reference against the brute force ---------------------------------------------------------------------------------------
def _tiny_set(seed, n, L, rate, inv):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, L, dtype=np.uint8)
    gs = []
    for g in range(n):
        x = anc.copy()
        x[rng.random(L) < rate] ^= 2
        if inv and g == n - 1:
            x[60:160] = C.rc(x[60:160])
        gs.append(x)
    return gs


def _asc(g):
    return "".join("ACGT"[int(c)] for c in g)


@pytest.mark.parametrize("seed,n,w,mode,inv", [(1, 2, 5, "mem", False), (2, 3, 5, "mem", True), (3, 3, 7, "unique", True), (4, 4, 5, "unique", False)])
def test_reference_equals_bruteforce(seed, n, w, mode, inv):
    gs = _tiny_set(seed, n, 260, 0.06, inv)
    if mode == "unique":
        gs[-1] = np.concatenate([gs[-1], gs[-1][20:70]])
    rule = R.MEM if mode == "mem" else R.UNIQUE
    for pat in (C.seed_table(w), C.solid(4), C.palindrome(9, 5)):
        seqs = [_asc(g) for g in gs]
        assert R.as_set(R.find(gs, pat, mode=rule)) == B.brute_matches(seqs, pat, mode=mode)
        assert R.as_set(R.find(gs, pat, mode=rule, extend=False)) == B.brute_matches(seqs, pat, mode=mode, extend=False)
        full = (1 << n) - 1
        assert R.as_set(R.find(gs, pat, mode=rule, mask=full)) == B.brute_matches(seqs, pat, mode=mode, mask=full)


def test_reference_equals_bruteforce_with_valid_intervals():
    gs = _tiny_set(21, 3, 300, 0.04, True)
    valid = [[(1, 120), (160, 300)], [(10, 290)], [(1, 99), (101, 180), (200, len(gs[2]))]]
    for pat in (C.seed_table(5), C.palindrome(9, 5)):
        got = R.find(gs, pat, valid=valid)
        assert R.as_set(got) == B.brute_matches([_asc(g) for g in gs], pat, mode="mem", valid=valid) and len(got["length"]) > 0


def test_patterns_are_what_the_contract_admits():
    seen = set()
    for key, pat in list(C.SOLID.items()) + list(C.SPACED.items()) + list(C.SPAN49.items()):
        offs, span = R.shape(pat)
        s = bin(pat)[2:]
        assert s == s[::-1] and span <= 49 and len(offs) <= 31 and key[1] in (span, len(offs))
        assert O.seed_length(pat) == span and O.seed_weight(pat) == len(offs)
        seen.add((span, len(offs)))
    assert {(s, s) for s in (1, 2, 3, 4, 5, 8, 16)} <= seen and (49, 31) in seen and (49, 5) in seen
    assert {s for s, w in seen if s != w} >= {7, 9, 15, 17, 31, 32, 33, 48, 49}


# ---- aims -----------------------------------------------------------------------------------------------------------------------
def _hits_in(ref, geo, lo, hi):
    """seed hits whose mer lies in [lo, hi) of the partially sorted list"""
    n = 0
    for m, comps, wins, strands in ref["hits"]:
        h = ref["canon"][comps[0]][wins[0]] >> np.uint64(geo["L"])
        n += lo <= int(np.searchsorted(geo["high"], h)) < hi
    return n


def _hit_at(ref, window, comps=None):
    return [h for h in ref["hits"] if h[2][0] == window and (comps is None or h[1] == comps)]


def _diag(h):
    return tuple((s ^ h[3][0], w + h[2][0] if s ^ h[3][0] else w - h[2][0]) for w, s in zip(h[2], h[3]))


def aim_bucket(case, ref):
    aim, name = case["aim"], case["name"]
    geo = C.geometry_of(case)
    assert geo["n"] == C.windows_of(case) > C.TINY_MAX or len(case["genomes"]) > 16
    declined = {c for c, _, _ in geo["declined"]}
    if name.startswith("limit_") and "place" in aim and aim["place"] != "spanning":
        c = aim["chunk"]
        lo, hi = geo["ranges"][c]
        s, e = aim["bucket"]
        assert hi - c * C.CHUNK == C.RANGE_CAP + aim["delta"] and hi == e and (c in declined) == (aim["delta"] > 0)
        assert _hits_in(ref, geo, lo, hi) > 0
        if aim["place"] == "first":
            assert c == 0 and s == 0
        if aim["place"] == "mid":
            assert c >= 1 and s - c * C.CHUNK >= 64
        if aim["place"] == "last":
            assert hi == geo["n"] and c == len(geo["ranges"]) - 2
    elif name.startswith("limit_spanning"):
        c = aim["chunk"]
        assert c in declined and all(geo["ranges"][c + i][0] >= geo["ranges"][c + i][1] for i in (1, 2)) and _hits_in(ref, geo, *geo["ranges"][c]) > 0
    elif name.startswith("bound_"):
        k = aim["edge"] // C.CHUNK
        if aim["distance"] == "n":
            assert geo["bound"][k] == geo["n"] == aim["edge"] + 100 and aim["bucket"][0] < aim["edge"]
        else:
            assert geo["bound"][k] - aim["edge"] == aim["distance"] and (aim["distance"] == 0 or aim["bucket"][0] < aim["edge"])
            assert int(geo["order"][geo["bound"][k]]) == aim["boundary_window"] and _hit_at(ref, aim["boundary_window"])      # (a window of genome 0)
    elif name.startswith("length_"):
        assert geo["n"] == aim["entries"]
    elif name.startswith("overflows_"):
        assert len(declined) >= 3 and all(_hits_in(ref, geo, lo, hi) > 0 for _, lo, hi in geo["declined"])
    elif name.startswith("width_"):
        assert [h[1] for h in _hit_at(ref, aim["once_at"])] == [aim["once"]]
        assert [h[1] for h in _hit_at(ref, aim["others_at"])] == ([aim["others"]] if case["mode"] == C.UNIQUE else [])
        assert int((ref["table"][1] == aim["twice_in"]).sum()) > 0
    elif name.startswith("selfrc_"):
        F, Rv = R.window_mers(case["genomes"][0], case["pattern"])
        assert F[aim["window"]] == Rv[aim["window"]] and _hit_at(ref, aim["window"]) and len(R.shape(case["pattern"])[0]) % 2 == 0
    else:
        raise AssertionError("no aim")
    return len(geo["declined"])


def aim_route(case, ref):
    aim = case["aim"]
    assert C.windows_of(case) == aim["windows"] and C.takes_tiny(case, False) == aim["tiny"] and len(ref["length"]) > 0
    span = ref["span"]
    off = np.cumsum([0] + [max(len(g) - span + 1, 0) for g in case["genomes"]])
    held = {int(off[c] + w) for h in ref["hits"] for c, w in zip(h[1], h[2])}
    assert set(aim.get("hit_windows", ())) <= held
    if "mask" in aim:                                  # hits of other component sets lie around: the same genomes without the mask have them
        free = R.find(case["genomes"], case["pattern"], mode=case["mode"])
        assert {h[0] for h in free["hits"]} >= {3, 5, 6, 7} and {h[0] for h in ref["hits"]} == {aim["mask"]}


def aim_tile(case, ref):
    aim, name = case["aim"], case["name"]
    pair = (0, 1)
    full = tuple(range(len(case["genomes"]))) if case["mode"] != C.PAIRWISE else pair
    if name.startswith("junction_"):
        a, b = aim["hits"]
        ha, hb = _hit_at(ref, a, full), _hit_at(ref, b if aim["d"] else a + 1, full)
        assert ha and hb and (_diag(ha[0]) != _diag(hb[0])) == (aim["d"] > 0)
        if ref["weight"] + 4 >= ref["span"] * 2 // 3:         # (a sparse pattern has chance hits among the windows over the junction)
            assert not any(_hit_at(ref, q, full) for q in range(a + 1, b))
    elif name.startswith("hitgap_"):
        a, b = aim["gap"]
        assert _diag(_hit_at(ref, a)[0]) == _diag(_hit_at(ref, b)[0]) and not any(_hit_at(ref, q) for q in range(a + 1, b))
        assert len([m for m in ref["matches"] if m["qlo"] <= a and m["qhi"] >= b]) == 1
    elif name.startswith("interleaved_"):
        for lo, mask in aim["sets"]:
            assert [h[0] for h in _hit_at(ref, lo + 8)] == [mask], (lo, mask)
        assert len({m for _, m in aim["sets"]}) == len(aim["sets"]) and aim["sets"][-1][0] + 16 <= C.TILE + C.ROUND
    elif name.startswith("phase3_"):
        p, d1, d2 = aim["p"], aim["d1"], aim["d2"]
        hp, h1, h2 = _hit_at(ref, p)[0], _hit_at(ref, p - d1)[0], _hit_at(ref, p - d2)[0]
        assert d1 < d2 <= ref["span"] and hp[0] == h1[0] == h2[0] and _diag(hp) == _diag(h2) != _diag(h1)
        through = [m for m in ref["matches"] if m["qlo"] <= p - d2 and m["qhi"] >= p and m["diag"] == _diag(hp)]
        assert len(through) == (1 if case["extend"] else 0) and (case["extend"] or len(ref["matches"]) == len(ref["hits"]))
    elif name.startswith("transposed_"):
        (q, p), d = aim["hits"], aim["d"]
        hq, hp = _hit_at(ref, q, full), _hit_at(ref, p, full)
        assert len(hq) == len(hp) == 1 and p - q == d <= ref["span"] and not any(_hit_at(ref, x, full) for x in range(q + 1, p))
        hq, hp = hq[0], hp[0]
        rev = hp[3][0] ^ hp[3][1]
        assert hq[0] == hp[0] and rev == (hq[3][0] ^ hq[3][1]) == int(aim["reverse"])
        # a hit of p's diagonal d windows back has its genome-1 window at -d (forward) / +d (reversed); this one has it on the other side
        assert hq[2][1] - hp[2][1] == (-d if rev else d) and _diag(hq) != _diag(hp)
        if case["extend"]:
            for h in (hq, hp):
                assert len([m for m in ref["matches"] if m["diag"] == _diag(h) and m["hits"][0] == h[2][0]]) == 1
    elif name.startswith("slice_edge_"):
        nw0 = len(ref["ok"][0])
        assert _hit_at(ref, aim["last_hit"], (0, 1)) and nw0 - aim["last_hit"] == aim["back"] and _hit_at(ref, 0, (1, 2))
    else:
        raise AssertionError("no aim")


def _match_with_hit(ref, q, which):
    got = [m for m in ref["matches"] if m["comps"] == (0, 1) and m["hits"][which] == q]
    assert len(got) == 1, (q, which, len(got))
    return got[0]


def aim_walk(case, ref):
    aim, name = case["aim"], case["name"]
    span = ref["span"]
    if name.startswith("repeat_"):
        assert len(aim["blocks"]) == 2 * len(aim["lengths"]) and sorted({b["r"] for b in aim["blocks"]}) == aim["lengths"]
        assert aim["lengths"] == C.repeat_lengths(span) or (ref["weight"] < 9 and set(aim["lengths"]) <= set(C.repeat_lengths(span)))
        for b in aim["blocks"]:
            at, q, r = b["at"], b["at"] + b["hit"], b["r"]
            if not case["extend"]:
                assert _hit_at(ref, q)
                continue
            if b["side"] == "led":
                m = _match_with_hit(ref, q, 0)
                D = m["diagonal"]
                assert m["qlo"] == q - r == at and D[q - r:q].all() and not D[q - r - 1], (name, b)
            else:
                m = _match_with_hit(ref, q, -1)
                D = m["diagonal"]
                assert m["qhi"] == q + r and D[q + 1:q + r + 1].all() and not D[q + r + 1], (name, b)
    elif name.startswith("gap_"):
        assert aim["blocks"] and {b["k"] for b in aim["blocks"]} >= {span}
        for b in aim["blocks"]:
            q, (lo, hi), k = b["at"] + b["hit"], (b["at"] + b["run"][0], b["at"] + b["run"][1]), b["k"]
            if not case["extend"]:
                assert _hit_at(ref, q) and not any(_hit_at(ref, x) for x in range(lo, hi + 1))
                continue
            m = _match_with_hit(ref, q, 0)
            D = m["diagonal"]
            assert hi - lo + 1 == k and not D[lo:hi + 1].any() and D[lo - 1] and D[hi + 1], (name, b)
            assert (lo - q == b["f"]) if b["side"] == "right" else (q - hi == b["f"])
            if k < span:
                assert m["qlo"] < lo and m["qhi"] > hi, (name, b)
            elif b["side"] == "right":
                assert m["qhi"] == lo - 1 and any(x["qlo"] == hi + 1 and x["diag"] == m["diag"] for x in ref["matches"]), (name, b)
            else:
                assert m["qlo"] == hi + 1, (name, b)
    elif name.startswith("end_") or name.startswith("components_"):
        g, side = aim["end"]
        L = len(case["genomes"][g])
        got = [(l, s[g]) for l, s in zip(ref["length"], ref["start"]) if sum(x != 0 for x in s) == aim["components"]]
        assert any(abs(s) == 1 if side == "first" else abs(s) + l - 1 == L for l, s in got), (name, got)
        if name.startswith("end_"):
            assert all(len(x) % 64 == aim["residue"] for x in case["genomes"]) and any(s[2] < 0 for s in ref["start"])
    elif name.startswith("selfrc_leads_"):
        w = aim["window"]
        lead = _hit_at(ref, w)
        assert len(lead) == 1 and len(set(lead[0][3])) == 1 and ref["weight"] % 2 == 0          # equal strand flags: a forward hit
        m = [x for x in ref["matches"] if x["qlo"] == w and x["diag"][1][0] == 1]
        assert len(m) == 1 and w < m[0]["hits"][0] <= w + ref["span"] and len(m[0]["comps"]) == aim["components"] and m[0]["length"] > 90
    elif name.startswith("masked_"):
        m = [x for x in ref["matches"] if x["qlo"] <= aim["window"] <= x["qhi"]]
        assert len(m) == 1
        m = m[0]
        if not case["extend"]:                          # every hit alone (side "right"): the agreeing windows are the hits
            held = {h[2][0] for h in ref["hits"]}
            run = next(k for k in range(len(case["genomes"][0])) if aim["window"] + k not in held)
            assert m["qlo"] == m["qhi"] and len(ref["matches"]) == len(ref["hits"]) and aim["side"] == "right"
            assert len(held & set(range(aim["window"], aim["window"] + aim["agree"]))) == aim["agree"] - aim["holes"], name
            m = dict(m, qhi=aim["window"] + run - 1)
            assert aim["holes"] or run == aim["agree"], (name, run)
        else:
            assert m["qhi"] - m["qlo"] + 1 == aim["agree"] and int((~m["diagonal"][m["qlo"]:m["qhi"] + 1]).sum()) == aim["holes"], (name, m["qlo"], m["qhi"])
        if not aim["holes"]:
            assert aim["spot"] == (m["qhi"] + span - 1 + aim["dist"] if aim["side"] == "right" else m["qlo"] - aim["dist"]), (name, m["qlo"], m["qhi"])
        spot = aim["spot"] if not aim["reverse"] else len(case["genomes"][1]) - 1 - aim["spot"]
        if aim["kind"] == "amb":
            assert case["invalid"][1][spot] and int(np.sum(case["invalid"][1])) == 1
        else:
            assert case["contigs"][1][1] in (spot, spot + 1)
    else:
        raise AssertionError("no aim")


def aim_pattern(case, ref):
    assert len(ref["length"]) > 0


AIMS = {"bucket": aim_bucket, "route": aim_route, "tile": aim_tile, "walk": aim_walk, "pattern": aim_pattern}


@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_oracle_equals_reference_and_the_cases_are_where_they_were_aimed(family):
    cases = C.family(family)
    assert len({c["name"] for c in cases}) == len(cases) > 0
    for case in cases:
        assert C.windows_of(case) < 70000, case["name"]
        ref = reference(case)
        ln, st = oracle(case)
        assert ln.tolist() == ref["length"] and st.tolist() == ref["start"], case["name"]
        AIMS[family](case, ref)


def test_callback_cases_have_hits_to_hand_over():
    for case in C.callback_cases():
        assert len(reference(case)["hits"]) > 50
