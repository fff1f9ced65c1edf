"""Planted genome sets for the recursive anchoring (mauvealigner_amd/csrc: recursive.cpp, the segmented
instantiations of seed_pass.hip, the per-gap chain routes of chain_dev.hip).  A recursion batch is planted through the genomes: shared
blocks that the root pass finds are the anchors, what lies between two blocks of one LCB is the gap, base for base.

A case is a dict: name, family, N, genomes (uint8 codes), params (what default_params takes), contigs / invalid (None, or what
set_genomes takes), pos (per genome: name -> (1-based start, length, reverse?) of every shared stretch and block), entry (align |
resume: through mauve_align_lcbs from the root LCB table | progressive: along the given `tree`, against the oracle alone), oracle (False: bitmap cases, which the oracle's whole path cannot take)
and aim -- what the case was planted for, as data that tests/test_recursion_cpu.py checks against the records of
tests/recursion_ref.py and the geometry stated here, never against the product.

Genomes: LCB X = blocks F0 .. Fk, forward in every genome, with the forward gaps between them; LCB Y = blocks R0 .. Rm, reverse
in genome rev_g, with the reverse gaps (given in LCB orientation; genome rev_g holds them mirrored and complemented).  The work
list of level 1 is X's gaps, then Y's.  Weights (root 15): a gap whose mean length is <= 181 wants weight 5 (span 7), <= 1448
weight 7 (span 9), <= 11585 weight 9 (span 13); a stretch shorter than a level's span is not seen by it.

The constants below state the batched form's geometry as recursive.cpp and chain_dev.hip have it; the tests state it, they do not
read it from the library."""
import functools

import numpy as np

from tests.extend_cases import BLOCK, FLANK, ROOT_W, SPAN, Builder, clean_intervals, pattern_of, planted, rc  # noqa: F401

WORD = 32               # bases per packed word of a virtual genome (rec_gather: one thread per word)
MASK_WORD = 64          # bases per word of the virtual ambiguity / contig bitmaps (rec_gather_mask)
GAP_KMAX = 512          # nodes of one gap that the device's greedy step takes
GAP_LINKS = 2560        # nodes x genomes of one gap that it takes
CH_CL_MAX = 48          # matches of one overlap cluster that a thread's registers take
SMALL = 2000            # genomes up to this length: every searched gap is also given to tests/bruteforce.py


# case name -> added to its builder's seed, where chance matches of the light seeds met the planted ones (a stretch whose every mer
# also stands elsewhere in its gap, a chance match that joins a planted node); tests/test_recursion_cpu.py fails a case that needs one
SHIFT = {"rule_root_weight_5": 1, "chain_crossing_tie_first_goes_pq": 1, "chain_overlaps_49": 101, "rule_clamped_to_7": 2,
         "limits_512_nodes_n4": 3, "limits_513_nodes_n4": 2, "limits_427_nodes_n6": 1}
_shift_now = 0


def SB(N, seed):
    return Builder(N, seed + _shift_now)


def shifted(fn):
    """the case that fn builds, built again with the seed shift recorded for its name"""
    @functools.wraps(fn)
    def build(*a, **kw):
        global _shift_now
        case = fn(*a, **kw)
        if case["name"] in SHIFT:
            _shift_now = SHIFT[case["name"]]
            try:
                case = fn(*a, **kw)
            finally:
                _shift_now = 0
        return case
    return build


def span_of(w):
    return SPAN[w] if w in SPAN else len(bin(pattern_of(w))) - 2


def _flip(segs):
    out = []
    for s in reversed(segs):
        out.append(s if s[0] == "s" else ("lit", rc(s[1])) if s[0] == "lit" else (s[0], -s[1]))
    return out


def lit(x):
    return ("lit", np.asarray(x, np.uint8))


def gap(N, base, over=None):
    """a gap: per genome its segments in LCB orientation (`over`: genome -> segments other than `base`)"""
    return [list((over or {}).get(g, base)) for g in range(N)]


def _assemble(b, fwd, rev=(), rev_g=None, block=BLOCK, lead=30):
    nF, nR = (len(fwd) + 1 if fwd else 0), (len(rev) + 1 if rev else 0)
    assert not (nF and nR and rev_g is None)
    for x in ["F%d" % i for i in range(nF)] + ["R%d" % i for i in range(nR)]:
        if x not in b.content:
            b.shared(x, block)
    for g in range(b.N):
        segs = [("s", lead)]
        for i in range(nF):
            segs.append(("F%d" % i, 1))
            if i < len(fwd):
                segs += fwd[i][g]
        if nF and nR:
            segs.append(("s", 40))
        part = []
        for i in range(nR):
            part.append(("R%d" % i, 1))
            if i < len(rev):
                part += rev[i][g]
        segs += _flip(part) if g == rev_g else part
        segs.append(("s", 30))
        b.genome(g, [s for s in segs if not (s[0] == "s" and s[1] == 0)])


def _case(name, family, b, aim, min_gap=40, entry="align", oracle=True, contigs=None, invalid=None, built=None, **params):
    gen, pos = built if built is not None else b.build()
    p = {"seed_weight": ROOT_W, "lcb_weight": -1, "extend_lcbs": 0, "max_extension_iters": 0, "collinear": 0, "lcb_scoring": 0, "recursive": 1,
         "gapped": 0, "min_recursive_gap": min_gap}
    p.update(params)
    return {"name": name, "family": family, "N": b.N, "genomes": gen, "pos": pos, "params": p, "aim": aim, "entry": entry, "oracle": oracle,
            "contigs": contigs, "invalid": invalid}


# ---- rule --------------------------------------------------------------------------------------------------------------------------
@shifted
def _rule_mx(plus, where, recursive=1):
    """the longest side of the gap is exactly min_recursive_gap (+ plus) bases: in genome 0, in the last genome, or in the last
    genome where the LCB is reverse; the other sides have 30; P (8 bases) waits for the weight-5 level"""
    N = 3
    b = SB(N, 2100 + 10 * plus + {"g0": 0, "last": 1, "rev": 2}[where])
    b.shared("P", 8)
    long_g = 0 if where == "g0" else 2
    g = gap(N, [("s", 11), ("P", 1), ("s", 11)], {long_g: [("s", 16), ("P", 1), ("s", 16 + plus)]})
    if where == "rev":
        _assemble(b, [], [g], 2)
    else:
        _assemble(b, [g])
    if not recursive:
        return _case("rule_recursive_off", "rule", b, {"absent": ["P"], "batches": [], "records": 0, "blocks": 2}, recursive=0)
    aim = {"blocks": 2, "lens": [(1, 0, [40 + plus if q == long_g else 30 for q in range(N)])]}
    if plus:
        aim.update(found=[("P", 1)], batches=[(1, 5, 1)])
    else:
        aim.update(absent=["P"], batches=[], why=[(1, 0, "short")])
    return _case("rule_mx_%d_%s" % (40 + plus, where), "rule", b, aim)


@shifted
def _rule_root(w):
    """root weight 7: one level at 5 and none below; root weights 6 and 5: nothing is searched (w - 2 < 5)"""
    N = 3
    b = SB(N, 2150 + w)
    b.shared("P", 8)
    _assemble(b, [gap(N, [("s", 45), ("P", 1), ("s", 47)], {1: [("s", 42), ("P", 1), ("s", 51)]})])
    aim = {"levels": [5] if w == 7 else [], "stops": "w<5"}
    aim.update({"found": [("P", 1)]} if w == 7 else {"absent": ["P"]})
    return _case("rule_root_weight_%d" % w, "rule", b, aim, seed_weight=w)


@shifted
def _rule_clamp():
    """root weight 9; the gap's mean length (1500) wants weight 9, which w_prev - 2 clamps to 7"""
    N = 3
    b = SB(N, 2170)
    b.shared("T", 12)                                              # (below the root seed's span of 13)
    _assemble(b, [gap(N, [("s", 740), ("T", 1), ("s", 748)], {1: [("s", 733), ("T", 1), ("s", 762)]})])
    return _case("rule_clamped_to_7", "rule", b, {"found": [("T", 1)], "first_batch": (1, 7, 1), "raw": (1, 0, 9)}, min_gap=200, seed_weight=9)


@shifted
def _rule_side(d):
    """the shortest side is span - 1, span, span + 1 at weight 7 (span 9).  At span the stretch IS genome 2's whole gap: both
    sub-gaps are empty there, and the next level stops on side<span"""
    N = 3
    b = SB(N, 2180 + d + 1)
    b.shared("P", 9)
    short = [("s", 8)] if d < 0 else [("P", 1)] + ([("s", 1)] if d else [])
    _assemble(b, [gap(N, [("s", 135), ("P", 1), ("s", 136)], {1: [("s", 130), ("P", 1), ("s", 141)], 2: short})])
    aim = {"blocks": 2, "lens": [(1, 0, [280, 280, 9 + d])]}
    if d < 0:
        aim.update(absent=["P"], batches=[], why=[(1, 0, "side<span")])
    else:
        aim.update(found=[("P", 1)], batches=[(1, 7, 1)], why=[(2, 0, "side<span"), (2, 1, "side<span")])
    return _case("rule_side_span%+d" % d, "rule", b, aim)


@shifted
def _rule_empty():
    """one side empty: the two anchors are adjacent in genome 2"""
    N = 3
    b = SB(N, 2190)
    b.shared("P", 8)
    _assemble(b, [gap(N, [("s", 25), ("P", 1), ("s", 27)], {2: []})])
    return _case("rule_one_side_empty", "rule", b, {"blocks": 2, "lens": [(1, 0, [60, 60, 0])], "batches": [], "why": [(1, 0, "side<span")]})


# ---- levels ------------------------------------------------------------------------------------------------------------------------
@shifted
def _levels_three():
    """a 2 kb gap: S9 (13 bases) is seen at weight 9, S7 (12 bases) at weight 7 inside the left sub-gap, S5 (8 bases) at weight 5
    inside the sub-gap in front of S7; the sub-gaps of that level stop on w<5"""
    N = 3
    b = SB(N, 2200)
    b.shared("S9", 13); b.shared("S7", 12); b.shared("S5", 8)
    _assemble(b, [gap(N, [("s", 20), ("S5", 1), ("s", 25), ("S7", 1), ("s", 330), ("S9", 1), ("s", 1600)],
                      {1: [("s", 24), ("S5", 1), ("s", 20), ("S7", 1), ("s", 340), ("S9", 1), ("s", 1590)]})])
    return _case("levels_9_7_5", "levels", b, {"found": [("S9", 1), ("S7", 2), ("S5", 3)], "levels": [9, 7, 5], "stops": "w<5"})


@shifted
def _levels_classes():
    """one level whose gaps want 9, 5, 7 and 9: three batches (5, 7, 9) on the same buffers"""
    N = 3
    b = SB(N, 2210)
    b.shared("T9", 14); b.shared("T5", 8); b.shared("T7", 10); b.shared("U9", 14)
    _assemble(b, [gap(N, [("s", 700), ("T9", 1), ("s", 790)]), gap(N, [("s", 25), ("T5", 1), ("s", 27)]),
                  gap(N, [("s", 140), ("T7", 1), ("s", 150)]), gap(N, [("s", 800), ("U9", 1), ("s", 690)])])
    return _case("levels_three_classes", "levels", b, {"found": [("T9", 1), ("T5", 1), ("T7", 1), ("U9", 1)], "blocks": 5,
                                                        "level1": [(1, 5, 1), (1, 7, 1), (1, 9, 2)]})


@shifted
def _nothing():
    N = 3
    b = SB(N, 2221)
    _assemble(b, [gap(N, [("s", 45)], {1: [("s", 43)]})])
    return _case("finds_nothing", "levels", b, {"blocks": 2, "batches": [(1, 5, 1)], "silent": True})


# ---- gather ------------------------------------------------------------------------------------------------------------------------
def _two_gaps(b, N, g_edge, first, second, rev_g):
    gs = [gap(N, [("s", 18), ("P", 1), ("s", 20)], {g_edge: first}), gap(N, [("s", 19), ("Q", 1), ("s", 19)], {g_edge: second})]
    if rev_g is None:
        _assemble(b, gs)
    else:
        _assemble(b, [], gs, rev_g)


@shifted
def _gather_seg(v, g_edge, rev_g=None):
    """genome g_edge: gap 0 has exactly v bases (gap 1 starts at virtual base v) and P on its last bases, Q on gap 1's first"""
    N = 3
    b = SB(N, 2300 + v + 1000 * g_edge + 3000 * (0 if rev_g is None else rev_g))
    b.shared("P", 12); b.shared("Q", 12)                            # (12 bases, 6 windows: a weight-5 mer is seldom unique in 256 bases)
    _two_gaps(b, N, g_edge, [("s", v - 12), ("P", 1)], [("Q", 1), ("s", 38)], rev_g)
    aim = {"found": [("P", 1), ("Q", 1)], "batches": [(1, 5, 2)], "blocks": 3, "seg": [(1, 5, g_edge, 1, v)]}
    return _case("gather_seg_%d_g%d_%s" % (v, g_edge, "fwd" if rev_g is None else "rev%d" % rev_g), "gather", b, aim)


@shifted
def _gather_total(T, g_edge, rev_g=None):
    """genome g_edge's virtual length is exactly T bases, P on the last of them"""
    N = 3
    b = SB(N, 2400 + T + (0 if rev_g is None else 25 + 25 * rev_g) + 500 * g_edge)
    b.shared("P", 12); b.shared("Q", 12)
    gs = [gap(N, [("s", 19), ("Q", 1), ("s", 19)]), gap(N, [("s", 18), ("P", 1), ("s", 20)], {g_edge: [("s", T - 50 - 12), ("P", 1)]})]
    if rev_g is None:
        _assemble(b, gs)
    else:
        _assemble(b, [], gs, rev_g)
    return _case("gather_total_%d_g%d_%s" % (T, g_edge, "fwd" if rev_g is None else "rev%d" % rev_g), "gather", b,
                 {"found": [("P", 1), ("Q", 1)], "batches": [(1, 5, 2)], "total": [(1, 5, g_edge, T)]})


@shifted
def _gather_inside(rev_g=None):
    """P across the 32-base border and Q across the 64-base border of the virtual genomes 0 and 1, inside one gap"""
    N = 3
    b = SB(N, 2450 + (0 if rev_g is None else rev_g))
    b.shared("P", 12); b.shared("Q", 12)
    g = gap(N, [("s", 26), ("P", 1), ("s", 20), ("Q", 1), ("s", 30)], {1: [("s", 25), ("P", 1), ("s", 22), ("Q", 1), ("s", 29)],
                                                                      2: [("s", 20), ("P", 1), ("s", 20), ("Q", 1), ("s", 20)]})
    if rev_g is None:
        _assemble(b, [g])
    else:
        _assemble(b, [], [g], rev_g)
    return _case("gather_across_words_%s" % ("fwd" if rev_g is None else "rev%d" % rev_g), "gather", b,
                 {"found": [("P", 1), ("Q", 1)], "batches": [(1, 5, 1)], "across": [("P", 0, 32), ("P", 1, 32), ("Q", 0, 64), ("Q", 1, 64)]})


@shifted
def _gather_realstart(off, rev_g=None):
    """the gap's real start lies on a word border of the resident genomes (0-based base 320), and one base off it; in a reverse gap
    the base read first is the one at start + length - 1"""
    N = 3
    b = SB(N, 2470 + off + (0 if rev_g is None else 10 * rev_g))
    b.shared("P", 12)
    g = gap(N, [("s", 18), ("P", 1), ("s", 20)])
    if rev_g is None:
        _assemble(b, [g], lead=20 + off)
    else:
        _assemble(b, [], [g], rev_g, lead=20 + off)
    return _case("gather_real_start_%d_%s" % (320 + off, "fwd" if rev_g is None else "rev%d" % rev_g), "gather", b, {"found": [("P", 1)], "batches": [(1, 5, 1)], "lo": [(1, 0, [321 + off] * N)]})


# ---- segments ----------------------------------------------------------------------------------------------------------------------
@shifted
def _seg_dup(twin):
    """the same 9 bases planted in two gaps of one batch (twin: the second copy in a gap of another weight class)"""
    N = 3
    b = SB(N, 2500 + twin)
    b.shared("D1", 9)
    b.content["D2"] = b.content["D1"].copy()
    second = gap(N, [("s", 140), ("D2", 1), ("s", 151)]) if twin else gap(N, [("s", 22), ("D2", 1), ("s", 20)])
    _assemble(b, [gap(N, [("s", 20), ("D1", 1), ("s", 21)]), second])
    return _case("segments_same_stretch_%s" % ("two_classes" if twin else "one_batch"), "segments", b,
                 {"found": [("D1", 1), ("D2", 1)], "level1": [(1, 5, 1), (1, 7, 1)] if twin else [(1, 5, 2)], "same_content": ("D1", "D2")})


@shifted
def _seg_seam():
    """H1 stands at the end of gap 0 and H2 at the start of gap 1 on one virtual diagonal, two bases apart that agree in the virtual
    genomes: genomes 0 and 2 hold H1 a | b H2, genome 1 holds H1 | a b H2.  (The two bases cannot be split the same way in every
    genome: a base that all genomes share next to a block belongs to the block's root match.)  Without the segment rule one match
    of |H1| + 2 + |H2| = 18; with it H1 (8) and b H2 (9, cropped at gap 1's start in genomes 0 and 2)"""
    N = 3
    b = SB(N, 2520)
    H1, H2 = b.shared("H1", 8), b.shared("H2", 8)
    a = (int(H1[-1]) + 1) % 4
    c = (a + 1) % 4
    _assemble(b, [gap(N, [("s", 30), ("H1", 1), lit([a])], {1: [("s", 33), ("H1", 1)]}),
                  gap(N, [lit([c]), ("H2", 1), ("s", 40)], {1: [lit([a, c]), ("H2", 1), ("s", 37)]})])
    return _case("segments_seam", "segments", b, {"batches": [(1, 5, 2)], "found": [("H1", 1)], "seam": ("H1", "H2", 18, 9), "blocks": 3})


@shifted
def _seg_straddle():
    """one weight-5 window T (1101011) across the border of gaps 0 | 1: genomes 0 and 2 hold T0 T1 y | T3 T4 T5 T6, genome 1 holds
    T0 T1 T2 T3 y' | T5 T6; the bases next to the border (y, y', T3 against T5) stand on don't-care offsets 2 and 4 or disagree,
    so the root matches end where they should, and the care bases agree.  The halves are too short to be seen alone"""
    N = 3
    b = SB(N, 2531)
    T = b.rng.integers(0, 4, 7, dtype=np.uint8)
    T[5] = (T[3] + 1) % 4
    y0, y1 = (int(T[2]) + 1) % 4, (int(T[4]) + 2) % 4
    if y0 == y1:
        y1 = (y1 + 1) % 4
    _assemble(b, [gap(N, [("s", 40), lit([T[0], T[1], y0])], {1: [("s", 38), lit([T[0], T[1], T[2], T[3], y1])]}),
                  gap(N, [lit(T[3:]), ("s", 40)], {1: [lit(T[5:]), ("s", 41)]})])
    return _case("segments_straddle", "segments", b, {"batches": [(1, 5, 2)], "straddle": True, "blocks": 3})


@shifted
def _seg_crop(side, rev_g=None):
    """C (12 bases) runs 3 bases into the anchor next to the gap in genome 1: the match is cropped at the gap's end there (left:
    its start; right: its end; in a reverse gap the virtual right end is the real left end)"""
    N = 3
    b = SB(N, 2540 + (side == "right") + (0 if rev_g is None else 2))
    Cc = b.shared("C", 12)
    blocks = "R" if rev_g is not None else "F"
    if side == "left":
        Cc[:3] = b.shared(blocks + "0", BLOCK)[-3:]
        g = gap(N, [("s", 15), ("C", 1), ("s", 30)], {1: [lit(Cc[3:]), ("s", 41)], 2: [("s", 17), ("C", 1), ("s", 26)]})
        want = (9, [19, 1, 21])
    else:
        Cc[-3:] = b.shared(blocks + "1", BLOCK)[:3]
        g = gap(N, [("s", 30), ("C", 1), ("s", 15)], {1: [("s", 41), lit(Cc[:-3])], 2: [("s", 26), ("C", 1), ("s", 17)]})
        want = (9, [31, 42, 27])
    if rev_g is None:
        _assemble(b, [g])
    else:
        _assemble(b, [], [g], rev_g)
    return _case("segments_crop_%s_%s" % (side, "fwd" if rev_g is None else "rev%d" % rev_g), "segments", b,
                 {"batches": [(1, 5, 1)], "blocks": 2, "local": [(1, 0, want)]})


# ---- count -------------------------------------------------------------------------------------------------------------------------
@shifted
def _count(K, w):
    """K gaps in one batch at weight w; the first, the last and one middle gap hold a stretch"""
    N = 2 if K > 1000 else 3
    L, glen, mg, at = (8, 45, 40, 12) if w == 5 else (10, 190, 150, 88)       # (the sub-gaps of a holder stay below min_recursive_gap)
    b = SB(N, 2600 + K + w)
    holders = sorted({0, K // 2, K - 1})
    gaps = []
    for k in range(K):
        if k in holders:
            b.shared("P%d" % k, L)
            gaps.append([[("s", at + g), ("P%d" % k, 1), ("s", glen - at - g - L)] for g in range(N)])
        else:
            gaps.append([[("s", glen)] for g in range(N)])
    _assemble(b, gaps, block=30)
    return _case("count_%d_w%d" % (K, w), "count", b, {"found": [("P%d" % k, 1) for k in holders], "level1": [(1, w, K)], "blocks": K + 1}, min_gap=mg)


# ---- chain -------------------------------------------------------------------------------------------------------------------------
@shifted
def _chain(name, seed, lens, orders, aim, rev_g=None, N=3):
    """one gap of about 300 bases (weight 7); orders[g]: the stretches of genome g as (name, +1 | -1), in LCB orientation"""
    b = SB(N, seed)
    for x, n in lens.items():
        b.shared(x, n)
    g = []
    for q in range(N):
        segs = [("s", 30 + q)]
        for i, (x, o) in enumerate(orders[q]):
            segs += [(x, o), ("s", 25 + i + q)]
        g.append(segs + [("s", 160)])
    if rev_g is None:
        _assemble(b, [g])
    else:
        _assemble(b, [], [g], rev_g)
    aim = dict(aim, first_batch=(1, 7, 1))
    return _case(name, "chain", b, aim, min_gap=100)


def _chain_cases():
    f = lambda *names: [(x, 1) for x in names]
    out = [
        _chain("chain_reverse_stretch_dropped", 2700, {"P": 12, "Q": 12}, [f("P", "Q"), [("P", 1), ("Q", -1)], f("P", "Q")],
               {"found": [("P", 1)], "non_forward": ["Q"], "absent": ["Q"]}),
        _chain("chain_forward_in_a_reverse_lcb", 2701, {"P": 12, "Q": 12}, [f("P", "Q")] * 3, {"found": [("P", 1), ("Q", 1)], "negative": [("P", 1)]}, rev_g=1),
        _chain("chain_crossing_lighter_goes", 2702, {"P": 12, "Q": 10}, [f("P", "Q"), f("Q", "P"), f("P", "Q")],
               {"found": [("P", 1)], "deleted": ["Q"]}),
        _chain("chain_crossing_tie_first_goes_pq", 2703, {"P": 10, "Q": 10}, [f("P", "Q"), f("Q", "P"), f("P", "Q")],
               {"found": [("Q", 1)], "deleted": ["P"], "tie": "P"}),
        _chain("chain_crossing_tie_first_goes_qp", 2704, {"P": 10, "Q": 10}, [f("Q", "P"), f("P", "Q"), f("Q", "P")],
               {"found": [("P", 1)], "deleted": ["Q"], "tie": "Q"}),
        _chain("chain_neighbours_merge_and_outweigh", 2705, {"A": 10, "X": 9, "B": 10, "D": 15}, [f("A", "X", "B", "D"), f("D", "A", "B", "X"), f("A", "X", "B", "D")],
               {"found": [("A", 1), ("B", 1)], "deleted": ["X", "D"], "deleted_order": ["X", "D"]}),
    ]
    return out + [_overlap_allbut1()] + [_overlap_chain(n) for n in (2, 3, CH_CL_MAX, CH_CL_MAX + 1)]


@shifted
def _overlap_allbut1():
    """P (14 bases) and Q (12) overlap in genome 1 only, by all but 1 column of Q: Q begins with P's last 11 bases, and genome 1
    holds P and then Q's last base alone.  The elimination takes 11 of Q's 12 columns: one column is left, and it stays in the chain.
    (The overlap by 1 column is chain_overlaps_2.)"""
    N = 3
    b = SB(N, 2790)
    P, Q = b.shared("P", 14), b.shared("Q", 12)
    Q[:11] = P[-11:]
    if Q[11] == P[2]:                                               # (Q's last base is not how P would go on once more)
        Q[11] = (Q[11] + 1) % 4
    g = [[("s", 30), ("P", 1), ("s", 25), ("Q", 1), ("s", 26), ("s", 160)], [("s", 31), ("P", 1), ("tail", "Q", 1, 11), ("s", 200)],
         [("s", 32), ("P", 1), ("s", 27), ("Q", 1), ("s", 25), ("s", 160)]]
    _assemble(b, [g])
    return _case("chain_overlap_all_but_1", "chain", b, {"first_batch": (1, 7, 1), "found": [("P", 1)], "cropped_to": ("Q", 11, 1), "cluster": (1, 2)}, min_gap=100)


def _clean_pieces(rng, n, L, pat):
    """n pieces of L bases, the last base of each equal to the first of the next, no two equal neighbours inside a piece (off its
    diagonal a piece disagrees with itself) -> (the pieces joined, the same with one base of every doubled pair).  Built base by
    base so that no mer of the two sequences occurs twice, on either strand, but for the planted pairs (a window inside one piece):
    a chance hit between them would join the overlap cluster"""
    from tests import seed_ref as S
    span = len(bin(pat)) - 2
    canon = lambda x: int(np.minimum(*S.window_mers(np.array(x[-span:], np.uint8), pat))[0])
    while True:
        whole, one, seen, stuck = [int(rng.integers(0, 4))], [], set(), False
        one.append(whole[0])
        for k in range(1, n * L):
            t = k % L
            if t == 0:                                             # the doubled base: in `whole` only
                cand = [whole[-1]]
            else:
                cand = [(whole[-1] + d) % 4 for d in rng.permutation([1, 2, 3])]
            for c in cand:
                w2, o2 = whole + [c], (one + [c] if t else one)
                new = []
                if len(w2) >= span:
                    new.append(canon(w2))
                if t and len(o2) >= span and not (t >= span - 1 and new and canon(o2) == new[0]):
                    new.append(canon(o2))
                if len(set(new)) == len(new) and not (set(new) & seen):
                    whole, one = w2, o2
                    seen |= set(new)
                    break
            else:
                stuck = True
                break
        if not stuck:
            return np.array(whole, np.uint8), np.array(one, np.uint8)


@shifted
def _overlap_chain(n):
    """n matches of 14 bases (weight 9, span 13), each overlapping the next by 1 column in genome 1 only: genomes 0 and 2 hold U0 U1 ...
    with the last base of every piece equal to the first of the next (a doubled base), genome 1 holds one base of each pair"""
    N, L = 3, 14
    b = SB(N, 2750 + n)
    whole, one = _clean_pieces(b.rng, n, L, pattern_of(9))
    pad = 2200 - len(whole) - 60                                   # (genome 1's side stays short: few spacer windows that could meet a piece by chance)
    _assemble(b, [gap(N, [("s", 30), lit(whole), ("s", 30 + pad)], {1: [("s", 32), lit(one), ("s", 29)], 2: [("s", 35), lit(whole), ("s", 26 + pad)]})])
    want = [(L, [31 + L * i, 33 + (L - 1) * i, 36 + L * i]) for i in range(n)]
    return _case("chain_overlaps_%d" % n, "chain", b, {"first_batch": (1, 9, 1), "local_all": (1, 0, want), "cluster": (1, n)}, min_gap=100)


# ---- limits ------------------------------------------------------------------------------------------------------------------------
@shifted
def _limits(n, N):
    """one gap with n mutually non-collinear nodes: n stretches of L bases in the opposite order in genome 1, two bases apart (two
    to four in the genomes behind genome 1, so that no two genomes share a junction).  All weigh the same: the collinear rule
    deletes them from the left, the last one stays"""
    L = 18 if N == 4 else 20
    b = SB(N, 2800 + n + N)
    names = ["n%d" % i for i in range(n)]
    for x in names:
        b.shared(x, L)
    g = []
    for q in range(N):
        sep = 2 if q < 2 else 2 + (q - 1) % 3
        segs = [("s", 10)]
        for x in (reversed(names) if q == 1 else names):
            segs += [(x, 1), ("s", sep)]
        g.append(segs + [("s", max(10, 1460 - 10 - n * (L + sep)))])
    _assemble(b, [g])
    return _case("limits_%d_nodes_n%d" % (n, N), "limits", b, {"first_batch": (1, 9, 1), "nodes": (1, 0, n), "survivor": names[-1],
                                                               "beyond": n > GAP_KMAX or n * N > GAP_LINKS}, min_gap=100)


# ---- width -------------------------------------------------------------------------------------------------------------------------
@shifted
def _width(N):
    """N genomes: one forward gap with P and one gap with V that is reverse in the last genome (bit 31 at N = 32).  Weight 7 and 16
    bases: a weight-5 mer is hardly ever unique in every one of 32 gaps"""
    b = SB(N, 2900 + N)
    b.shared("P", 16); b.shared("V", 16)
    _assemble(b, [[[("s", 80 + g % 5), ("P", 1), ("s", 94 - g % 5)] for g in range(N)]], [[[("s", 85 + g % 4), ("V", 1), ("s", 89 - g % 4)] for g in range(N)]], N - 1)
    return _case("width_n%d" % N, "width", b, {"found": [("P", 1), ("V", 1)], "level1": [(1, 7, 2)], "negative": [("V", N - 1)]}, min_gap=150)


# ---- bitmaps -----------------------------------------------------------------------------------------------------------------------
@shifted
def _bitmap(kind, where, rev):
    """genome 1 carries an ambiguous base / a contig start next to or inside P (10 bases; weight 5, span 7), in a forward gap and in
    a gap that is reverse in genome 1.  `where` is told in LCB orientation"""
    N = 3
    b = SB(N, 3000 + rev)
    b.shared("P", 10)
    g = gap(N, [("s", 20), ("P", 1), ("s", 20)])
    if rev:
        _assemble(b, [], [g], 1)
    else:
        _assemble(b, [g])
    gen, pos = b.build()
    s = pos[1]["P"][0] - 1                                          # 0-based real start of P in genome 1
    first, last = (s + 9, s) if rev else (s, s + 9)                 # P's first / last base in LCB orientation
    step = -1 if rev else 1
    glo = pos[1]["R1" if rev else "F0"][0] - 1 + BLOCK              # the gap's real left end in genome 1, 0-based
    gfirst = glo + 49 if rev else glo                               # its first base in LCB orientation
    inv = con = None
    if kind == "invalid":
        at = {"inside": first + 4 * step, "front": first - step, "behind": last + step}[where]
        inv = [np.zeros(len(x), bool) for x in gen]
        inv[1][at] = True
    else:
        base = {"inside": first + 4 * step, "first": first, "gapfirst": gfirst}[where]      # the boundary lies in front of it (LCB orientation)
        at = base + 1 if rev else base                              # ... so on a reverse gap the contig starts one base further on
        con = [[0, at] if q == 1 else [0] for q in range(N)]
    whole = where in ("front", "behind", "first", "gapfirst")
    aim = {"batches": [(1, 5, 1)], "found" if whole else "absent": [("P", 1)] if whole else ["P"]}
    return _case("bitmap_%s_%s_%s" % (kind, where, "rev" if rev else "fwd"), "bitmaps", b, aim, oracle=False, contigs=con, invalid=inv, built=(gen, pos))


@shifted
def _bitmap_word(bit):
    """the flagged base of genome 1 at bit 63 | 64 of the virtual mask words: gap 1 starts at virtual base 50, P at its local
    offset 14 (virtual 64 .. 73); the ambiguous base right in front of P (63: P whole) or on its first base (64: 9 bases left)"""
    N = 3
    b = SB(N, 3050)
    b.shared("P", 10); b.shared("Q", 8)
    _assemble(b, [gap(N, [("s", 21), ("Q", 1), ("s", 21)]), gap(N, [("s", 14), ("P", 1), ("s", 26)])])
    gen, pos = b.build()
    inv = [np.zeros(len(x), bool) for x in gen]
    inv[1][pos[1]["P"][0] - 1 + (bit - 64)] = True
    aim = {"batches": [(1, 5, 2)], "seg": [(1, 5, 1, 1, 50)], "mask_bit": (1, 1, "P", bit)}
    aim.update({"found": [("P", 1), ("Q", 1)]} if bit == 63 else {"found": [("Q", 1)], "absent": ["P"], "local": [(1, 1, (9, [16, 16, 16]))]})
    return _case("bitmap_invalid_at_mask_bit_%d" % bit, "bitmaps", b, aim, oracle=False, invalid=inv, built=(gen, pos))


# ---- entries -----------------------------------------------------------------------------------------------------------------------
def _entries(cases):
    by = {c["name"]: c for c in cases}
    out = []

    def variant(base, tag, entry="align", **params):
        c = dict(by[base])
        c["params"] = dict(c["params"], **params)
        c.update(name="entry_%s_%s" % (tag, base), family="entries", entry=entry, aim={k: v for k, v in c["aim"].items() if k in ("found", "absent")})
        out.append(c)

    for base in ("rule_mx_41_g0", "chain_crossing_lighter_goes", "chain_neighbours_merge_and_outweigh"):
        for u in (1, 0):
            variant(base, "gapped_unaligned%d" % u, gapped=1, add_unaligned=u)
    out += [_entry_extension(0), _entry_extension(1)]
    for base in ("gather_seg_64_g1_rev1", "chain_overlaps_3"):
        variant(base, "resume", entry="resume", gapped=1)
    return out


@shifted
def _entry_extension(rev):
    """four extension rounds in front of the recursion.  The extension searches outside the LCB extents only, so what it can give
    the recursion is a new gap: E (20 bases: the root seed of span 21 misses it, round 0's of span 19 finds it) stands 60 bases in
    front of the LCB and joins it; the gap E .. block 0 then holds P2, the gap block 0 .. block 1 holds P, and the recursion has two
    gaps where it would have one.  rev: the LCB is reverse in the last genome"""
    N = 3
    b = SB(N, 3200 + rev)
    for x, n in (("E", 20), ("P2", 12), ("P", 12), ("K0", BLOCK), ("K1", BLOCK)):      # (P2, P: inside the LCB extent from round 1 on, so no round sees them)
        b.shared(x, n)
    for g in range(N):
        part = [("E", 1), ("s", 25 + g), ("P2", 1), ("s", 27 - g), ("K0", 1), ("s", 18 + g), ("P", 1), ("s", 24 - g), ("K1", 1)]
        b.genome(g, [("s", 30)] + (_flip(part) if rev and g == N - 1 else part) + [("s", 30)])
    aim = {"found": [("P2", 1), ("P", 1)], "batches": [(1, 5, 2)], "extension": ("E", 13)}
    return _case("entry_extension_in_front_%s" % ("rev" if rev else "fwd"), "entries", b, aim, extend_lcbs=1, max_extension_iters=4)


@shifted
def _progressive(rev):
    """three genomes along the tree ((1, 2), 0): all three share C; genomes 1 and 2 also share A . gap . B with P (12 bases) in the
    gap (reverse-complemented as a whole in genome 2 when rev), genome 0 has nothing like it.  The root node anchors C; the node over
    {1, 2} gets the stretch in front of it, anchors A and B and runs the recursion with gmap = {1, 2}"""
    from tests.progressive_cases import tree_of
    b = SB(3, 3100 + rev)
    for x in "ABC":
        b.shared(x, BLOCK)
    b.shared("P", 12)
    part = [("A", 1), ("s", 20), ("P", 1), ("s", 22), ("B", 1)]
    part2 = [("A", 1), ("s", 18), ("P", 1), ("s", 25), ("B", 1)]
    # (the builder makes the flanks disagree between ITS genomes 0 and 1: they are genomes 1 and 2 of the case)
    b.genome(0, [("s", 30)] + part + [("s", 40), ("C", 1), ("s", 30)])
    b.genome(1, [("s", 35)] + (_flip(part2) if rev else part2) + [("s", 44), ("C", 1), ("s", 30)])
    b.genome(2, [("s", 400), ("C", 1), ("s", 60)])
    gen, pos = b.build()
    c = _case("entry_progressive_%s" % ("rev" if rev else "fwd"), "entries", b, {"progressive": True}, entry="progressive", gapped=1,
              built=([gen[2], gen[0], gen[1]], [pos[2], pos[0], pos[1]]))
    c["tree"] = tree_of(3, [(1, 2), (0, 3)])
    return c


FAMILIES = ("rule", "levels", "gather", "segments", "count", "chain", "limits", "width", "bitmaps", "entries")


@functools.lru_cache(maxsize=None)
def _all():
    cases = [_rule_mx(p, w) for p in (0, 1) for w in ("g0", "last", "rev")]
    cases += [_rule_root(w) for w in (7, 6, 5)] + [_rule_clamp()] + [_rule_side(d) for d in (-1, 0, 1)] + [_rule_empty(), _rule_mx(1, "g0", recursive=0)]
    cases += [_levels_three(), _levels_classes(), _nothing()]
    edges = [e + d for e in (WORD, MASK_WORD, 256) for d in (-1, 0, 1)]
    cases += [_gather_seg(v, g, r) for g in (0, 1) for v in edges for r in (None, 1, 2)]
    cases += [_gather_total(T, g, r) for g in (0, 1) for T in (96, 97) for r in (None, 1, 2)]
    cases += [_gather_inside(r) for r in (None, 1, 2)] + [_gather_realstart(o, r) for o in (0, 1) for r in (None, 1, 2)]
    cases += [_seg_dup(0), _seg_dup(1), _seg_seam(), _seg_straddle()] + [_seg_crop(s, r) for s, r in (("left", None), ("right", None), ("left", 1), ("right", 1))]
    cases += [_count(K, 7) for K in (1, 2, 3, 4)] + [_count(K, 5) for K in (63, 64, 255, 256, 257)] + [_count(K, 7) for K in (1023, 1024)]
    cases += _chain_cases()
    cases += [_limits(n, N) for n, N in ((80, 32), (81, 32), (426, 6), (427, 6), (512, 4), (513, 4))]
    cases += [_width(N) for N in (2, 3, 5, 16, 17, 32)]
    cases += [_bitmap("invalid", w, r) for w in ("inside", "front", "behind") for r in (0, 1)]
    cases += [_bitmap("contig", w, r) for w in ("inside", "first", "gapfirst") for r in (0, 1)]
    cases += [_bitmap_word(63), _bitmap_word(64)]
    cases += _entries(cases) + [_progressive(0), _progressive(1)]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def family(name):
    return [c for c in _all() if c["family"] == name]


def all_cases():
    return list(_all())


NOTHING = "finds_nothing"


@functools.lru_cache(maxsize=None)
def _reference(name):
    from tests import extend_ref as E, recursion_ref as R, seed_ref as S
    case = next(c for c in _all() if c["name"] == name)
    p, N = case["params"], case["N"]
    clean = clean_intervals(case)
    root = S.find(case["genomes"], pattern_of(p["seed_weight"]), S.MEM, (1 << N) - 1, True, clean)
    iters = p["max_extension_iters"] if p["extend_lcbs"] else 0
    ext = E.extend(case["genomes"], root["length"], root["start"], pattern_of, p["seed_weight"], p["lcb_weight"], iters, bool(p["collinear"]), clean)
    anchors = list(zip(ext["anchor_length"], ext["anchor_start"]))
    ref = R.recurse(case["genomes"], anchors, ext["anchor_lcb"], pattern_of, span_of, p["seed_weight"], p["min_recursive_gap"], clean, bool(p["recursive"]))
    ref.update(mums=(root["length"], root["start"]), n_lcb=ext["n_lcb"], lcb_weight=ext["lcb_weight"],
               ext_rounds=[(q["weight"], len(q["new"]), q["kept"]) for q in ext["rounds"] if not q["starved"]],
               root={"anchor_length": ext["anchor_length"], "anchor_start": ext["anchor_start"], "anchor_lcb": ext["anchor_lcb"]})
    return ref


def reference(case):
    """tests/recursion_ref.py on the case, from the root anchors that tests/seed_ref.py and tests/extend_ref.py give (once per process)"""
    return _reference(case["name"])


def trace_batches(ref):
    """what the trace must say per batch, in the order they run: (level, weight, gaps, N-way matches before the forward filter)"""
    return [(lv, w, len(recs), sum(len(r["matches"]) for r in recs)) for (lv, w), recs in ref["batches"].items()]


@functools.lru_cache(maxsize=None)
def _pair_reference(name):
    from tests import recursion_ref as R, seed_ref as S
    case = next(c for c in _all() if c["name"] == name)
    pair = [case["genomes"][1], case["genomes"][2]]
    root = S.find(pair, pattern_of(ROOT_W), S.MEM, 3, True, None)
    found = sorted(zip(root["length"], root["start"]), key=lambda m: m[1][0])
    assert [l for l, _ in found] == [BLOCK] * 3, found               # A, B and C
    ref = R.recurse(pair, found[:2], [0, 0], pattern_of, span_of, ROOT_W, case["params"]["min_recursive_gap"])
    ref["root"] = found
    return ref


def pair_reference(case):
    """a progressive entry: what tests/recursion_ref.py makes of the node over genomes {1, 2} -- the pairwise root search finds A, B
    and C; A and B are that node's chain (C belongs to the root node), and the gap between them recurses"""
    return _pair_reference(case["name"])
