"""Planted inputs for the progressive path (section 8 says what they cover).  Every case is a dict that names
the rule it aims at (`aim`); the expected results are assembled here from tests/progressive_ref.py, never from the oracle or the library.

Three families:
  refinement_sets()   genomes made of exact shared blocks with planted stretches between them: the root's anchors are exactly the blocks
                      (the planter checks it with tests/seed_ref.py, the CPU tests with the oracle's anchor table), so the root interval
                      is full columns per block and R.refine_interval per stretch
  walk_sets()         small genome sets whose interval table (genome set, left, right) the case writes out
  tree_sets(), bp_sets()   guide-tree and breakpoint-count inputs

seed_weight = 11 is passed explicitly everywhere; recursive = 0 wherever the planted intervals must stay as planted."""
import functools

import numpy as np

from tests import progressive_ref as R
from tests import scoring_schemes as SS
from tests import seed_ref as SR

P11 = 0b111011010110111            # getSeed(11, 0), span 15 (tests/test_progressive_cpu.py holds it to the table)
SPAN = 15
SOLID11 = (1 << 11) - 1            # eleven care positions in a row: one substitution ends a match
S, GO, GE = SS.HOXD70, SS.DEFAULT_GAPS[0], SS.DEFAULT_GAPS[1]
EMPTY = np.zeros(0, np.uint8)


def rnd(rng, n):
    return rng.integers(0, 4, int(n), dtype=np.uint8)


def cat(*parts):
    parts = [np.asarray(p, np.uint8) for p in parts]
    return np.concatenate(parts) if parts else EMPTY


def revcomp(s):
    return (3 - np.asarray(s, np.uint8))[::-1].copy()


def diverged(seq, phase, period=4):
    """a copy with every `period`-th base replaced: no window of the seed agrees with the original"""
    out = np.array(seq, np.uint8)
    out[phase::period] = (out[phase::period] + 1 + phase % 3) % 4
    return out


def periodic(unit, n):
    """a genome in which every mer occurs many times: it takes part in no seed hit (S3: MEM)"""
    unit = np.asarray(unit, np.uint8)
    return np.tile(unit, n // len(unit) + 1)[:n].copy()


def block(rng, n):
    """an exact shared block; it starts and ends with A, so a border rule can be stated against it"""
    b = rnd(rng, n)
    b[0] = b[-1] = 0
    return b


def tree_of(N, merges):
    left, right = [-1] * (2 * N - 1), [-1] * (2 * N - 1)
    for k, (a, b) in enumerate(merges):
        left[N + k], right[N + k] = a, b
    return np.array(left, np.int32), np.array(right, np.int32)


def balanced_tree(N):
    ids, merges, nxt = list(range(N)), [], N
    while len(ids) > 1:
        up = []
        for i in range(0, len(ids), 2):
            merges.append((ids[i], ids[i + 1]))
            up.append(nxt)
            nxt += 1
        ids = up
    return tree_of(N, merges)


def caterpillar_tree(N):
    return tree_of(N, [(0, 1)] + [(k, N + k - 2) for k in range(2, N)])


# =========================================================================================================== refinement sets
def border_ok(seqs):
    """at both borders of a stretch the adjacent bases do not all agree; an empty stretch counts as the neighbouring block's base (A)"""
    first = {int(s[0]) if len(s) else 0 for s in seqs}
    last = {int(s[-1]) if len(s) else 0 for s in seqs}
    return len(first) > 1 and len(last) > 1


def refined(seqs, rounds=9, wrong=None):
    return R.refine_interval(seqs, rounds, S, GO, GE, wrong)


def searched(n, slots, pred, seed0, lo=3, hi=10):
    """the first seeded random stretch (lengths lo .. hi in `slots`, empty elsewhere) with legal borders that `pred` accepts"""
    for seed in range(seed0, seed0 + 20000):
        rng = np.random.default_rng(seed)
        seqs = [rnd(rng, rng.integers(lo, hi + 1)) if g in slots else EMPTY for g in range(n)]
        if border_ok(seqs) and pred(seqs):
            return seqs
    raise AssertionError("no stretch from seed %d on" % seed0)


def wins(r):
    """the stretch whose rotation r is strictly the best of all its rotations"""
    def pred(seqs):
        obj = refined(seqs)[3]
        return len(obj) > r and all(obj[r] > o for q, o in enumerate(obj) if q != r)
    return pred


def tied(seqs):
    """two rotations with different columns share the highest objective"""
    nz = [s for s in seqs if len(s)]
    if len(nz) < 3:
        return False
    obj = refined(seqs)[3]
    best = [r for r, o in enumerate(obj) if o == max(obj)]
    return len(best) >= 2 and not np.array_equal(refined(seqs)[0], refined(seqs, wrong="ties_high")[0])


TIE_SEED = 122                     # the first seed of `searched(3, (0, 1, 2), tied, 0)`


def layout_stretch(seed, L, o, t):
    """three copies of one sequence, each with its own substitutions (phases 0, 2, 4 of period 6: no seed window agrees in all), and t
    bases inserted into the middle copy in front of its base o: the kept alignment is L + t columns, the pair (0, 1) one-sided at columns
    o .. o + t - 1, the pair (0, 2) in neither of them.  The case asserts the layout on the reference."""
    rng = np.random.default_rng(seed)
    X = rnd(rng, L)
    seqs = []
    for g in range(3):
        s = X.copy()
        s[2 * g::6] = (s[2 * g::6] + 1 + g) % 4
        seqs.append(s)
    seqs[2][-1] = (X[-1] + 2) % 4
    ins = rnd(rng, t)
    ins[0] = (seqs[1][o] + 2) % 4                  # the inserted run cannot slide: its ends differ from the bases it would swap with
    ins[-1] = (seqs[1][o - 1] + 2) % 4
    seqs[1] = cat(seqs[1][:o], ins, seqs[1][o:])
    return seqs


def layout_of(seqs, rounds):
    cols = refined(seqs, rounds)[0]
    return R.pair_layout(cols, 0, 1), R.pair_layout(cols, 0, 2)


# (name, seed, L, o, t, what the kept alignment holds for dp_sp_scores); the seed is the first from 900 + 20 i at which the reference shows
# the layout at 1, 2 and 9 rounds (o and o - 1 avoid the middle copy's own substitutions: there the inserted run could slide)
LAYOUTS = [
    ("cross_63_64", 905, 120, 60, 8, "128 columns; pair (0,1) one-sided over 60..67, pair (0,2) in neither at 63 and 64"),
    ("cross_127_128", 921, 141, 124, 8, "pair (0,1) one-sided over 124..131"),
    ("start_64", 940, 75, 64, 4, "a run that starts at column 64"),
    ("end_63", 963, 81, 58, 6, "a both-column at lane 0 (column 64) after a run that ended at lane 63"),
    ("cols_64", 982, 60, 30, 4, "64 columns"),
    ("cols_65", 1002, 61, 22, 4, "65 columns"),
]


def assemble(blocks, stretches, gids, rounds, wrong=None):
    """the interval of genomes `gids` made of the blocks and the stretches between them -> (columns, dp score, winners)"""
    full = sum(1 << g for g in gids)
    cols, score, winners = [], 0, []
    for i, b in enumerate(blocks):
        cols += [full] * len(b)
        if i == len(stretches):
            break
        seqs = stretches[i]
        if sum(1 for s in seqs if len(s)) >= 2:
            c, sc, win, obj = refined(seqs, rounds, wrong)
            cols += [sum(1 << gids[j] for j in range(len(gids)) if int(x) >> j & 1) for x in c]
            score += sc
            winners.append(win)
        else:
            for j, s in enumerate(seqs):
                cols += [1 << gids[j]] * len(s)
            winners.append(None)
    return cols, score, winners


def genomes_of(n, blocks, stretches):
    return [cat(blocks[0], *[x for i, st in enumerate(stretches) for x in (st[g], blocks[i + 1])]) for g in range(n)]


def _block_starts(n, blocks, stretches):
    """1-based start of every block in every genome"""
    out, at = [], [1] * n
    for i, b in enumerate(blocks):
        out.append(tuple(at))
        for g in range(n):
            at[g] += len(b) + (len(stretches[i][g]) if i < len(stretches) else 0)
    return out


def plant_refinement(name, n, seed, stretches, aim):
    """blocks from the first seed at which the root's matches are exactly the blocks (a window that reaches a few bases into a stretch can
    agree at the seed's don't-care positions; such a draw is passed over)"""
    assert all(border_ok(st) for st in stretches), name
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        blocks = [block(rng, 60 + int(rng.integers(0, 25))) for _ in range(len(stretches) + 1)]
        genomes = genomes_of(n, blocks, stretches)
        f = SR.find(genomes, P11, mode=SR.MEM, mask=(1 << n) - 1)
        want = {(len(b), st) for b, st in zip(blocks, _block_starts(n, blocks, stretches))}
        if SR.as_set(f) == want:
            break
    else:
        raise AssertionError("%s: the root's matches are not the blocks" % name)
    return {"name": name, "aim": aim, "n": n, "genomes": genomes, "blocks": blocks, "stretches": stretches, "tree": None,
            "anchors": sorted(want, key=lambda x: x[1][0]),
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0}}


def expect_refinement(case, rounds, wrong=None):
    """the one root interval of a refinement set"""
    n = case["n"]
    cols, score, winners = assemble(case["blocks"], case["stretches"], list(range(n)), rounds, wrong)
    return {"left": np.ones((1, n), np.int64), "right": np.array([[len(g) for g in case["genomes"]]], np.int64),
            "col_off": np.array([0, len(cols)], np.int64), "cols": np.array(cols, np.uint32), "dp_score": np.array([score], np.int64),
            "winners": winners}


@functools.lru_cache(maxsize=None)
def refinement_sets():
    sets = []
    # N = 3: the rotation winners, k < 3 neighbours, and the 64-column edges of the objective kernel
    st = [searched(3, (0, 1, 2), wins(0), 100), searched(3, (0, 1), lambda s: True, 110), searched(3, (0, 1, 2), wins(1), 120),
          searched(3, (2,), lambda s: True, 130), searched(3, (0, 1, 2), wins(2), 140), searched(3, (1, 2), lambda s: True, 150)]
    lay = [layout_stretch(seed, L, o, t) for nm, seed, L, o, t, what in LAYOUTS]
    if TIE_SEED is not None:
        st.append(searched(3, (0, 1, 2), tied, TIE_SEED))
    sets.append(plant_refinement("n3", 3, 31, st + lay, "winners 0, 1, 2 (2 only from two rounds on), k = 2 and k = 1 between them, rounds > k - 1, "
                                 "the lowest rotation on a tie, kept alignments of 64, 65 and 128 columns and one-sided runs on the 64-column edges"))
    sets[-1]["layouts"] = list(range(len(st), len(st) + len(lay)))
    sets[-1]["tie"] = len(st) - 1 if TIE_SEED is not None else None
    # N = 4
    st = [searched(4, (0, 1, 2, 3), wins(0), 200), searched(4, (1, 3), lambda s: True, 210), searched(4, (0, 1, 2, 3), wins(1), 220),
          searched(4, (0,), lambda s: True, 230), searched(4, (0, 1, 2, 3), wins(2), 240), searched(4, (0, 2, 3), wins(2), 250),
          searched(4, (0, 1, 2, 3), wins(3), 260)]
    sets.append(plant_refinement("n4", 4, 41, st, "winners 0 .. 3 among four sequences; an empty slot in front ((0,2,3): rotation slots are not node slots)"))
    # N = 5: non-empty slots {0, 2, 3} and {1, 2, 4}
    st = [searched(5, (0, 2, 3), wins(1), 300), searched(5, (1, 4), lambda s: True, 310), searched(5, (1, 2, 4), wins(2), 320),
          searched(5, (3,), lambda s: True, 330), searched(5, (0, 1, 2, 3, 4), wins(0), 340), searched(5, (0, 1, 2, 3, 4), wins(4), 350),
          searched(5, (1, 2, 4), wins(1), 360), searched(5, (0, 2, 3), wins(2), 370)]
    sets.append(plant_refinement("n5", 5, 51, st, "non-empty slots {0,2,3} and {1,2,4} of five: the map of a rotation's column bits back to the node's slots; "
                                 "rotation 4 wins only with rounds = 9"))
    return sets


ROUNDS = (1, 2, 9)


@functools.lru_cache(maxsize=None)
def clade_set():
    """a segment (blocks and stretches) that only genomes {2, 3, 4} carry, between two root blocks, longer than min_recursive_gap: the
    root is cut there, node {2, 3, 4} of the given tree aligns it -- gm = (2, 3, 4), the byte LUT of node_blocks, rotations' slots"""
    n = 5
    rng = np.random.default_rng(61)
    rst = [searched(5, (0, 1, 2, 3, 4), wins(1), 400), searched(5, (0, 2, 3), wins(2), 410)]
    cst = [searched(3, (0, 1, 2), wins(2), 420), searched(3, (0, 2), lambda s: True, 430), searched(3, (0, 1, 2), wins(1), 440)]
    rb = [block(rng, 70 + int(rng.integers(0, 20))) for _ in range(4)]          # root blocks: rb0 st0 rb1 | clade | rb2 st1 rb3
    cb = [block(rng, 70 + int(rng.integers(0, 20))) for _ in range(4)]
    cb[0][0], cb[-1][-1] = 1, 2                                                 # (the clade's outer ends differ from the root blocks' A)
    clade = [cat(cb[0], *[x for i, st in enumerate(cst) for x in (st[g], cb[i + 1])]) for g in range(3)]
    assert min(len(c) for c in clade) > 200
    genomes = [cat(rb[0], rst[0][g], rb[1], clade[g - 2] if g >= 2 else EMPTY, rb[2], rst[1][g], rb[3]) for g in range(n)]
    tree = tree_of(5, [(0, 1), (3, 4), (2, 6), (5, 7)])
    return {"name": "clade", "aim": "a node of genomes (2,3,4): non-identity gm, the LUT of node_blocks, the rotation-to-slot map", "n": n,
            "genomes": genomes, "tree": tree, "rb": rb, "cb": cb, "rst": rst, "cst": cst, "clade": clade,
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0}}


def expect_clade(case, rounds, wrong=None):
    n, rb, cb, rst, cst, genomes = 5, case["rb"], case["cb"], case["rst"], case["cst"], case["genomes"]
    a = assemble(rb[:2], rst[:1], list(range(5)), rounds, wrong)
    b = assemble(rb[2:], rst[1:], list(range(5)), rounds, wrong)
    c = assemble(cb, cst, [2, 3, 4], rounds, wrong)
    la = [len(rb[0]) + len(rst[0][g]) + len(rb[1]) for g in range(n)]
    lc = [len(case["clade"][g - 2]) if g >= 2 else 0 for g in range(n)]
    left = np.array([[1] * n, [la[g] + lc[g] + 1 for g in range(n)], [la[g] + 1 if g >= 2 else 0 for g in range(n)]], np.int64)
    right = np.array([la, [len(x) for x in genomes], [la[g] + lc[g] if g >= 2 else 0 for g in range(n)]], np.int64)
    cols = a[0] + b[0] + c[0]
    return {"left": left, "right": right, "col_off": np.array([0, len(a[0]), len(a[0]) + len(b[0]), len(cols)], np.int64),
            "cols": np.array(cols, np.uint32), "dp_score": np.array([a[1], b[1], c[1]], np.int64), "winners": a[2] + b[2] + c[2]}


# ================================================================================================================= walk sets
TREE3 = tree_of(3, [(0, 1), (2, 3)])


def row(gs, left, right):
    return (tuple(gs), tuple(left), tuple(right))


def placed_border(e, mirrored):
    """genomes 0 and 1 are identical; genome 2 shares only the part X of them.  Plain: X comes first and ends at base e, the child
    (0, 1) must start at e + 1 although its genomes agree across that border.  Mirrored: the child's part comes first and ends at e."""
    rng = np.random.default_rng(700 + e + 1000 * mirrored)
    Y = rnd(rng, 150)
    if not mirrored:
        X = rnd(rng, e)
        a = cat(X, Y)
        g2 = cat(X, [(Y[0] + 1) % 4], rnd(rng, 90))
        table = [row((0, 1, 2), (1, 1, 1), (e, e, e)), row((0, 1), (e + 1, e + 1), (len(a), len(a))), row((2,), (e + 1,), (len(g2),))]
        wrong = [row((0, 1, 2), (1, 1, 1), (e, e, e)), row((0, 1), (1, 1), (len(a), len(a))), row((2,), (e + 1,), (len(g2),))]
    else:
        X = rnd(rng, 110)
        Y = Y[:e]
        a = cat(Y, X)
        Z = rnd(rng, 90)
        Z[-1] = (Y[-1] + 1) % 4
        g2 = cat(Z, X)
        table = [row((0, 1, 2), (e + 1, e + 1, len(Z) + 1), (len(a), len(a), len(g2))), row((0, 1), (1, 1), (e, e)), row((2,), (1,), (len(Z),))]
        wrong = [table[0], row((0, 1), (1, 1), (len(a), len(a))), table[2]]
    return {"name": "placed_border_%s%d" % ("m" if mirrored else "", e), "genomes": [a, a.copy(), g2], "tree": TREE3,
            "aim": "extension at the child stops at a base the root placed; the border on a word edge of the placed-base bitmap",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0, "lcb_weight": 30}, "table": table,
            "wrong": {"no_border_stop": wrong}}


def four_identical():
    rng = np.random.default_rng(721)
    g = rnd(rng, 900)
    L = len(g)
    return {"name": "four_identical", "genomes": [g.copy() for _ in range(4)], "tree": None, "aim": "one interval; every child pool is empty",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0}, "table": [row((0, 1, 2, 3), (1,) * 4, (L,) * 4)], "wrong": {}}


def private_insert(n_free):
    """R1 and R2 are shared by all three, R2 inverted in genome 2: two root intervals.  Between them genome 1 (and with n_free = 2 genome 0
    too) carries `T`: free bases that no root interval takes.  Genome 2 has nothing left; with n_free = 1 genome 0 has nothing left either."""
    rng = np.random.default_rng(730 + n_free)
    R1, R2, T = rnd(rng, 120), rnd(rng, 120), rnd(rng, 100)
    R1[-1] = R2[0] = R2[-1] = 0                        # (genome 2 goes on with T behind R1: the complement of R2's last base)
    T[0], T[-1] = 1, 2
    g0 = cat(R1, T if n_free == 2 else EMPTY, R2)
    g1 = cat(R1, T, R2)
    g2 = cat(R1, revcomp(R2))
    if n_free == 2:
        T1 = diverged(T, 1)
        g1 = cat(R1, T1, R2)
    a = len(R1)
    o0, o1 = len(g0) - 120, len(g1) - 120
    table = [row((0, 1, 2), (1, 1, 1), (a, a, a)), row((0, 1, 2), (o0 + 1, o1 + 1, a + 1), (len(g0), len(g1), len(g2)))]
    if n_free == 2:
        table.append(row((0,), (a + 1,), (o0,)))
    table.append(row((1,), (a + 1,), (o1,)))
    return {"name": "private_insert_%d" % n_free, "genomes": [g0, g1, g2], "tree": TREE3,
            "aim": "a node where one genome has nothing left and its sister has a private insert" if n_free == 1 else
                   "a node whose two genomes have unrelated free stretches: leftovers in genome and position order",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0}, "table": table, "wrong": {}}


def short_free(n):
    """as private_insert, with the same n free bases in genomes 0 and 1: n = span - 1 holds no window and stays a leftover; n = span is one
    match, and with lcb_weight = 15 (10 for two of three genomes) the child places it"""
    rng = np.random.default_rng(740 + n)
    R1, R2, T = rnd(rng, 120), rnd(rng, 120), rnd(rng, n)
    R1[-1] = R2[0] = R2[-1] = 0
    T[0], T[-1] = 1, 2
    g0 = cat(R1, T, R2)
    g2 = cat(R1, revcomp(R2))
    a = len(R1)
    table = [row((0, 1, 2), (1, 1, 1), (a, a, a)), row((0, 1, 2), (a + n + 1, a + n + 1, a + 1), (len(g0), len(g0), len(g2)))]
    placed = table + [row((0, 1), (a + 1, a + 1), (a + n, a + n))]
    left = table + [row((0,), (a + 1,), (a + n,)), row((1,), (a + 1,), (a + n,))]
    return {"name": "short_free_%d" % n, "genomes": [g0, g0.copy(), g2], "tree": TREE3,
            "aim": "a free stretch of span - 1 bases between two placed blocks stays a leftover; span bases are found",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0, "lcb_weight": 15}, "table": left if n < SPAN else placed,
            "wrong": {"window_fits": placed if n < SPAN else left}}


def chain_cut():
    """root blocks R1, R2, R3 with segments S1, S2 that only genomes 0 and 1 have between them (longer than min_recursive_gap = 50: the
    root is cut there).  Node (0, 1) finds S1 and S2 as one collinear chain and must cut it at the placed R2: two intervals"""
    rng = np.random.default_rng(750)
    R1, R2, R3, S1, S2 = rnd(rng, 110), rnd(rng, 110), rnd(rng, 110), rnd(rng, 80), rnd(rng, 80)
    S1[0], S1[-1], S2[0], S2[-1] = (R2[0] + 1) % 4, (R1[-1] + 1) % 4, (R3[0] + 1) % 4, (R2[-1] + 1) % 4
    g0 = cat(R1, S1, R2, S2, R3)
    g2 = cat(R1, R2, R3)
    table = [row((0, 1, 2), (1, 1, 1), (110, 110, 110)), row((0, 1, 2), (191, 191, 111), (300, 300, 220)), row((0, 1, 2), (381, 381, 221), (490, 490, 330)),
             row((0, 1), (111, 111), (190, 190)), row((0, 1), (301, 301), (380, 380))]
    uncut = table[:3] + [row((0, 1), (111, 111), (380, 380))]
    return {"name": "chain_cut", "genomes": [g0, g0.copy(), g2], "tree": TREE3, "aim": "the cut of a chain at a placed block (node_pieces)",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0, "min_recursive_gap": 50}, "table": table, "wrong": {"no_chain_cut": uncut}}


def split_gap(n):
    """S1 of n bases in genomes 0 and 1 only, between root blocks; min_recursive_gap = 50.  n = 50 is aligned at the root (one interval),
    n = 51 is left to node (0, 1)"""
    rng = np.random.default_rng(760)
    R1, R2, S1 = rnd(rng, 110), rnd(rng, 110), rnd(rng, n)
    S1[0], S1[-1] = (R2[0] + 1) % 4, (R1[-1] + 1) % 4
    g0 = cat(R1, S1, R2)
    g2 = cat(R1, R2)

    def table(wrong=None):
        if R.cut_after_stretch([n, n, 0], 50, 10000, wrong):
            return [row((0, 1, 2), (1, 1, 1), (110, 110, 110)), row((0, 1, 2), (111 + n, 111 + n, 111), (220 + n, 220 + n, 220)),
                    row((0, 1), (111, 111), (110 + n, 110 + n))]
        return [row((0, 1, 2), (1, 1, 1), (220 + n, 220 + n, 220))]
    return {"name": "split_gap_%d" % n, "genomes": [g0, g0.copy(), g2], "tree": TREE3,
            "aim": "node_split_long: > min_recursive_gap in at least two but not all genomes",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0, "min_recursive_gap": 50}, "table": table(), "root_anchors": [110, 110],
            "wrong": {"gap_ge": table("gap_ge")} if n == 50 else {}}


def split_len(n):
    """a stretch all three genomes share (diverged copies: no seed window agrees), the longest side n bases, max_gapped_len = 120: n = 120
    is aligned inside the one root interval, n = 121 is cut and, unanchored in the subtree too, ends as leftovers"""
    rng = np.random.default_rng(770)
    R1, R2, T = rnd(rng, 110), rnd(rng, 110), rnd(rng, n)
    T[0], T[-1] = (R2[0] + 1) % 4, (R1[-1] + 1) % 4
    ts = [T, diverged(T, 1)[:n - 3], diverged(T, 2)[:n - 5]]
    for g in (1, 2):
        ts[g][0], ts[g][-1] = (T[0] + g) % 4, (T[-1] + g) % 4
    gs = [cat(R1, t, R2) for t in ts]

    def table(wrong=None):
        ln = [len(t) for t in ts]
        if R.cut_after_stretch(ln, 200, 120, wrong):
            return [row((0, 1, 2), (1, 1, 1), (110, 110, 110)), row((0, 1, 2), [111 + x for x in ln], [220 + x for x in ln])] + \
                   [row((g,), (111,), (110 + ln[g],)) for g in range(3)]
        return [row((0, 1, 2), (1, 1, 1), [220 + x for x in ln])]
    return {"name": "split_len_%d" % n, "genomes": gs, "tree": TREE3, "aim": "node_split_long: the longest side > max_gapped_len",
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0, "max_gapped_len": 120}, "table": table(), "root_anchors": [110, 110],
            "wrong": {"len_ge": table("len_ge")} if n == 120 else {}}


def thirty_two(shape):
    """32 genomes of about 1.5 kb: R1 (all), C (genomes 16..31 only, each with two substituted bases of its own: two-base stretches
    of sixteen sequences), R2 (all), D (shared by genomes 2i and 2i + 1), R3 (all).  Bit 31, and along the balanced tree a node of genomes 16..31"""
    rng = np.random.default_rng(780)
    R1, R2, R3, C = rnd(rng, 250), rnd(rng, 250), rnd(rng, 250), rnd(rng, 330)
    gs = []
    D = None
    for g in range(32):
        if g % 2 == 0:
            D = rnd(rng, 300)
        c = EMPTY
        if g >= 16:
            c = C.copy()
            at = 20 + 18 * (g - 16)                                      # (two bases: one could sit on a don't-care position of every window)
            c[at:at + 2] = (c[at:at + 2] + 1) % 4
        gs.append(cat(R1, c, R2, D, R3))
    return {"name": "thirty_two_" + shape, "genomes": gs, "tree": balanced_tree(32) if shape == "balanced" else caterpillar_tree(32),
            "aim": "32 genomes through the walk: bit 31, a 16-genome node of genomes 16..31", "table": None, "wrong": {},
            "params": {"seed_weight": 11, "recursive": 0, "lcb_scoring": 0, "refine_rounds": 2}}


@functools.lru_cache(maxsize=None)
def walk_sets():
    out = [placed_border(e, False) for e in (63, 64, 65, 127, 128)] + [placed_border(e, True) for e in (63, 64, 65, 127, 128)]
    out += [four_identical(), private_insert(1), private_insert(2), short_free(SPAN - 1), short_free(SPAN), chain_cut()]
    out += [split_gap(50), split_gap(51), split_len(120), split_len(121), thirty_two("balanced"), thirty_two("caterpillar")]
    return out


# ==================================================================================================== guide tree, breakpoints
def mutated(rng, seq, rate):
    out = np.array(seq, np.uint8)
    hit = rng.random(len(out)) < rate
    out[hit] = (out[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    return out


def block_genome(blocks, order, sep, length=0, filler=None):
    """blocks in `order` (i: block i; ~i: its reverse complement), each behind one separator base; padded to `length` with `filler`, a
    periodic run that takes part in no seed hit"""
    parts = []
    for i in order:
        parts += [[sep], revcomp(blocks[~i]) if i < 0 else blocks[i]]
    g = cat(*parts, [sep])
    if length:
        assert len(g) <= length, (len(g), length)
        g = cat(g, periodic(filler, length - len(g) + 40)[:length - len(g)])
    return g


@functools.lru_cache(maxsize=None)
def tree_sets():
    out = []
    rng = np.random.default_rng(800)
    g = rnd(rng, 1500)
    out.append({"name": "identical4", "genomes": [g.copy() for _ in range(4)], "pattern": P11, "aim": "all distances 0: merges (0,1), (2,3), (4,5)",
                "merges": [(0, 1), (2, 3), (4, 5)], "moved_by": ["ties_high"]})
    a = rnd(rng, 2000)
    out.append({"name": "unrelated", "genomes": [a, mutated(rng, a, 0.08), periodic([0, 1, 1, 2, 3, 3, 0], 2000), periodic([0, 2, 1, 3, 3, 1, 2, 2, 0], 2000)],
                "pattern": P11, "aim": "distances of exactly 10^6 and the ties among them", "merges": [(0, 1), (2, 3), (4, 5)], "moved_by": ["ties_high"]})
    # five genomes of 3000 bases; blocks of 40 under the solid seed: sim(0,1) = 20 blocks, (0,2) = 1, (1,2) = 3, (2,3) = 2.  After (0,1) -> 5:
    # d(5,2) = (986667 + 960000) / 2 = 973333.5 -> 973333 < d(2,3) = 973334: (2,5) merges next; a rounded mean ties with (2,3), which then wins
    bl = [rnd(rng, 40) for _ in range(26)]
    fill = [[0, 1, 2, 3, 1], [1, 3, 0, 2, 2], [2, 0, 3, 1, 1, 0], [3, 1, 0, 0, 2, 1], [0, 0, 1, 3, 2, 2, 1]]
    orders = [list(range(20)) + [20], list(range(20)) + [21, 22, 23], [20, 21, 22, 23, 24, 25], [24, 25], []]
    out.append({"name": "fractions5", "genomes": [block_genome(bl, orders[g], g % 4, 3000, fill[g]) for g in range(5)], "pattern": SOLID11,
                "aim": "size-weighted means that are not integers: the floor", "merges": [(0, 1), (2, 5), (3, 6), (4, 7)], "moved_by": ["round"],
                "dist": {(0, 1): 1000000 - 266666, (0, 2): 986667, (1, 2): 960000, (2, 3): 973334, (0, 3): 1000000, (3, 4): 1000000}})
    a = rnd(rng, 2000)
    big = cat(rnd(rng, 9000), mutated(rng, a, 0.03), rnd(rng, 9000))
    out.append({"name": "lengths_2k_20k", "genomes": [a, big, mutated(rng, big, 0.2)], "pattern": P11, "aim": "min(L_i, L_j) with lengths of 2 kb against 20 kb",
                "merges": None, "moved_by": ["longer"]})
    out.append({"name": "two", "genomes": [a, mutated(rng, a, 0.05)], "pattern": P11, "aim": "N = 2: one merge", "merges": [(0, 1)], "moved_by": []})
    anc = rnd(rng, 600)
    gs = [mutated(rng, anc, 0.002 * (g % 8)) for g in range(28)]
    gs += [gs[26].copy(), gs[27].copy(), gs[0].copy(), periodic([0, 1, 2, 2, 3, 1, 0, 3], 600)]
    out.append({"name": "thirty_two", "genomes": gs, "pattern": P11, "aim": "32 genomes: 1024 pair counters, pair ids up to 1023; identical genomes tie at 0",
                "merges": None, "moved_by": ["ties_high"]})
    return out


def bp_pair(K, order_b, seed, blen=40, lens=None, pad=(0, 0)):
    rng = np.random.default_rng(seed)
    bl = [rnd(rng, (lens or {}).get(i, blen)) for i in range(K)]
    a = block_genome(bl, list(range(K)), 0, pad[0], [0, 1, 2, 3, 1])
    b = block_genome(bl, order_b, 1, pad[1], [1, 3, 0, 2, 2])
    return [a, b]


@functools.lru_cache(maxsize=None)
def bp_sets():
    """-> cases with genomes, pattern, and `runs`: (min_len, {pair: count} or None where only the reference speaks)"""
    K = 12
    ident = list(range(K))
    out = []

    def add(name, genomes, runs, aim, moved_by, pattern=SOLID11, **kw):
        out.append(dict(name=name, genomes=genomes, runs=runs, aim=aim, moved_by=moved_by, pattern=pattern, **kw))
    add("identity", bp_pair(K, ident, 810), [(22, {(0, 1): 0})], "no breakpoint", ["steps_swapped"])
    add("inversion_middle", bp_pair(K, ident[:4] + [~i for i in range(7, 3, -1)] + ident[8:], 811), [(22, {(0, 1): 2})], "one inversion: 2", ["steps_swapped"])
    add("inversion_start", bp_pair(K, [~i for i in range(3, -1, -1)] + ident[4:], 812), [(22, {(0, 1): 1})], "an inversion at the very start: 1", ["steps_swapped"])
    add("inversion_end", bp_pair(K, ident[:8] + [~i for i in range(11, 7, -1)], 813), [(22, {(0, 1): 1})], "an inversion at the very end: 1", ["steps_swapped"])
    add("moved_block", bp_pair(K, [0, 1, 3, 4, 5, 6, 7, 2, 8, 9, 10, 11], 814), [(22, {(0, 1): 3})], "a moved block: 3", ["steps_swapped"])
    g = bp_pair(K, ident, 815)
    add("whole_reverse", [g[0], revcomp(g[1])], [(22, {(0, 1): 0})], "genome b reverse-complemented: rank steps of -1, count 0", ["steps_swapped"],
        all_reverse=True)
    for k in (255, 256, 257):
        rng = np.random.default_rng(820 + k)
        bl = [rnd(rng, 40) for _ in range(k)]
        gs = [block_genome(bl, list(range(k)), 0), block_genome(bl, list(range(k)), 1),
              block_genome(bl, [0, 1, 2, 3, ~4, 5, 6, 7, 8, 9], 2)]     # (one block: the complement of this separator is genome 1's)
        add("boundary_%d" % k, gs, [(22, {(0, 1): 0, (0, 2): 2, (1, 2): 2})], "pair (0,1) holds exactly %d counted records: the pair boundary at %d|%d" % (k, k - 1, k),
            ["pair_boundary"], counted={(0, 1): k, (0, 2): 10, (1, 2): 10})
    # a short reverse match between two collinear ones
    add("floor", bp_pair(5, [0, 1, ~2, 3, 4], 830, lens={2: 30}), [(30, {(0, 1): 2}), (31, {(0, 1): 0})],
        "min_len equal to a match length, and one above it", ["floor_strict"])
    # matches of 40, 50 (reverse) and 60 bases
    g = bp_pair(3, [0, ~1, 2], 831, lens={0: 40, 1: 50, 2: 60})
    add("few_records", g, [(61, {(0, 1): 0}), (60, {(0, 1): 0}), (50, {(0, 1): 1}), (40, {(0, 1): 2})], "floors that leave 0, 1, 2 and 3 records", ["floor_strict"],
        counted_by_floor={61: 0, 60: 1, 50: 2, 40: 3})
    for L in (4095, 4096):
        order = list(range(91)) + [~i for i in range(98, 90, -1)]
        add("key_width_%d" % L, bp_pair(99, order, 840, pad=(L, 4070)), [(22, {(0, 1): 1})],
            "the longest genome %d bases: keys of %d bits; the inversion lies past position 4000" % (L, 16 if L == 4095 else 17), ["steps_swapped"], past=4000)
    return out


def dup_pair(seed):
    """a small pair with duplicated, mutated segments (the seeded sweep of S11c's tie rules)"""
    rng = np.random.default_rng(seed)
    a = rnd(rng, 500)
    parts = [mutated(rng, a, 0.03)]
    for _ in range(3):
        lo = int(rng.integers(0, 400))
        seg = a[lo:lo + int(rng.integers(40, 100))]
        parts.append(mutated(rng, seg if rng.random() < 0.5 else revcomp(seg), 0.05))
    b = cat(*parts)
    return [a, b]


DUP_SEED = 8                       # the first seed at which two counted records (min_len 22) start at the same base of genome 0


def same_start_in_a(genomes, min_len=0):
    rec = R.bp_sorted(R.pair_records(genomes, P11), 0, 1, min_len)
    return any(x[0] == y[0] for x, y in zip(rec, rec[1:]))
