"""Planted genomes for the repeat map, a few thousand bases each, shared by tests/test_repeat_cpu.py (liveness: the
reference yields the record a case is aimed at) and tests/test_gpu_repeat_map.py (the device equals the reference).  A builder takes
the seed pattern and returns a Case, or None where the plant cannot exist for that pattern (said at the builder)."""
import itertools

import numpy as np

from tests import repeat_map_ref as RM

EDGES = (0, 1, 62, 63, 64, 65, 127, 128, 129)


class Case:
    def __init__(self, name, codes, aim, contig_starts=None, invalid=None, min_multi=2, max_multi=32):
        self.name, self.codes, self.aim = name, np.asarray(codes, np.uint8), aim
        self.contig_starts, self.invalid, self.min_multi, self.max_multi = contig_starts, invalid, min_multi, max_multi

    def reference(self, pattern):
        return RM.repeat_matches(self.codes, pattern, self.min_multi, self.max_multi, self.contig_starts, self.invalid)


def _seed_of(name, pattern):
    return [sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (1 << 31), int(pattern) % (1 << 31)]


def bg(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def assemble(parts):
    """parts: arrays; -> genome and the start of every part"""
    pos, at = [], 0
    for p in parts:
        pos.append(at); at += len(p)
    return np.concatenate(parts).astype(np.uint8), pos


def direct_flanks(g, copies, span):
    """copies: (start, length) of direct copies of one element.  The span - 1 bases in front of and behind copy i are set so that they
    differ from copy to copy: a window that reaches outside the element has a care position there (the first and the last are), so no
    offset outside the element agrees"""
    r = np.random.default_rng(span).integers(0, 4, (2, span))      # (random, so that the flanks are no repeats themselves)
    for i, (s, L) in enumerate(copies):
        for d in range(1, span):
            if s - d >= 0:
                g[s - d] = (r[0, d] + i) & 3
            if s + L - 1 + d < len(g):
                g[s + L - 1 + d] = (r[1, d] + i) & 3


def has(records, length, starts):
    return (length, tuple(starts)) in records


# ---- walk rounds: a direct pair whose emitting hit has k_lo and k_hi of its own -------------------------------------------------
def walk(pattern, klo, khi):
    """copies of E at a and b; with klo > 0 a third copy of E's first span - 1 + klo bases makes the first klo windows 3-fold, so the
    pair's lowest hit sits at window klo and walks klo offsets left and khi right: one 2-fold record of the whole of E"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("walk%d_%d" % (klo, khi), pattern))
    T = span - 1 + klo if klo else 0
    L = khi + span + klo
    E = bg(rng, L)
    parts = [bg(rng, 40), E, bg(rng, 45), E, bg(rng, 50)] + ([E[:T], bg(rng, 40)] if T else [])
    g, pos = assemble(parts)
    a, b = pos[1], pos[3]
    direct_flanks(g, [(a, L), (b, L)] + ([(pos[5], T)] if T else []), span)
    for d in range(span - 1):                               # the third copy does not run on like E
        if T and T + d < L:
            g[pos[5] + T + d] = (int(E[T + d]) + 2) & 3
    aims = [(L, (a + 1, b + 1))] + ([(T, (a + 1, b + 1, pos[5] + 1))] if T else [])

    def aim(rec):
        for ln, st in aims:
            assert has(rec, ln, st), (ln, st, rec)
    return Case("walk-%d-%d" % (klo, khi), g, aim)


# ---- chaining -------------------------------------------------------------------------------------------------------------------
def _killed_runs(pattern, subs, lo, hi):
    care, span = RM.care_offsets(pattern)
    care = set(care)
    killed = [any((x - p) in care for x in subs) for p in range(lo, hi)]
    runs, n = [], 0
    for k in killed + [False]:
        if k:
            n += 1
        elif n:
            runs.append(n); n = 0
    return runs


def _subs_for_gap(pattern, gap):
    """substitution positions (relative, up to three inside two spans) after which the longest run of disagreeing offsets is exactly
    gap - 1, i.e. two agreeing offsets exactly `gap` apart with none between; None when no such set exists for the pattern (a solid
    seed: every substitution kills exactly span windows in a row, so gap = span cannot be planted)"""
    span = RM.care_offsets(pattern)[1]
    for n in (1, 2, 3):
        for subs in itertools.combinations(range(span, 2 * span + 2), n):
            if max(_killed_runs(pattern, subs, 0, 4 * span)) == gap - 1:
                return subs
    return None


def chain(pattern, kind):
    """kind 'span': substitutions in the second copy leave agreeing offsets exactly span apart -- one record; 'span+1': exactly
    span + 1 apart -- two records of one diagonal; 'dontcare': one substitution, which breaks nothing when the longest run of offsets
    it kills is below span (any seed with a don't-care position; a solid seed has none: no case)"""
    span = RM.care_offsets(pattern)[1]
    if kind == "dontcare":
        if max(_killed_runs(pattern, (2 * span,), 0, 4 * span)) >= span:
            return None
        subs = (2 * span,)
    else:
        subs = _subs_for_gap(pattern, span if kind == "span" else span + 1)
        if subs is None:
            return None
    rng = np.random.default_rng(_seed_of("chain" + kind, pattern))
    L = 5 * span
    E = bg(rng, L)
    E2 = E.copy()
    for x in subs:
        E2[x] = (E2[x] + 1) & 3
    g, pos = assemble([bg(rng, 40), E, bg(rng, 45), E2, bg(rng, 50)])
    a, b = pos[1], pos[3]
    direct_flanks(g, [(a, L), (b, L)], span)

    def aim(rec):
        diag = [r for r in rec if len(r[1]) == 2 and r[1][1] - r[1][0] == b - a and r[1][0] > 0 and r[1][1] > 0]
        if kind == "span+1":
            assert len(diag) == 2 and diag[0][1][0] == a + 1 and diag[1][1][0] + diag[1][0] == a + 1 + L, diag
        else:
            assert diag == [(L, (a + 1, b + 1))], diag
    return Case("chain-" + kind, g, aim)


# ---- the order rule: inverted pairs ----------------------------------------------------------------------------------------------
def inverted(pattern, spacer, L):
    """X, `spacer` bases, the reverse complement of X.  The windows of the two arms walk towards each other; S20 stops them while the
    forward window still starts in front of the reverse one.  spacer 0 is a perfect palindrome: every offset agrees up to that point,
    so the arms run on for (d - 1) >> 1 offsets, d = 2 L - span the distance of the outermost windows"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("inv%d_%d" % (spacer, L), pattern))
    X = bg(rng, L)
    S = bg(rng, spacer)
    g, pos = assemble([bg(rng, 40), X, S, rc(X), bg(rng, 40)])
    a, b = pos[1], pos[3]
    g[a - 1] = 0; g[b + L] = 0                              # the bases outside the arms do not pair (A with A)
    if spacer >= 2:
        g[a + L] = 0; g[b - 1] = 0                          # nor the first bases of the spacer (A pairs with T)

    def aim(rec):
        r = [x for x in rec if len(x[1]) == 2 and x[1][0] == a + 1 and x[1][1] < 0]
        assert len(r) == 1, rec
        ln, (s0, s1) = r[0]
        assert ln >= L and -s1 + ln - 1 == b + L, r                            # the reverse arm ends with the last base of rc(X)
        assert (s0 - 1) + (ln - span) < (-s1 - 1), r                            # the last forward window starts in front of its partner: never crossed
        if spacer == 0:
            assert ln == ((2 * L - span - 1) >> 1) + span, r                    # the arms stop where the windows would meet, span - 1 bases past the centre
            assert (s0 - 1) + (ln - span) + 2 >= (-s1 - 1), r                   # ... and no earlier: the outermost pair is one or two windows apart
        if spacer >= span:
            assert ln == L, r
    return Case("inverted-%d-%d" % (spacer, L), g, aim)


# ---- even weight: a mer that is its own reverse complement ------------------------------------------------------------------------
def selfcomp(pattern, arrangement):
    """a window W whose masked mer is its own reverse complement (even weight only: at odd weight the centre is a care position and no
    base is its own complement -> no case), planted in the middle of X; X then stands twice, as an inverted or a direct pair.  W's
    family has both flags 0: a forward hit with a cluster of its own; the pair's diagonal passes it and is emitted once"""
    care, span = RM.care_offsets(pattern)
    if len(care) % 2:
        return None
    rng = np.random.default_rng(_seed_of("selfcomp" + arrangement, pattern))
    W = bg(rng, span)
    for t in care:
        if t < span - 1 - t:
            W[span - 1 - t] = 3 - W[t]
    L = 4 * span + 1
    X = bg(rng, L)
    o = (L - span) // 2
    X[o:o + span] = W
    second = rc(X) if arrangement == "inverted" else X
    g, pos = assemble([bg(rng, 40), X, bg(rng, 2 * span + 3), second, bg(rng, 40)])
    a, b = pos[1], pos[3]
    g[a - 1] = 0; g[b - 1] = 1; g[a + L] = 0; g[b + L] = 1 if arrangement == "direct" else 2
    wb = b + (L - span - o if arrangement == "inverted" else o)           # where W stands in the second copy

    def aim(rec):
        if arrangement == "inverted":
            assert has(rec, L, (a + 1, -(b + 1))), rec                            # the reverse diagonal, once, through W
            own = [r for r in rec if r[1][:2] == (a + o + 1, wb + 1) and len(r[1]) == 2]
            assert len(own) == 1 and own[0][0] >= span, rec                       # W's family: forward, its own cluster
        else:
            assert has(rec, L, (a + 1, b + 1)), rec                               # direct: W is a hit of the diagonal like its neighbours
            assert len([r for r in rec if len(r[1]) == 2 and r[1][1] - r[1][0] == b - a and r[1][1] > 0]) == 1, rec
    return Case("selfcomp-" + arrangement, g, aim)


# ---- nesting: three copies of a core, two of which run on ---------------------------------------------------------------------------
def nesting(pattern, side, strands, min_multi=2, max_multi=32):
    """copies 1 and 2 hold ext + core (+ ext), copy 3 the core alone: one 3-fold record of the core and one 2-fold record of the long
    copies that runs through it.  strands: orientation of the three copies, e.g. 'FRF'; 'R' first makes component 0 the reverse copy"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("nest" + side + strands, pattern))
    K = bg(rng, 3 * span + 2)
    Le = bg(rng, 2 * span + 1) if side in ("left", "both") else bg(rng, 0)
    Re = bg(rng, 2 * span + 4) if side in ("right", "both") else bg(rng, 0)
    E = np.concatenate([Le, K, Re]).astype(np.uint8)
    cp = [E, E, K]
    parts = [bg(rng, 40)]
    for c, s in zip(cp, strands):
        parts += [rc(c) if s == "R" else c, bg(rng, 2 * span + 7)]
    g, pos = assemble(parts)
    st = [pos[1], pos[3], pos[5]]
    for i, (c, s) in enumerate(zip(cp, strands)):           # the bases around every copy, read along the diagonal, differ from the others'
        lo, hi = st[i] - 1, st[i] + len(c)
        before, after = (hi, lo) if s == "R" else (lo, hi)
        vb, va = i, (i + 1) & 3
        if i == 2 and len(Le):
            vb = (int(Le[-1]) + 1) & 3                      # (the core alone: unlike what precedes / follows the core in the long copies)
        if i == 2 and len(Re):
            va = (int(Re[0]) + 1) & 3
        g[before] = (3 - vb) if s == "R" else vb
        g[after] = (3 - va) if s == "R" else va
    rel = [s != strands[0] for s in strands]
    # core of copy i, as a signed start
    def core_start(i):
        off = len(Re) if strands[i] == "R" else len(Le)
        if i == 2:
            off = 0
        return st[i] + off + 1
    want3 = (len(K), tuple(-core_start(i) if rel[i] else core_start(i) for i in range(3)))
    want2 = (len(E), tuple(-(st[i] + 1) if rel[i] else st[i] + 1 for i in range(2)))

    def aim(rec):
        assert (want3 in rec) == (min_multi <= 3 <= max_multi), (want3, rec)
        assert (want2 in rec) == (min_multi <= 2 <= max_multi), (want2, rec)
        assert all(min_multi <= len(r[1]) <= max_multi for r in rec), rec
    return Case("nesting-%s-%s-%d-%d" % (side, strands, min_multi, max_multi), g, aim, min_multi=min_multi, max_multi=max_multi)


# ---- multiplicity limits --------------------------------------------------------------------------------------------------------------
def copies(pattern, n):
    """n copies of a unit of span + 10 bases between random spacers, and two copies of a long element A + unit + B: with n + 2 = 32 the
    unit's families are emitted, 32-fold; with 33 they are not, and the 2-fold record of the long element runs through them unharmed"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("copies%d" % n, pattern))
    U = bg(rng, span + 10)
    A, B = bg(rng, 2 * span), bg(rng, 2 * span + 3)
    E = np.concatenate([A, U, B]).astype(np.uint8)
    parts, units = [bg(rng, 30), E, bg(rng, 33), E, bg(rng, 31)], []
    for i in range(n):
        units.append(len(parts)); parts += [U, bg(rng, 25 + i % 7)]
    g, pos = assemble(parts)
    a, b = pos[1], pos[3]
    g[a - 1] = 0; g[b - 1] = 1; g[a + len(E)] = 0; g[b + len(E)] = 1
    for j, ui in enumerate(units):                          # a unit copy continues neither like the long element nor like its neighbours
        u = pos[ui]
        g[u - 1] = (int(A[-1]) + 1 + j % 3) & 3; g[u + len(U)] = (int(B[0]) + 1 + (j + 1) % 3) & 3
    m = n + 2

    def aim(rec):
        assert has(rec, len(E), (a + 1, b + 1)), rec
        assert all(len(r[1]) <= 32 for r in rec)
        big = [r for r in rec if len(r[1]) == m]
        assert (len(big) >= 1) == (m <= 32), (m, [len(r[1]) for r in rec])
        if m <= 32:
            assert any(r[0] >= len(U) and r[1][0] == a + len(A) + 1 for r in big), big
    return Case("copies-%d" % m, g, aim)


def homopolymer(pattern):
    """a run of 400 A: one family of 400 - span + 1 windows (and its reverse complement's none), above 255 -- the size table saturates;
    a direct pair beside it is found as usual and nothing of the run is emitted"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("homopolymer", pattern))
    E = bg(rng, 3 * span)
    g, pos = assemble([bg(rng, 40), E, bg(rng, 30), np.zeros(400, np.uint8), bg(rng, 30), E, bg(rng, 40)])
    a, b = pos[1], pos[5]
    g[a - 1] = 0; g[b - 1] = 1; g[a + len(E)] = 2; g[b + len(E)] = 1; g[pos[3] - 1] = 1; g[pos[3] + 400] = 2

    def aim(rec):
        fam = RM.families(g, pattern)[0]
        assert max(len(v) for v in fam.values()) > 255
        assert has(rec, len(E), (a + 1, b + 1)), rec
        assert not any(pos[3] <= abs(s) - 1 < pos[3] + 400 - span for r in rec for s in r[1]), rec
    return Case("homopolymer", g, aim)


# ---- tandem arrays ----------------------------------------------------------------------------------------------------------------------
def tandem(pattern, period, ncopy):
    """`ncopy` copies of a unit of `period` bases in a row: the components of a family lie `period` apart and overlap each other"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("tandem%d_%d" % (period, ncopy), pattern))
    while True:
        U = bg(rng, period)
        if len(set(U.tolist())) > 1:
            break
    g, pos = assemble([bg(rng, 50), np.tile(U, ncopy), bg(rng, 50)])
    g[pos[1] - 1] = (int(U[-1]) + 1) & 3; g[pos[2]] = (int(U[0]) + 1) & 3      # the array does not run on
    nwin = period * ncopy - span + 1                        # windows inside the array

    def aim(rec):
        if nwin < 2 * period:
            return                                           # fewer than two windows per mer: no family inside the array
        ov = [r for r in rec if len(r[1]) >= 2 and pos[1] < r[1][0] <= pos[1] + period + 1 and all(0 < y - x < r[0] for x, y in zip(r[1], r[1][1:]))]
        assert ov and all(y - x == period for r in ov for x, y in zip(r[1], r[1][1:])), rec
    return Case("tandem-%d-%d" % (period, ncopy), g, aim)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
def flush(pattern):
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("flush", pattern))
    E = bg(rng, 3 * span + 1)
    g, pos = assemble([E, bg(rng, 2 * span + 5), E])
    g[len(E)] = (int(g[-len(E) - 1]) + 1) & 3

    def aim(rec):
        assert has(rec, len(E), (1, pos[2] + 1)), rec
    return Case("flush", g, aim)


def contig_cut(pattern):
    """the second copy is cut by a contig join h bases in: the span - 1 windows across the join are invalid, and the valid windows either
    side of it abut -- agreeing offsets exactly span apart -- so the record runs through (S3: matches abut across a collinear join;
    here they chain, as in S4); without the table the same windows are hits"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("contig", pattern))
    L, h = 5 * span, 2 * span + 3
    E = bg(rng, L)
    g, pos = assemble([bg(rng, 40), E, bg(rng, 45), E, bg(rng, 40)])
    a, b = pos[1], pos[3]
    direct_flanks(g, [(a, L), (b, L)], span)

    def aim(rec):
        assert has(rec, L, (a + 1, b + 1)), rec
        ok = RM.window_valid(len(g), span, [0, b + h])
        assert ok.count(False) == span - 1 and not ok[b + h - 1] and ok[b + h] and ok[b + h - span], ok
    return Case("contig-cut", g, aim, contig_starts=[0, b + h])


def ambiguous(pattern):
    """one ambiguous base x bases into the second copy only: the windows over it are invalid, two records"""
    span = RM.care_offsets(pattern)[1]
    rng = np.random.default_rng(_seed_of("ambiguous", pattern))
    L, x = 5 * span, 2 * span + 1
    E = bg(rng, L)
    g, pos = assemble([bg(rng, 40), E, bg(rng, 45), E, bg(rng, 40)])
    a, b = pos[1], pos[3]
    direct_flanks(g, [(a, L), (b, L)], span)
    inv = np.zeros(len(g), bool); inv[b + x] = True

    def aim(rec):
        assert has(rec, x, (a + 1, b + 1)) and has(rec, L - x - 1, (a + x + 2, b + x + 2)), rec
    return Case("ambiguous", g, aim, invalid=inv)


# ---- emit once ----------------------------------------------------------------------------------------------------------------------------
def long_pair(pattern, div):
    """a 600-base direct pair: hundreds of hits on one diagonal, one record; with 5 % substitutions in the second copy the diagonal
    breaks into the reference's handful of records"""
    rng = np.random.default_rng(_seed_of("long%d" % int(div * 100), pattern))
    L = 600
    E = bg(rng, L)
    E2 = E.copy()
    hit = np.flatnonzero(rng.random(L) < div)
    E2[hit] = (E2[hit] + rng.integers(1, 4, len(hit))) & 3
    g, pos = assemble([bg(rng, 50), E, bg(rng, 60), E2, bg(rng, 50)])
    a, b = pos[1], pos[3]
    direct_flanks(g, [(a, L), (b, L)], RM.care_offsets(pattern)[1])

    def aim(rec):
        diag = [r for r in rec if len(r[1]) == 2 and r[1][1] - r[1][0] == b - a and r[1][0] > 0]
        if div == 0:
            assert diag == [(L, (a + 1, b + 1))], diag
        else:
            assert 1 <= len(diag) <= 60 and len(hit) > 10 and all(x[1][0] + x[0] <= y[1][0] + RM.care_offsets(pattern)[1] for x, y in zip(diag, diag[1:])), diag
    return Case("long-pair-%d" % int(div * 100), g, aim)


# ---- canonical order ------------------------------------------------------------------------------------------------------------------------
def order_ties(pattern):
    """three copies of E, the second with one substitution at x2, the third with one at x1: the windows over x1 are 2-fold (copies 1, 2),
    those over x2 are 2-fold (copies 1, 3), the rest 3-fold.  Where one substitution does not break a chain (a seed with a don't-care
    position; a solid seed: no case) all three diagonals span the whole of E: three records with the same start 0, two of them 2-fold"""
    span = RM.care_offsets(pattern)[1]
    if max(_killed_runs(pattern, (2 * span,), 0, 4 * span)) >= span:
        return None
    rng = np.random.default_rng(_seed_of("ties", pattern))
    L = 6 * span
    E = bg(rng, L)
    E2, E3 = E.copy(), E.copy()
    E2[4 * span] = (E2[4 * span] + 1) & 3
    E3[2 * span] = (E3[2 * span] + 2) & 3
    g, pos = assemble([bg(rng, 40), E, bg(rng, 41), E2, bg(rng, 43), E3, bg(rng, 40)])
    a, b, c = pos[1], pos[3], pos[5]
    direct_flanks(g, [(a, L), (b, L), (c, L)], span)

    def aim(rec):
        same = [r for r in rec if r[1][0] == a + 1]
        assert same == [(L, (a + 1, b + 1)), (L, (a + 1, c + 1)), (L, (a + 1, b + 1, c + 1))], rec
    return Case("order-ties", g, aim)


def all_cases(pattern, walks=True):
    """every planted case that exists for the pattern"""
    span = RM.care_offsets(pattern)[1]
    out = []
    if walks:
        out += [walk(pattern, lo, hi) for lo in EDGES for hi in EDGES]
    out += [chain(pattern, k) for k in ("span", "span+1", "dontcare")]
    out += [inverted(pattern, s, L) for s in (0, 1, 2, span - 1, span, 2 * span) for L in (3 * span, 3 * span + 1)]
    out += [selfcomp(pattern, k) for k in ("inverted", "direct")]
    out += [nesting(pattern, side, st) for side in ("left", "right", "both") for st in ("FFF", "FRF", "RFF")]
    out += [nesting(pattern, "both", "FRF", min_multi=3), nesting(pattern, "both", "FFF", max_multi=2)]
    out += [copies(pattern, 30), copies(pattern, 31), homopolymer(pattern)]
    out += [tandem(pattern, p, n) for p in (3, span + 1) for n in (6, 20)]
    out += [flush(pattern), contig_cut(pattern), ambiguous(pattern), long_pair(pattern, 0.0), long_pair(pattern, 0.05), order_ties(pattern)]
    return [c for c in out if c is not None]
