"""Alignments built to break the homology pass, and the scoring schemes they run under.  Every generator is
seeded and returns a case: a dict with the genomes `gs` and `left, right, reverse, col_off, cols` in the layout of
mauve_align_fetch, plus what the tests need to know about what was planted.  The kernels cut an interval into steps of 64
and segments of 4096 columns and re-split the whole column array by tiles of 4096: the sizes below sit on those edges."""
import functools

import numpy as np

from tests import homology_ref as HR

STEP, SEG = 64, 4096

# match, mismatch, gap, go_homologous, go_unrelated
SCHEMES = {
    "default": (1030, -916, -500, -11513, -20723),             # the call site's knobs: identity 0.7, pgh 1e-5, pgu 1e-9
    "cheap": (1030, -916, -500, -4605, -4605),                 # pgh = pgu = 1e-2
    "ties1": (1, -1, -1, -2, -2),
    "ties2": (2, -2, -1, -4, -6),
    "zero": (1, -1, 0, 0, 0),                                  # lo == hi at every column: the state follows the sign of the score
    "posgap": (3, -5, 2, -7, -3),
    "limit": (65536, -65536, -65536, -(1 << 28), -(1 << 28)),  # the largest magnitudes the device accepts
}
PLANT_SCHEME = "cheap"                                          # the planted edges and identity runs are sized for this one
EDGES = (63, 64, 65, 4095, 4096, 4097, 8191, 8192)


def revcomp(x):
    return (3 - x)[::-1]


def mutate(rng, x, rate=0.1):
    """a copy with about `rate` substitutions (each to a different base)"""
    y = x.copy()
    hit = rng.random(len(x)) < rate
    y[hit] = (y[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    return y.astype(np.uint8)


def differ(rng, x):
    """a base different from x at every position"""
    return ((x + rng.integers(1, 4, len(x))) % 4).astype(np.uint8)


def assemble(rng, N, ivs):
    """ivs: per interval (bases [N, L] on the interval's strand, pres [N, L] bool, rev [N] bool).  Genomes are laid out interval after
    interval with a few bases of padding, reverse-strand stretches stored reverse-complemented; columns nobody has are dropped."""
    parts = [[rng.integers(0, 4, 3, dtype=np.uint8)] for _ in range(N)]
    glen = [3] * N
    n_iv = len(ivs)
    left = np.zeros((n_iv, N), np.int64); right = np.zeros((n_iv, N), np.int64); reverse = np.zeros((n_iv, N), np.int8)
    col_off = [0]; cols = []
    for i, (bases, pres, rev) in enumerate(ivs):
        pres = np.asarray(pres, bool)
        mask = np.zeros(pres.shape[1], np.uint32)
        for g in range(N):
            mask |= pres[g].astype(np.uint32) << np.uint32(g)
            seq = np.asarray(bases[g], np.uint8)[pres[g]]
            if not len(seq):
                continue
            pad = rng.integers(0, 4, int(rng.integers(0, 6)), dtype=np.uint8)
            parts[g] += [pad, revcomp(seq) if rev[g] else seq]
            left[i, g] = glen[g] + len(pad) + 1
            glen[g] += len(pad) + len(seq)
            right[i, g] = glen[g]
            reverse[i, g] = 1 if rev[g] else 0
        mask = mask[mask != 0]
        cols.append(mask); col_off.append(col_off[-1] + len(mask))
    gs = [np.ascontiguousarray(np.concatenate(p).astype(np.uint8)) for p in parts]
    return dict(gs=gs, left=left, right=right, reverse=reverse, col_off=np.array(col_off, np.int64),
                cols=np.ascontiguousarray(np.concatenate(cols).astype(np.uint32)))


def args(case):
    return case["gs"], case["left"], case["right"], case["reverse"], case["col_off"], case["cols"]


def _single(rng, N, L):
    """an interval only one genome has"""
    g = int(rng.integers(0, N))
    pres = np.zeros((N, L), bool); pres[g] = True
    return rng.integers(0, 4, (N, L), dtype=np.uint8), pres, np.zeros(N, bool)


# ---------------------------------------------------------------------------------------------- (a) mosaic
def mosaic(seed, N=5, lengths=(1, 63, 64, 65, 4095, 4096, 4097, 2 * SEG + 1)):
    """per interval a random genome subset (>= 2); per genome blocks that are a copy of a common ancestor with about 10 %
    substitutions, random bases, or absent; random strands; single-genome intervals in between"""
    rng = np.random.default_rng(seed)
    ivs = []
    for L in lengths:
        k = int(rng.integers(2, min(N, 4) + 1))
        S = np.sort(rng.choice(N, k, replace=False))
        anc = rng.integers(0, 4, L, dtype=np.uint8)
        bases = np.zeros((N, L), np.uint8); pres = np.zeros((N, L), bool)
        for g in S:
            c = 0
            while c < L:
                n = int(rng.integers(1, max(2, min(L, 700))))
                kind = rng.random()
                e = min(L, c + n)
                if kind < 0.5:
                    bases[g, c:e] = mutate(rng, anc[c:e]); pres[g, c:e] = True
                elif kind < 0.75:
                    bases[g, c:e] = rng.integers(0, 4, e - c); pres[g, c:e] = True
                c = e
            if not pres[g].any():
                pres[g, int(rng.integers(0, L))] = True
        ivs.append((bases, pres, rng.random(N) < 0.4))
        ivs.append(_single(rng, N, int(rng.integers(1, 90))))
    case = assemble(rng, N, ivs)
    case["name"] = "mosaic%d" % seed
    return case


# ---------------------------------------------------------------------------------------------- (b) planted edges
LEAD, BLOCK, TAIL = 20, 40, 60


@functools.lru_cache(maxsize=None)
def _core(seed):
    """LEAD identical columns, a block of BLOCK random bases in genome 1 (first and last differing), TAIL identical columns, and
    where the reference path leaves and re-enters H in it under PLANT_SCHEME (columns relative to the core's start)"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, LEAD + BLOCK + TAIL, dtype=np.uint8)
    other = anc.copy()
    other[LEAD:LEAD + BLOCK] = rng.integers(0, 4, BLOCK)
    other[LEAD:LEAD + 1] = differ(rng, anc[LEAD:LEAD + 1]); other[LEAD + BLOCK - 1:LEAD + BLOCK] = differ(rng, anc[LEAD + BLOCK - 1:LEAD + BLOCK])
    pre = rng.integers(0, 4, 30, dtype=np.uint8)
    L = 30 + len(anc)
    case = assemble(rng, 2, [(np.stack([np.concatenate([pre, anc]), np.concatenate([pre, other])]), np.ones((2, L), bool), np.zeros(2, bool))])
    fl = HR.homology_ref(*args(case), SCHEMES[PLANT_SCHEME])[3][(0, 0, 1)]
    assert [s for _, s in fl] == [0, 1], "the core must leave H once and come back once"
    return anc, other, fl[0][0] - 30, fl[1][0] - 30


def planted(seed, N=2, aligned=False):
    """one interval per (b, direction): an identical pair but for the core's block, placed so that the reference path leaves H
    ('out') or re-enters it ('in') exactly at interval column b.  Each follows a shorter interval, so b is relative to the interval
    and not a multiple of anything in the column array -- or, with `aligned`, a filler makes it start on a multiple of 4096.
    N = 3 adds a third genome related to both.  case['planted'] lists (interval, b, state after the flip)."""
    rng = np.random.default_rng(seed)
    anc, other, d_out, d_in = _core(1000 + seed)
    ivs, plant, at = [], [], 0
    for b in EDGES:
        for new_state, d in ((0, d_out), (1, d_in)):
            short = int(rng.integers(5, 60))
            if aligned:
                short = (-at - 1) % SEG + 1                       # this interval then ends on a multiple of 4096
            pre = rng.integers(0, 4, short, dtype=np.uint8)
            rows = [pre, mutate(rng, pre, 0.02)] + ([mutate(rng, pre)] if N == 3 else [])
            ivs.append((np.stack(rows), np.ones((N, short), bool), np.zeros(N, bool)))
            at += short
            head = rng.integers(0, 4, b - d, dtype=np.uint8)      # b - d identical columns in front: the flip lands on b
            tail = rng.integers(0, 4, int(rng.integers(0, 200)), dtype=np.uint8)
            r0, r1 = np.concatenate([head, anc, tail]), np.concatenate([head, other, tail])
            rows = [r0, r1] + ([mutate(rng, r0)] if N == 3 else [])
            rev = rng.random(N) < 0.5
            plant.append((len(ivs), b, new_state))
            ivs.append((np.stack(rows), np.ones((N, len(r0)), bool), rev))
            at += len(r0)
    case = assemble(rng, N, ivs)
    case["planted"] = plant
    case["name"] = "planted%d_N%d%s" % (seed, N, "_aligned" if aligned else "")
    return case


# ---------------------------------------------------------------------------------------------- (c) identity runs
def identity_runs(seed):
    """N = 3.  Stretches only genome 2 has bases in -- columns pair (0, 1) skips, the identity function on the device -- of 64,
    4096 and 4096 + 70 columns, beginning at a step start, inside a step and at a segment start, once inside a homologous
    region and once inside an unrelated one, with a state change of the pair on each side; and an interval whose first 5000
    columns the pair skips.  case['runs'] lists (interval, first column of the run, length, state carried across)."""
    rng = np.random.default_rng(seed)
    ivs, runs = [], []

    def build(pieces):
        rows = [[], [], []]; pres = [[], [], []]
        for kind, n in pieces:
            a = rng.integers(0, 4, n, dtype=np.uint8)
            rows[0].append(a); rows[2].append(mutate(rng, a))
            rows[1].append(a.copy() if kind == "H" else differ(rng, a))
            for g in range(3):
                pres[g].append(np.full(n, kind != "N" or g == 2))
        return np.stack([np.concatenate(r) for r in rows]), np.stack([np.concatenate(p) for p in pres]), np.zeros(3, bool)

    for length in (STEP, SEG, SEG + 70):
        for start in (10 * STEP, 10 * STEP + 29, SEG):
            runs.append((len(ivs), start, length, 1))
            ivs.append(build([("H", 200), ("U", 150), ("H", start - 350), ("N", length), ("H", 100), ("U", 150), ("H", 100)]))
            runs.append((len(ivs), start, length, 0))
            ivs.append(build([("H", 200), ("U", start - 200), ("N", length), ("U", 100), ("H", 200)]))
    runs.append((len(ivs), 0, 5000, 0))
    ivs.append(build([("N", 5000), ("H", 300), ("U", 200), ("H", 300)]))
    case = assemble(rng, 3, ivs)
    case["runs"] = runs
    case["name"] = "identity%d" % seed
    return case


# ---------------------------------------------------------------------------------------------- (d) tile edges
def tile_edges(seed):
    """N = 3; interval lengths that put several col_off entries, the last one included, on multiples of 4096, with a stretch of
    genome 1 that differs everywhere over the last 60 columns in front of every offset and the first 60 behind it"""
    rng = np.random.default_rng(seed)
    ivs = []
    for L in (SEG, 100, SEG - 100, 2 * SEG, 300, SEG - 300, SEG):
        a = rng.integers(0, 4, L, dtype=np.uint8)
        b = a.copy()
        n = min(60, L // 3)
        b[:n] = differ(rng, a[:n]); b[L - n:] = differ(rng, a[L - n:])
        ivs.append((np.stack([a, b, mutate(rng, a)]), np.ones((3, L), bool), rng.random(3) < 0.3))
    case = assemble(rng, 3, ivs)
    assert case["col_off"][-1] % SEG == 0 and int((case["col_off"][1:] % SEG == 0).sum()) >= 4
    case["name"] = "tiles%d" % seed
    return case


# ---------------------------------------------------------------------------------------------- (e) width
def wide(seed, N, L):
    """one interval with all N genomes (bit N - 1 included): per genome blocks of ancestor copy / random bases / absent"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, L, dtype=np.uint8)
    bases = rng.integers(0, 4, (N, L), dtype=np.uint8)
    pres = np.ones((N, L), bool)
    for g in range(N):
        cuts = np.sort(rng.integers(0, L, max(2, L // 600)))
        edges = [0] + cuts.tolist() + [L]
        for c, e in zip(edges[:-1], edges[1:]):
            kind = rng.random()
            if kind < 0.6:
                bases[g, c:e] = mutate(rng, anc[c:e])
            elif kind > 0.8 and (c or e < L):
                pres[g, c:e] = False
        if not pres[g].any():
            pres[g, 0] = True
    empty = np.flatnonzero(~pres.any(axis=0))                     # a column nobody has would be dropped: the length is part of the case
    pres[rng.integers(0, N, len(empty)), empty] = True
    case = assemble(rng, N, [(bases, pres, rng.random(N) < 0.3)])
    assert (case["left"][0] != 0).all() and len(case["cols"]) == L
    case["name"] = "wide%d_N%d_L%d" % (seed, N, L)
    return case


# ---------------------------------------------------------------------------------------------- the score limits
def limit_cases(seed):
    """N = 2, for the scheme at the device's limits.  (1) 6000 unrelated columns, 14000 identical, 6000 unrelated: entering H costs
    2^28 = 4096 matches of 65536, so a segment's summed score reaches 2^28 and the path flips once each way (the last stretch
    differs everywhere: random bases match too often to pay for leaving).  (2) 8192 and 8193 one-sided columns at gap = -65536
    between identical stretches of 9000: staying in H through them costs exactly the two transitions, 2^29, or one gap more --
    a tie at the largest magnitudes, which stays, and the same case one column past the tie, which leaves.  One-sided columns
    come out the same in either state, so (3) is (2) with the second half of the stretch present in both genomes and differing
    everywhere (mismatch = gap = -65536): at the tie nothing moves, one column further 2 * 4097 residues do."""
    rng = np.random.default_rng(seed)
    out = []
    a = rng.integers(0, 4, 26000, dtype=np.uint8)
    b = a.copy(); b[:6000] = rng.integers(0, 4, 6000); b[20000:] = differ(rng, a[20000:])        # leaving H costs 4096 mismatches: these are 6000
    c = assemble(rng, 2, [(np.stack([a[:50], a[:50]]), np.ones((2, 50), bool), np.zeros(2, bool)), (np.stack([a, b]), np.ones((2, 26000), bool), np.array([False, True]))])
    c["name"] = "limit_flip"; out.append(c)
    for k in (2 * SEG, 2 * SEG + 1):
        L = 9000 + k + 9000
        a = rng.integers(0, 4, L, dtype=np.uint8)
        pres = np.ones((2, L), bool); pres[1, 9000:9000 + k] = False
        c = assemble(rng, 2, [(np.stack([a, a]), pres, np.zeros(2, bool))])
        c["name"] = "limit_gap%d" % k; out.append(c)
        b = a.copy(); b[9000 + SEG:9000 + k] = differ(rng, a[9000 + SEG:9000 + k])
        pres = np.ones((2, L), bool); pres[0, 9000:9000 + SEG] = False
        c = assemble(rng, 2, [(np.stack([a, b]), pres, np.array([True, False]))])
        c["name"] = "limit_mix%d" % k; out.append(c)
    return out


def end_ties(seed):
    """N = 2, short intervals whose last column leaves v_H == v_U under the small-integer schemes (H wins there): k identical
    columns, k identical then j differing ones, 20 identical then j differing ones"""
    rng = np.random.default_rng(seed)
    ivs = []
    for k, j in [(k, 0) for k in range(1, 8)] + [(k, j) for k in range(1, 6) for j in range(1, 6)] + [(20, j) for j in range(1, 9)]:
        a = rng.integers(0, 4, k + j, dtype=np.uint8)
        b = a.copy(); b[k:] = differ(rng, a[k:])
        ivs.append((np.stack([a, b]), np.ones((2, k + j), bool), rng.random(2) < 0.3))
    case = assemble(rng, 2, ivs)
    case["name"] = "endties%d" % seed
    return case


@functools.lru_cache(maxsize=None)
def small_cases():
    """every family at the sizes the Python reference is run on"""
    return tuple([mosaic(1), mosaic(2, N=3), planted(1, 2), planted(2, 3), planted(3, 2, aligned=True), identity_runs(1), tile_edges(1),
                  wide(1, 17, 700), wide(2, 32, 2 * SEG + 3), end_ties(1)] + limit_cases(1))


@functools.lru_cache(maxsize=None)
def big_case():
    """32 genomes, 35 * 4096 + 7 columns: 496 pairs x 36 segments = 17856 waves of work, more than the grid holds at once"""
    return wide(3, 32, 35 * SEG + 7)
