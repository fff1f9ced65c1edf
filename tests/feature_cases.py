"""Planted inputs of the range map and the overlap join, shared by tests/test_feature_cpu.py and
tests/test_gpu_feature.py: the queries of the hand case, a built alignment whose intervals and query ends sit on the block, word and
sample edges of the coordinate index, the tie cases of `best`, and the planted and shuffled tables of the join."""
import numpy as np

from tests.coord_ref import CoordRef
from tests.project_ref import HAND

BLOCK, SAMPLE = 448, 512                       # columns per block record and residues between two samples of the index
BIG = (1 << 31) - 1


def ref_of(a):
    return CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])


def _q(rows):
    rows = np.array(rows, np.int64).reshape(-1, 3)
    return rows[:, 0].astype(np.int32), rows[:, 1].copy(), rows[:, 2].copy()


# HAND (tests/project_ref.py): interval 0 is reversed in genome 0, interval 3 lacks genome 1.  Genome 0 holds [1,4] [6,8] [12,14] [20,22].
# One base; one interval exactly; one base beyond each end; all intervals of genome 0; wholly between two intervals; then genome 2
# across its reversed interval 2 and a range that runs past everything.
HAND_QUERIES = _q([(0, 2, 2), (0, 6, 8), (0, 5, 9), (0, 1, 22), (0, 15, 19), (2, 41, 50), (1, 4, 6), (0, 22, BIG)])
HAND_WANT = dict(
    piece_off=[0, 1, 2, 3, 7, 7, 9, 11, 12], covered=[1, 3, 3, 13, 0, 3, 2, 1], best=[0, 1, 2, 3, -1, 7, 10, 11],
    piece_query=[0, 1, 2, 3, 3, 3, 3, 5, 5, 6, 6, 7], piece_iv=[0, 1, 1, 0, 1, 2, 3, 2, 3, 0, 1, 3],
    piece_col=[4, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0, 3], piece_len=[1, 4, 4, 6, 4, 3, 4, 2, 1, 1, 1, 1],
    clip_lo=[2, 6, 6, 1, 6, 12, 20, 41, 50, 4, 6, 22], clip_hi=[2, 8, 8, 4, 8, 14, 22, 42, 50, 4, 6, 22],
    n_res=[[1, 1, 0], [3, 3, 3], [3, 3, 3], [4, 4, 5], [3, 3, 3], [3, 3, 3], [3, 0, 3], [2, 2, 2], [1, 0, 1], [1, 1, 1], [1, 1, 1], [1, 0, 1]],
    ext_left=[[-2, 3, 0], [6, 6, 10], [6, 6, 10], [-1, 1, 30], [6, 6, 10], [12, 9, -40], [20, 0, 50], [12, 9, -41], [20, 0, 50], [-1, 4, 34], [6, 6, 10], [22, 0, 52]],
    ext_right=[[-2, 3, 0], [8, 8, 12], [8, 8, 12], [-4, 4, 34], [8, 8, 12], [14, 11, -42], [22, 0, 52], [13, 10, -42], [20, 0, 50], [-1, 4, 34], [6, 6, 10], [22, 0, 52]])

# two pieces of equal clipped length, the greater interval id second and first in genome 0's order; then three equal ones
TIES = dict(left=np.array([[1, 1], [11, 21], [41, 41], [31, 61], [71, 0], [81, 0], [76, 0]], np.int64),
            right=np.array([[10, 10], [20, 30], [50, 50], [40, 70], [75, 0], [85, 0], [80, 0]], np.int64),
            reverse=np.array([[0, 0], [0, 1], [1, 0], [0, 0], [0, 0], [0, 0], [1, 0]], np.int8),
            col_off=np.array([0, 10, 20, 30, 40, 45, 50, 55], np.int64),
            cols=np.concatenate([np.full(40, 3, np.uint32), np.full(15, 1, np.uint32)]))
TIES_QUERIES = _q([(0, 1, 20), (0, 31, 50), (0, 5, 16), (0, 35, 46), (0, 71, 85), (0, 1, 85), (0, 9, 12), (0, 39, 43)])
TIES_BEST_IV = [1, 3, 1, 3, 6, 3, 1, 2]


LENS = (1, 63, 64, 65, 447, 448, 449, 3000, 450, 3000, 1, 130)
GAPS = (0, 1, 7, 0, 30)
STRETCH = 7                                    # the interval in which genome 1 has only gaps in columns [1000, 1600) but for column 1300, and genome 0 a residue in each


def built(N, seed):
    """an alignment of N >= 2 genomes whose intervals are 1, 63, 64, 65, 447, 448, 449 and 3000 columns long, so that they begin and end
    around multiples of 64 and 448 columns.  Every genome meets the intervals in an order of its own, on a strand of its own, with 0, 1,
    7 or 30 bases between two of them; with three or more genomes every third interval lacks the last one.  -> (alignment, genome lengths)"""
    rng = np.random.default_rng(seed)
    K = len(LENS)
    bits, present = [], np.ones((K, N), bool)
    for i, L in enumerate(LENS):
        if N > 2 and i % 3 == 1:
            present[i, N - 1] = False
        b = (rng.random((L, N)) < 0.75) & present[i]
        b[rng.random(L) < 0.1] = False                                              # columns of no genome
        b[0] = b[L - 1] = present[i]
        if i == STRETCH:
            b[1000:1600, 0], b[1000:1600, 1], b[1300, 1] = True, False, True
        bits.append(b)
    rev = (rng.random((K, N)) < 0.5) & present
    left, right = np.zeros((K, N), np.int64), np.zeros((K, N), np.int64)
    lens = np.zeros(N, np.int64)
    for g in range(N):
        nxt = 1
        for k, i in enumerate(rng.permutation(K)):
            if present[i, g]:
                left[i, g], right[i, g] = nxt, nxt + bits[i][:, g].sum() - 1
                nxt = right[i, g] + 1 + GAPS[(k + g) % len(GAPS)]
        lens[g] = nxt + 10
    cols = np.concatenate([(b.astype(np.uint64) << np.arange(N, dtype=np.uint64)).sum(axis=1).astype(np.uint32) for b in bits])
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    return dict(left=left, right=right, reverse=rev.astype(np.int8), col_off=off, cols=cols), lens


def edge_residues(R):
    """(genome, position) of the residues that sit in columns 0, 1, 63, 64, 65 and 447 of a block of the index (447, 448 and 449 columns
    into it and its neighbour), that have the ordinals 511, 512, 513 and 1023, 1024, 1025 of their genome in the whole column array, and
    that are the first and the last of an interval row -> int64 [k, 2], and the labels of the kinds that occur"""
    n_cols = len(R.bits)
    iv_of = np.repeat(np.arange(R.n_iv, dtype=np.int64), np.diff(R.col_off))
    out, kinds = [], set()
    xs = np.array([b * BLOCK + o for b in range(n_cols // BLOCK + 1) for o in (0, 1, 63, 64, 65, 447) if b * BLOCK + o < n_cols], np.int64)
    pos, _ = R.column_positions(iv_of[xs], xs - R.col_off[iv_of[xs]])
    for k, g in zip(*np.nonzero(pos)):
        out.append((g, abs(int(pos[k, g]))))
        kinds.add("col%d" % (xs[k] % BLOCK))
    for g in range(R.N):
        for T in (SAMPLE - 1, SAMPLE, SAMPLE + 1, 2 * SAMPLE - 1, 2 * SAMPLE, 2 * SAMPLE + 1):
            if T < R.cum[-1, g]:
                x = int(np.searchsorted(R.cum[1:, g], T, side="right"))           # the column that holds the residue with T in front of it
                p, _ = R.column_positions([iv_of[x]], [x - R.col_off[iv_of[x]]])
                if p[0, g]:                                                        # (its interval may lack the genome's row: then the bit is another's)
                    out.append((g, abs(int(p[0, g]))))
                    kinds.add("rank%d" % T)
        for i in np.flatnonzero(R.left[:, g]):
            out += [(g, int(R.left[i, g])), (g, int(R.right[i, g]))]
    return np.array(out, np.int64).reshape(-1, 2), kinds


def built_queries(a, lens):
    """the ranges of the built alignment: around every edge residue (the residue alone, 40 bases to either side, to the next edge residue
    of the genome), the stretch in which genome 1 has no residue / its only one in the first / the last column, between two intervals,
    every genome whole and past its end"""
    R = ref_of(a)
    e, _ = edge_residues(R)
    rows = []
    for g in range(R.N):
        p = np.unique(e[e[:, 0] == g, 1])
        for k, x in enumerate(p):
            rows += [(g, x, x), (g, max(1, x - 40), x), (g, x, x + 40)]
            if k + 1 < len(p):
                rows.append((g, x, p[k + 1]))
        t = R.by_left[g]
        for u, v in zip(t[:-1], t[1:]):
            if R.left[v, g] - R.right[u, g] > 1:
                rows.append((g, R.right[u, g] + 1, R.left[v, g] - 1))               # no piece
            rows.append((g, R.right[u, g], R.left[v, g]))                            # one base of each
        rows += [(g, 1, BIG), (g, 1, lens[g]), (g, lens[g] - 5, lens[g] + 100)]
    c = np.array([1100, 1200, 1300, 1400], np.int64)
    p0 = np.abs(R.column_positions(np.full(4, STRETCH), c)[0][:, 0])
    rows += [(0, min(p0[u], p0[v]), max(p0[u], p0[v])) for u, v in ((0, 1), (1, 2), (2, 3), (0, 3))]
    return _q(rows)


def no_piece_queries(a, lens, n):
    """n ranges of the built alignment that meet no interval: behind every genome's last base"""
    g = np.arange(n, dtype=np.int64) % a["left"].shape[1]
    lo = np.asarray(lens, np.int64)[g] + np.arange(n, dtype=np.int64) % 7
    return g.astype(np.int32), lo, lo + 50


def random_queries(a, seed, per_genome=200):
    """about per_genome seeded ranges of every genome, and every interval's ends one base to either side"""
    rng = np.random.default_rng(seed)
    left, right = np.asarray(a["left"], np.int64), np.asarray(a["right"], np.int64)
    rows = []
    for g in range(left.shape[1]):
        top = int(right[:, g].max()) + 20
        lo = rng.integers(1, top, per_genome)
        ln = np.where(rng.random(per_genome) < 0.5, rng.integers(0, 30, per_genome), rng.integers(0, top, per_genome))
        rows += [(g, x, x + y) for x, y in zip(lo, ln)]
        for i in np.flatnonzero(left[:, g]):
            for x in (left[i, g] - 1, left[i, g], left[i, g] + 1, right[i, g] - 1, right[i, g], right[i, g] + 1):
                if x >= 1:
                    rows += [(g, x, x), (g, x, x + 3), (g, max(1, x - 3), x)]
    return _q(rows)


# the join, planted.  Genome 0: a long entry that contains short ones, a duplicate, and two pairs of entries that tie in both index
# orders; genome 1: nothing; genome 2: two adjacent entries; genome 3: one entry; genome 5: one entry
JOIN_TAB = _q([(0, 1, 1000), (0, 10, 20), (2, 100, 200), (0, 15, 18), (0, 10, 20), (0, 500, 510), (2, 201, 300), (3, 50, 60),
               (0, 2010, 2019), (0, 2030, 2039), (0, 3030, 3039), (0, 3010, 3019), (5, 7, 7)])
JOIN_QUERIES = _q([(0, 12, 16), (0, 10, 20), (0, 19, 30), (0, 600, 700), (0, 1000, 1500), (0, 1001, 1500),            # inside the long entry, at its last base, behind it
                   (2, 200, 200), (2, 90, 100), (2, 200, 201), (2, 301, 400), (2, 1, 99), (2, 1, 50), (2, 5000, 6000),  # one shared base at either end, adjacent, before, behind
                   (3, 61, 70), (3, 40, 49), (3, 60, 61), (3, 49, 50), (3, 1, BIG),
                   (1, 1, 1000), (4, 1, 1000), (31, 1, 5), (5, 7, 7), (5, 1, 6), (5, 8, 9),                             # empty slices between and behind non-empty ones
                   (0, 2015, 2034), (0, 3015, 3034), (0, 2019, 2030), (0, 3019, 3030),                                  # equal overlaps in both index orders
                   (0, 0, 0), (2, 0, 0), (2, -120, -150), (0, -12, -18), (3, -60, -60), (1, -1, -5)])
JOIN_WANT = dict(n_hit=[4, 4, 3, 1, 1, 0,  1, 1, 2, 0, 0, 0, 0,  0, 0, 1, 1, 1,  0, 0, 0, 1, 0, 0,  2, 2, 2, 2,  0, 0, 1, 4, 1, 0],
                 best=[4, 4, 0, 0, 0, -1,  2, 2, 6, -1, -1, -1, -1,  -1, -1, 7, 7, 7,  -1, -1, -1, 12, -1, -1,  9, 11, 9, 11,  -1, -1, 2, 4, 7, -1],
                 overlap=[5, 11, 12, 101, 1, 0,  1, 1, 1, 0, 0, 0, 0,  0, 0, 1, 1, 11,  0, 0, 0, 1, 0, 0,  5, 5, 1, 1,  0, 0, 31, 7, 1, 0])
# the tie entries alone: the greater table index wins, whichever of the two lies first
JOIN_TIES_TAB = tuple(v[8:12] for v in JOIN_TAB)
JOIN_TIES_QUERIES = _q([(0, 2015, 2034), (0, 3015, 3034), (0, 2019, 2030), (0, 3019, 3030)])
JOIN_TIES_WANT = dict(n_hit=[2, 2, 2, 2], best=[1, 3, 1, 3], overlap=[5, 5, 1, 1])


def shuffled_table(m, seed):
    """m annotated ranges in shuffled order over the genomes 0, 1, 3 and 6 (2, 4 and 5 stay empty): short ones, nested ones, duplicates"""
    rng = np.random.default_rng(seed)
    seq = rng.choice([0, 1, 3, 6], m)
    lo = rng.integers(1, 60000, m)
    ln = np.where(rng.random(m) < 0.02, rng.integers(1000, 5000, m), rng.integers(0, 300, m))
    dup = rng.random(m) < 0.05
    src = rng.integers(0, m, m)
    seq, lo, ln = np.where(dup, seq[src], seq), np.where(dup, lo[src], lo), np.where(dup, ln[src], ln)
    return seq.astype(np.int32), lo.astype(np.int64), (lo + ln).astype(np.int64)


def shuffled_queries(tab, n, seed):
    """n queries against a shuffled table: around its entries' ends, anywhere, in the empty genomes, signed, nothing"""
    rng = np.random.default_rng(seed)
    ts, tl, th = tab
    k = rng.integers(0, len(ts), n)
    seq = np.where(rng.random(n) < 0.8, ts[k], rng.integers(0, 8, n))
    lo = np.where(rng.random(n) < 0.5, np.where(rng.random(n) < 0.5, tl[k], th[k]) + rng.integers(-2, 3, n), rng.integers(1, 66000, n))
    lo = np.maximum(lo, 1)
    hi = lo + np.where(rng.random(n) < 0.5, rng.integers(0, 4, n), rng.integers(0, 2000, n))
    neg = rng.random(n) < 0.3
    lo, hi = np.where(neg, -lo, lo), np.where(neg, -hi, hi)
    none = rng.random(n) < 0.05
    return seq.astype(np.int32), np.where(none, 0, lo).astype(np.int64), np.where(none, 0, hi).astype(np.int64)


def gene_table(a, seed, per_genome=40):
    """a planted annotation of the alignment a: per genome about per_genome genes of 30 to 900 bases in shuffled order, some overlapping
    -> one (seq, lo, hi) table of all genomes"""
    rng = np.random.default_rng(seed)
    right = np.asarray(a["right"], np.int64)
    rows = []
    for g in range(right.shape[1]):
        top = int(right[:, g].max())
        lo = rng.integers(1, max(2, top - 30), per_genome)
        rows += [(g, x, min(top + 50, x + y)) for x, y in zip(lo, rng.integers(30, 900, per_genome))]
    rows = [rows[k] for k in rng.permutation(len(rows))]
    return _q(rows)
