"""Planted cases for the repeat-map score, each with the figures worked out by hand: `CASES` maps a name to
dict(truth, row_offset, records, totals).  Shared by tests/test_repeat_score_cpu.py (the restatement against the hand figures) and
tests/test_gpu_repeat_score.py (the device against the restatement).  `random_case` makes the sized inputs of the GPU test."""
import numpy as np


def truth_of(intervals, nseq):
    """intervals: list of {row: (left, reverse, pattern)}; pattern: one character per column, '-' a gap; right = left + residues - 1"""
    left = np.zeros((len(intervals), nseq), np.int64)
    right = np.zeros_like(left)
    rev = np.zeros((len(intervals), nseq), np.int8)
    col_off, cols = [0], []
    for k, iv in enumerate(intervals):
        width = len(next(iter(iv.values()))[2])
        c = np.zeros(width, np.uint32)
        for g, (lf, rv, pat) in iv.items():
            assert len(pat) == width and lf >= 1
            bits = np.array([ch != "-" for ch in pat])
            assert bits.any()
            left[k, g], right[k, g], rev[k, g] = lf, lf + int(bits.sum()) - 1, int(rv)
            c |= bits.astype(np.uint32) << np.uint32(g)
        cols.append(c)
        col_off.append(col_off[-1] + width)
    return dict(left=left, right=right, reverse=rev, col_off=np.array(col_off, np.int64),
                cols=np.concatenate(cols) if cols else np.zeros(0, np.uint32))


def csr(records):
    """records: list of (length, (signed starts)) -> length, mult, start_off, starts"""
    length = np.array([r[0] for r in records], np.int64)
    mult = np.array([len(r[1]) for r in records], np.int64)
    off = np.concatenate([[0], np.cumsum(mult)]).astype(np.int64)
    starts = np.array([s for r in records for s in r[1]], np.int64)
    return length, mult, off, starts


def _tot(possible, truepos, exact, comps, comps_hit, cpairs, cpairs_hit):
    return dict(sp_possible=possible, sp_truepos=truepos, sp_exact=exact, components=comps, components_hit=comps_hit, component_pairs=cpairs,
                component_pairs_hit=cpairs_hit, reserved=0)


def _case(intervals, nseq, records, totals, row_offset=None):
    return dict(truth=truth_of(intervals, nseq), row_offset=None if row_offset is None else np.array(row_offset, np.int64), records=csr(records), totals=totals)


X10 = "x" * 10
CASES = {}
# one family of three copies, the middle one reversed: base 101 + x pairs with 210 - x and 301 + x; the reverse component -201 holds base q
# in column 210 - q: all 3 * 10 pairs are supported exactly
CASES["hand3"] = _case([{0: (101, 0, X10), 1: (201, 1, X10), 2: (301, 0, X10)}], 3, [(10, (101, -201, 301))], _tot(30, 30, 30, 3, 3, 3, 3))
# the same in the tool's concatenated form: rows as contigs of 200, 100 and 100 bases
CASES["hand3_concat"] = _case([{0: (101, 0, X10), 1: (1, 1, X10), 2: (1, 0, X10)}], 3, [(10, (101, -201, 301))], _tot(30, 30, 30, 3, 3, 3, 3), row_offset=[0, 200, 300])
# both bases of every pair lie in component 0 (101 .. 120) and in no other: c1 == c2 is no alignment
CASES["same_component"] = _case([{0: (101, 0, X10), 1: (106, 0, X10)}], 2, [(20, (101, 501))], _tot(10, 0, 0, 2, 0, 1, 0))
# a tandem record, period 5: base 106 + x lies in components 0 and 1, base 111 + x in 1 and 2.  Pair x = (101 + x, 106 + x): (0, 1) always and
# exactly; for x >= 5 also (1, 2), exactly, and (0, 2), columns x and x - 5.  Pairing the k-th elements of two intersections would miss two of them
CASES["tandem"] = _case([{0: (101, 0, X10), 1: (106, 0, X10)}], 2, [(10, (101, 106, 111))], _tot(10, 10, 10, 3, 3, 3, 3))
# the chain holds every pair but on the wrong strand
CASES["orientation"] = _case([{0: (101, 0, X10), 1: (201, 0, X10)}], 2, [(10, (101, -201))], _tot(10, 0, 0, 2, 0, 1, 0))
# an indel between the copies: row 1 lacks column 5, so behind it base 101 + x pairs with 200 + x, one column off in the ungapped match
CASES["indel"] = _case([{0: (101, 0, X10), 1: (201, 0, "xxxxx-xxxx")}], 2, [(10, (101, 201))], _tot(9, 9, 5, 2, 2, 1, 1))
# two families, the first without row 2
CASES["absent_row"] = _case([{0: (101, 0, X10), 1: (201, 0, X10)}, {0: (401, 0, "xxxxx"), 1: (501, 0, "xxxxx"), 2: (601, 0, "xxxxx")}], 3,
                            [(10, (101, 201)), (5, (401, 501, 601))], _tot(25, 25, 25, 5, 5, 4, 4))
# the truth is twice as long as the match: columns 0 .. 4 and 15 .. 19 lie outside every record
CASES["outside"] = _case([{0: (101, 0, "x" * 20), 1: (201, 0, "x" * 20)}], 2, [(10, (106, 206))], _tot(20, 10, 10, 2, 2, 1, 1))
# a 2-copy match of 30 bases running through a 3-copy region of 10
CASES["nested"] = _case([{0: (101, 0, X10), 1: (201, 0, X10), 2: (301, 0, X10)}], 3, [(30, (91, 191)), (10, (101, 201, 301))], _tot(30, 30, 30, 5, 5, 4, 4))
CASES["mult2"] = _case([{0: (11, 0, "xxxx"), 1: (31, 1, "xxxx")}], 2, [(4, (11, -31))], _tot(4, 4, 4, 2, 2, 1, 1))
# 32 copies of 3 bases, the odd ones reversed: 496 row pairs and as many component pairs
CASES["mult32"] = _case([{g: (100 * (g + 1) + 1, g & 1, "xxx") for g in range(32)}], 32,
                        [(3, tuple((-1 if g & 1 else 1) * (100 * (g + 1) + 1) for g in range(32)))], _tot(1488, 1488, 1488, 32, 32, 496, 496))
# one extent of 1000 bases over the first components of 200 matches of 2 bases, whose second components lie elsewhere: every stab under the
# long extent walks back over the short ones in front of it and finds the long one alone
CASES["walk_back"] = _case([{0: (1001, 0, "x" * 1000), 1: (3001, 0, "x" * 1000)}], 2,
                           [(1000, (1001, 3001))] + [(2, (1001 + 5 * k, 5001 + 5 * k)) for k in range(200)], _tot(1000, 1000, 1000, 402, 2, 201, 1))


def random_case(seed, nrows, ncols, n_records, gap=0.1):
    """one truth interval of nrows rows and ncols columns with gaps and reversed rows, and n_records matches cut from it: most follow the
    truth, some carry a wrong strand, a shifted component or a component somewhere else; multiplicities 2 .. min(nrows, 32) and above nrows
    (extra components outside the truth).  -> dict(truth, row_offset, records)"""
    rng = np.random.default_rng(seed)
    stride = ncols + 64
    iv, pos = {}, {}
    for g in range(nrows):
        bits = rng.random(ncols) >= gap
        bits[rng.integers(0, ncols)] = True
        rv = bool(rng.random() < 0.3)
        lf = 1 + g * stride + int(rng.integers(0, 8))
        iv[g] = (lf, rv, "".join("x" if b else "-" for b in bits))
        k = np.cumsum(bits) - 1
        rt = lf + int(bits.sum()) - 1
        pos[g] = np.where(bits, rt - k if rv else lf + k, 0)
    far = 1 + nrows * stride
    recs = []
    for _ in range(n_records):
        m = int(rng.integers(2, min(nrows, 6) + 1)) if rng.random() < 0.9 else int(rng.integers(2, 33))
        rows = rng.permutation(nrows)[:min(m, nrows)]
        a = int(rng.integers(0, ncols))
        ln = int(rng.integers(1, max(2, min(40, ncols - a + 1))))
        st = []
        for g in rows:
            p = int(pos[g][a]) or int(pos[g][pos[g] > 0][0])
            rv = iv[int(g)][1]
            lo = max(1, p - ln + 1 if rv else p) + (int(rng.integers(-3, 4)) if rng.random() < 0.2 else 0)
            st.append((-1 if rv != (rng.random() < 0.1) else 1) * max(1, lo))
        while len(st) < m:
            st.append(int(rng.choice([-1, 1])) * (far + int(rng.integers(0, 500))))
        recs.append((ln, tuple(st)))
    return dict(truth=truth_of([iv], nrows), row_offset=None, records=csr(recs))
