"""numpy restatement of the pairwise column statistics: the expected value of every device answer in
tests/test_gpu_pairstats.py, pinned itself in tests/test_pairstats_cpu.py against a scalar state machine written out there and against
hand-counted cases.  Independent of the product (no import of it).  It counts on the rows of ExtractRef.extract() (tests/extract_ref.py):
a cell is the S15 cell.

A record is WORDS int64 for one ordered pair (a, b) over one range, x the cell of a and y the cell of b, letters A C G T N -> 0..4:
[5x + y] both have a residue, [25] only a, [26] only b, [27] / [28] the only_a / only_b columns that open a run (their nearest earlier
column of the same range that is not `neither` is missing or of another kind), [29] neither, [30] and [31] zero."""
import numpy as np

WORDS = 32
ONLY_A, ONLY_B, RUNS_A, RUNS_B, NEITHER = 25, 26, 27, 28, 29
DIAG = [0, 6, 12, 18, 24]


def all_pairs(N):
    """the default pair list: a < b, row-major in the upper triangle"""
    a, b = np.triu_indices(N, 1)
    return a.astype(np.int32), b.astype(np.int32)


def letter_codes(rows):
    """uint8 letters -> A C G T N = 0..4, '-' = 5"""
    lut = np.full(256, 255, np.uint8)
    for k, ch in enumerate(b"ACGTN-"):
        lut[ch] = k
    codes = lut[rows]
    assert not np.any(codes == 255)
    return codes


def count_rows(codes, rid, R, pairs):
    """the records of the pairs over the code matrix [N, n] whose column j belongs to range instance rid[j] (ascending) -> [R, P, 32]"""
    pa, pb = pairs
    out = np.zeros((R, len(pa), WORDS), np.int64)
    for p, (a, b) in enumerate(zip(pa, pb)):
        x, y = codes[a].astype(np.int64), codes[b].astype(np.int64)
        t = np.bincount(rid * 36 + 6 * x + y, minlength=R * 36).reshape(R, 6, 6)
        out[:, p, :25] = t[:, :5, :5].reshape(R, 25)
        out[:, p, ONLY_A] = t[:, :5, 5].sum(axis=1)
        out[:, p, ONLY_B] = t[:, 5, :5].sum(axis=1)
        out[:, p, NEITHER] = t[:, 5, 5]
        occ = np.flatnonzero((x != 5) | (y != 5))
        kind = np.where(y[occ] == 5, 1, np.where(x[occ] == 5, 2, 0))                  # 1: only a, 2: only b, 0: both
        r = rid[occ]
        prev = np.concatenate([[-1], kind[:-1]])
        prev[np.concatenate([[True], r[1:] != r[:-1]])] = -1                          # the range's first occupied column: no predecessor
        for k, slot in ((1, RUNS_A), (2, RUNS_B)):
            out[:, p, slot] = np.bincount(r[(kind == k) & (prev != k)], minlength=R)
    return out


def pair_stats(E, pairs=None, ranges=None, per_range=False):
    """E: an ExtractRef.  -> int64 [n_pair, 32], with per_range [n_range, n_pair, 32]; the totals are the sums of the per-range records"""
    if pairs is None:
        pairs = all_pairs(E.N)
    pairs = tuple(np.asarray(v, np.int64) for v in pairs)
    rows, _, _, roff = E.extract(ranges=ranges)
    R = len(roff) - 1
    rid = np.repeat(np.arange(R, dtype=np.int64), np.diff(roff))
    out = count_rows(letter_codes(rows), rid, R, pairs)
    return out if per_range else out.sum(axis=0)


def identity(stats):
    st = np.asarray(stats, np.int64)
    both = st[..., :25].sum(axis=-1)
    same = st[..., DIAG].sum(axis=-1)
    return np.where(both > 0, same / np.maximum(both, 1), 0.0)


def sp_score(stats, matrix, gap_open, gap_extend):
    """N scores as A"""
    st = np.asarray(stats, np.int64)
    m = np.asarray(matrix, np.int64)
    m5 = m[np.ix_([0, 1, 2, 3, 0], [0, 1, 2, 3, 0])].reshape(25)
    runs = st[..., RUNS_A] + st[..., RUNS_B]
    return (st[..., :25] * m5).sum(axis=-1) + gap_open * runs + gap_extend * (st[..., ONLY_A] + st[..., ONLY_B] - runs)
