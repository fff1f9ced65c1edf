"""Restatement of the excursions of the column scores: the expected value of every device answer in
tests/test_gpu_excursions.py, pinned itself in tests/test_excursion_cpu.py against hand cases, pinned fixture totals and the output of the
reference's own loop.  Independent of the product (no import of it).  It works on the rows of ExtractRef.extract() (tests/extract_ref.py):
a cell is the S15 cell, letters A C G T N -> 0..4 as in S16, N scoring as A.

Two walks of one value stream: walk_rules, the four rules written out (the definition), and walk, the same in numpy through the max-form
x_c = max(0, x_{c-1} + v_c).  tests/test_excursion_cpu.py holds them equal; the large GPU shapes use the second."""
import numpy as np

from tests.pairstats_ref import all_pairs, letter_codes

FRACTIONS = (.95, .99, .999, .9999)


def walk_rules(v, cols):
    """the four rules of S18 on the values v (v = -s) of a stream whose columns are cols -> (heights, end columns, (x, h) at the end)"""
    x = h = 0
    hs, es = [], []
    for val, c in zip([int(t) for t in v], [int(t) for t in cols]):
        if x > 0 and x + val < 0:
            hs.append(h)
            es.append(c)
            x = h = 0
        elif x == 0 and val > 0:
            x = val
            h = max(h, x)
        elif x > 0:
            x += val
            h = max(h, x)
    return np.array(hs, np.int64), np.array(es, np.int64), (x, h)


def walk(v, cols):
    """the max-form: x_c = max(0, x_{c-1} + v_c) = S_c - min(0, min S_j); an emission at c iff x_{c-1} > 0 and x_{c-1} + v_c < 0; h is the
    maximum of x since the last emission or the start"""
    v = np.asarray(v, np.int64)
    cols = np.asarray(cols, np.int64)
    if len(v) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), (0, 0)
    S = np.cumsum(v)
    x = S - np.minimum(0, np.minimum.accumulate(S))
    xp = np.concatenate([[0], x[:-1]])
    e = np.flatnonzero((xp > 0) & (xp + v < 0))
    # the pieces between emissions: [0, e0), [e0, e1), ...; x is 0 at an emission, so it may stand in either piece (e0 > 0: x starts at 0)
    starts = np.concatenate([[0], e])
    seg = np.maximum.reduceat(x, starts)
    # (a piece [e_k, e_{k+1}) holds the x of e_k = 0 and of the columns up to e_{k+1} - 1: the height the emission at e_{k+1} reports)
    heights = seg[:len(e)].copy()
    return heights.astype(np.int64), cols[e], (int(x[-1]), int(seg[-1]))


def pair_values(x, y, matrix, gap_open, gap_extend):
    """codes x, y (0..4, 5 = '-') of one range -> (the stream's column indices inside the range, v = -s there)"""
    m = np.asarray(matrix, np.int64)[np.ix_([0, 1, 2, 3, 0], [0, 1, 2, 3, 0])]
    occ = np.flatnonzero((x != 5) | (y != 5))
    xo, yo = x[occ].astype(np.int64), y[occ].astype(np.int64)
    kind = np.where(yo == 5, 1, np.where(xo == 5, 2, 0))
    prev = np.concatenate([[-1], kind[:-1]])
    s = np.where(kind == 0, m[np.minimum(xo, 4), np.minimum(yo, 4)], np.where(prev != kind, gap_open, gap_extend))
    return occ, -s.astype(np.int64)


def core_values(codes, members, matrix):
    """codes [N, n] of one range, members: ascending genome ids -> (column indices where all have a residue, v = -sum over g < h of matrix)"""
    m = np.asarray(matrix, np.int64)[np.ix_([0, 1, 2, 3, 0], [0, 1, 2, 3, 0])]
    sub = codes[members].astype(np.int64)
    occ = np.flatnonzero(np.all(sub != 5, axis=0))
    s = np.zeros(len(occ), np.int64)
    for i in range(len(members)):
        for j in range(i + 1, len(members)):
            s += m[sub[i, occ], sub[j, occ]]
    return occ, -s


class Result:
    def __init__(self, height, end_col, stream_off, tail):
        self.height, self.end_col, self.stream_off, self.tail = height, end_col, stream_off, tail

    def arrays(self):
        return self.height, self.end_col, self.stream_off, self.tail


def _ranges(E, ranges):
    if ranges is None:
        return np.arange(E.n_iv, dtype=np.int64), np.zeros(E.n_iv, np.int64), np.diff(E.col_off).astype(np.int64)
    return tuple(np.asarray(t, np.int64) for t in ranges)


def _run(E, ranges, n_set, values, walker):
    rows = E.extract()[0]                               # every interval whole, all genomes: the ranges are slices of it
    codes = letter_codes(rows)
    r_iv, r_col, r_len = _ranges(E, ranges)
    hs, es, off, tail = [], [], [0], []
    for i, c, n in zip(r_iv.tolist(), r_col.tolist(), r_len.tolist()):
        x0 = int(E.col_off[i]) + c
        part = codes[:, x0:x0 + n]
        for k in range(n_set):
            occ, v = values(part, k)
            h, e, t = walker(v, occ + c)
            hs.append(h)
            es.append(e)
            off.append(off[-1] + len(h))
            tail.append(t)
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    return Result(cat(hs), cat(es), np.array(off, np.int64), np.array(tail, np.int64).reshape(-1, 2))


def excursions_pairs(E, matrix, gap_open, gap_extend, pairs=None, ranges=None, walker=walk):
    """E: an ExtractRef -> Result; streams range-major, stream = r * n_pair + k"""
    pa, pb = all_pairs(E.N) if pairs is None else pairs
    pa, pb = [int(t) for t in pa], [int(t) for t in pb]
    return _run(E, ranges, len(pa), lambda part, k: pair_values(part[pa[k]], part[pb[k]], matrix, gap_open, gap_extend), walker)


def excursions_core(E, matrix, masks=None, ranges=None, walker=walk):
    """masks: genome masks or lists of genome ids (None: one group of every genome)"""
    masks = [(1 << E.N) - 1] if masks is None else [int(m) if np.ndim(m) == 0 else sum(1 << int(g) for g in m) for m in masks]
    members = [[g for g in range(E.N) if m >> g & 1] for m in masks]
    return _run(E, ranges, len(masks), lambda part, k: core_values(part, members[k], matrix), walker)


def thresholds(height):
    """evd.cpp:108-126: the height at index min((size_t)(n * f), n - 1) of the sorted heights, and n minus that index; zeros for n = 0"""
    h = np.sort(np.asarray(height, np.int64))
    n = len(h)
    if n == 0:
        return [0] * 4, [0] * 4
    idx = [min(int(float(n) * f), n - 1) for f in FRACTIONS]
    return [int(h[i]) for i in idx], [n - i for i in idx]
