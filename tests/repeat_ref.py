"""CPU reference of the repeat penalty: numpy over the oracle's per-window mers (oracle.pyoracle.mers) and its LCB
chaining on given weights (orc_compute_lcbs_w).  Read-only use of the oracle; nothing here needs a GPU."""
import ctypes as C

import numpy as np

from oracle import pyoracle as O

OFF, NEGATIVE, ZERO = 0, 1, 2


def window_valid(L, span, contig_starts=None, invalid=None):
    """S3 validity of every window start of a genome of length L: inside one contig, no ambiguous base"""
    nw = max(0, L - span + 1)
    ok = np.ones(nw, bool)
    if nw == 0:
        return ok
    if invalid is not None:
        c = np.concatenate([[0], np.cumsum(np.asarray(invalid, bool)[:L])])
        ok &= (c[span:span + nw] - c[:nw]) == 0
    for b in (contig_starts or []):
        if 0 < b < L:                                   # a window may not run across the join in front of base b
            ok[max(0, b - span + 1):min(nw, b)] = False
    return ok


def window_counts(codes, pattern, contig_starts=None, invalid=None):
    """cnt_g(w) of every valid window (0 for an invalid one), not saturated"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    span = O.seed_length(pattern)
    canon, _ = O.mers(codes, pattern)
    ok = window_valid(len(codes), span, contig_starts, invalid)
    cnt = np.zeros(len(canon), np.int64)
    if ok.any():
        _, inv, counts = np.unique(canon[ok], return_inverse=True, return_counts=True)
        cnt[ok] = counts[inv]
    return cnt


def multiplicity(codes, pattern, contig_starts=None, invalid=None):
    """m_g(p): minimum of the (saturated) counts of the valid windows covering p, 1 where none does -> uint8[L]"""
    L = len(codes)
    span = O.seed_length(pattern)
    cnt = np.minimum(window_counts(codes, pattern, contig_starts, invalid), 255)
    big = np.where(cnt > 0, cnt, 256)
    m = np.full(L, 256, np.int64)
    nw = len(big)
    for d in range(span):                               # window w covers positions w .. w + span - 1
        if nw:
            m[d:d + nw] = np.minimum(m[d:d + nw], big)
    m[m == 256] = 1
    return m.astype(np.uint8)


def _tdiv(a, r):
    """C integer division (truncation toward zero), r > 0"""
    return np.sign(a) * (np.abs(a) // r)


def penalize(s, r, mode):
    """pair score of S11d from the substitution score s and r = max multiplicity (arrays, int64)"""
    s = np.asarray(s, np.int64)
    r = np.asarray(r, np.int64)
    if mode == OFF:
        return s
    p = _tdiv(s * (2 - r), r) if mode == NEGATIVE else _tdiv(s, r)
    return np.where(s > 0, p, s)


def sp_scores_repeat(seqs, mults, length, start, mode, matrix):
    """penalized sum-of-pairs score of every ungapped match (S11 columns, S11d pairs)"""
    M = np.asarray(matrix, np.int64)
    start = np.asarray(start, np.int64)
    out = np.zeros(len(length), np.int64)
    for i, ln in enumerate(np.asarray(length, np.int64).tolist()):
        if ln <= 0:
            continue
        c = np.arange(ln, dtype=np.int64)
        comp = []
        for g in range(start.shape[1]):
            st = int(start[i, g])
            if not st:
                continue
            p = st - 1 + c if st > 0 else -st - 1 + (ln - 1 - c)
            b = np.asarray(seqs[g], np.int64)[p]
            if st < 0:
                b = 3 - b
            comp.append((b, np.asarray(mults[g], np.int64)[p]))
        acc = 0
        for x in range(len(comp)):
            for y in range(x + 1, len(comp)):
                s = M[comp[x][0], comp[y][0]]
                acc += int(penalize(s, np.maximum(comp[x][1], comp[y][1]), mode).sum())
        out[i] = acc
    return out


def compute_lcbs_w(length, start, weights, min_weight, collinear=False):
    """the oracle's LCB chaining on given match weights (orc_compute_lcbs_w)"""
    m, keep = O._np_to_matches(length, start)
    w = np.ascontiguousarray(weights, dtype=np.int64)
    out = O.Lcbs()
    O.lib().orc_compute_lcbs_w(C.byref(m), w.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int64(int(min_weight)), int(collinear),
                               C.byref(out))
    d = O._lcbs_to_dict(out, len(keep[0]))
    O.lib().orc_free_lcbs(C.byref(out))
    return d
