"""CPU reference of the repeat penalty: numpy over the oracle's per-window mers (oracle.pyoracle.mers) and its LCB
chaining on given weights (orc_compute_lcbs_w), and the genome sets with planted repeats that the CPU and GPU tests share.  Read-only
use of the oracle; nothing here needs a GPU."""
import ctypes as C

import numpy as np

from mauvealigner_amd import synth
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


def repeat_genomes(n, L, seed, copies=12, elem=(300, 1500), div=0.02):
    """n genomes of about L bases from one ancestor that carries `copies` planted copies (half of them reverse-complemented,
    each point-mutated by 3 %) of one repeat element, then mutated per genome at `div`"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, L).astype(np.uint8)
    e = rng.integers(0, 4, int(rng.integers(*elem))).astype(np.uint8)
    for k, p in enumerate(np.sort(rng.choice(L - len(e), copies, replace=False)).tolist()):
        c = e.copy()
        hit = rng.random(len(c)) < 0.03
        c[hit] = (c[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        anc[p:p + len(c)] = synth.revcomp(c) if k % 2 else c
    return [synth.mutate(anc, div, np.random.default_rng(seed * 100 + g)) for g in range(n)]


def _blocks_and_repeats(seed, tag=0):
    """two genomes: unique blocks U0..U7 in the same order, a copy of one 300-base element E between every two; the caller's match
    list pairs U_k with U_k and the copies of E out of order.  tag > 0: copy j is E between two unique tags of `tag` bases, and
    genome 1 holds it in slot perm[j], so the genomes' own seed search finds the copies paired out of order (the tags seed them)
    while the tags break the diagonal of the blocks"""
    rng = np.random.default_rng(seed)
    U = [rng.integers(0, 4, 800).astype(np.uint8) for _ in range(8)]
    E = rng.integers(0, 4, 300).astype(np.uint8)
    perm = [3, 0, 5, 1, 6, 2, 4]
    if tag:
        cp = [np.concatenate([rng.integers(0, 4, tag), E, rng.integers(0, 4, tag)]).astype(np.uint8) for _ in range(7)]
    else:
        cp = [E] * 7
    le = len(cp[0])
    g0, pos_u, pos_e = [], [], []
    at = 0
    for k in range(8):
        pos_u.append(at); g0.append(U[k]); at += 800
        if k < 7:
            pos_e.append(at); g0.append(cp[k]); at += le
    g0 = np.concatenate(g0)
    g1 = g0.copy()
    for p in pos_u:
        hit = np.flatnonzero(rng.random(800) < 0.01) + p
        g1[hit] = (g1[hit] + 1) & 3
    for j in range(7):
        g1[pos_e[perm[j]]:pos_e[perm[j]] + le] = cp[j]
    ln, st = [], []
    for p in pos_u:
        ln.append(800); st.append([p + 1, p + 1])
    for j, p in enumerate(pos_e):
        ln.append(le); st.append([p + 1, pos_e[perm[j]] + 1])
    order = np.argsort([s[0] for s in st], kind="stable")
    return [g0, g1], np.array(ln, np.int64)[order], np.array(st, np.int64)[order]
