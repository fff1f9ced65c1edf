"""numpy restatement of the scoring of an alignment against a correct one: score_records(truth, calc, nseq) -> the
records [N, N, 8] of mauve_score_alignment, totals(records) -> the figures of scoreAlignment.cpp.  Both alignments are dicts with left,
right, reverse [n_iv, N], col_off, cols (the arrays of a fetched alignment); positions follow S14 (1-based, present iff left != 0)."""
import numpy as np

WORDS = 8
TP, FP_BASE, FP_GAP, FN_UNALIGNED, FN_BASE, TN = range(6)


def _arrays(aln, N):
    left = np.asarray(aln["left"], np.int64).reshape(-1, N)
    right = np.asarray(aln["right"], np.int64).reshape(-1, N)
    rev = np.asarray(aln["reverse"]).reshape(-1, N)
    return left, right, rev, np.asarray(aln["col_off"], np.int64), np.asarray(aln["cols"], np.uint32)


def _positions(c, g, left, right, rev):
    """1-based position of genome g's residue in each column of one interval (0 where it has none)"""
    present = (c >> np.uint32(g) & np.uint32(1)).astype(bool)
    k = np.cumsum(present) - 1
    return np.where(present, (right - k) if rev else (left + k), 0).astype(np.int64)


def score_records(truth, calc, nseq):
    N = int(nseq)
    tl, tr, trev, toff, tcols = _arrays(truth, N)
    cl, cr, crev, coff, ccols = _arrays(calc, N)
    size = int(max(tr.max(initial=0), cr.max(initial=0))) + 1
    # the calculated alignment, per genome i: the interval that covers every base (-1: none) and its column in the whole array
    c_iv = np.full((N, size), -1, np.int64)
    c_col = np.zeros((N, size), np.int64)
    c_pos = np.zeros((N, len(ccols)), np.int64)                  # position of every genome's residue in every column (0: none)
    for iv in range(cl.shape[0]):
        c = ccols[coff[iv]:coff[iv + 1]]
        for g in range(N):
            if not cl[iv, g]:
                continue
            p = _positions(c, g, int(cl[iv, g]), int(cr[iv, g]), bool(crev[iv, g]))
            c_pos[g, coff[iv]:coff[iv + 1]] = p
            at = np.flatnonzero(p)
            c_iv[g, p[at]] = iv
            c_col[g, p[at]] = coff[iv] + at
    rec = np.zeros((N, N, WORDS), np.int64)
    for iv in range(tl.shape[0]):
        c = tcols[toff[iv]:toff[iv + 1]]
        pos = [_positions(c, g, int(tl[iv, g]), int(tr[iv, g]), bool(trev[iv, g])) if tl[iv, g] else np.zeros(len(c), np.int64) for g in range(N)]
        for i in range(N):
            at = np.flatnonzero(pos[i])
            if not len(at):
                continue
            p = pos[i][at]
            civ, ccol = c_iv[i, p], c_col[i, p]
            found = civ >= 0
            for j in range(N):
                if j == i:
                    continue
                T = pos[j][at]
                inside = found & (cl[np.maximum(civ, 0), j] != 0) if cl.shape[0] else np.zeros(len(at), bool)
                P = np.where(inside, c_pos[j, ccol] if len(ccols) else 0, 0)
                has, hit = T != 0, P != 0
                r = rec[i, j]
                r[TP] += np.count_nonzero(has & hit & (P == T))
                r[FP_BASE] += np.count_nonzero(has & hit & (P != T))
                r[FP_GAP] += np.count_nonzero(has & ~hit & inside)
                r[FN_UNALIGNED] += np.count_nonzero(has & ~hit & ~inside)
                r[FN_BASE] += np.count_nonzero(~has & hit)
                r[TN] += np.count_nonzero(~has & ~hit)
    return rec


def totals(records):
    """the tool's totals: a truth base-base pair counts once, from the lower sequence index; a base-gap pair from the side with the base"""
    rec = np.asarray(records, np.int64)
    N = rec.shape[0]
    up = np.triu(np.ones((N, N), bool), 1)
    off = ~np.eye(N, dtype=bool)
    tp = int(rec[up, TP].sum())
    fp = int(rec[up, FP_BASE].sum() + rec[up, FP_GAP].sum())
    un = int(rec[up, FN_UNALIGNED].sum())
    fn = un + int(rec[off, FN_BASE].sum())
    tn = int(rec[off, TN].sum())
    return {"tp": tp, "tn": tn, "fp": fp, "fn": fn, "total": tp + tn + fp + fn, "unaligned_fn": un,
            "sensitivity": tp / max(tp + fn, 1), "specificity": tn / max(tn + fp, 1)}
