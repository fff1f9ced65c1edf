"""A plain restatement of DESIGN.md S7 (gapped alignment of one interval) and of the S13 objective, in Python integers.

Nothing here shares code with oracle/ or with the library.  Minus infinity is a real minus infinity, so there is no clamp:
at the sizes of the tests no reachable cell of the int32 formulation comes anywhere near -2^29, and the states that hold
minus infinity are never chosen and never walked through.

S7: progressive in genome order over the non-empty sequences; a step aligns the profile (m columns of per-base counts,
k rows) with the next sequence by a three-state affine DP -- M (column on base), X (column against a gap), Y (base against a
gap) -- with sub(i, b) = sum_a cnt_i[a] * S[a][b], a gap run costing `open` for its first column and `extend` for every
further one, scaled by the residues it faces (the residues of column i for X, the k rows for Y).  Every state may follow
every state; among equal predecessors M is preferred, then X, then Y, in every state and in the final cell."""
import numpy as np

NEG = float("-inf")


def _best(a, b, c):
    """value and index of the first of (M, X, Y) that attains the maximum"""
    if a >= b and a >= c:
        return a, 0
    if b >= c:
        return b, 1
    return c, 2


def profile_step(cnt, k_rows, seq, S, go, ge):
    """profile columns cnt[i] = [nA, nC, nG, nT] with k_rows rows against seq -> (ops left to right, score);
    ops: 3 column on base, 1 column against a gap, 2 base against a gap"""
    m, n = len(cnt), len(seq)
    if m == 0 and n == 0:
        return [], 0
    M = [[NEG] * (n + 1) for _ in range(m + 1)]
    X = [[NEG] * (n + 1) for _ in range(m + 1)]
    Y = [[NEG] * (n + 1) for _ in range(m + 1)]
    pM = [[0] * (n + 1) for _ in range(m + 1)]
    pX = [[0] * (n + 1) for _ in range(m + 1)]
    pY = [[0] * (n + 1) for _ in range(m + 1)]
    M[0][0] = 0
    gyo, gye = go * k_rows, ge * k_rows
    for i in range(m + 1):
        if i:
            c = cnt[i - 1]
            r = c[0] + c[1] + c[2] + c[3]
            gxo, gxe = go * r, ge * r
            sub = [sum(c[a] * S[a][b] for a in range(4)) for b in range(4)]
        for j in range(n + 1):
            if i and j:
                v, p = _best(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1])
                M[i][j], pM[i][j] = v + sub[seq[j - 1]], p
            if i:
                v, p = _best(M[i - 1][j] + gxo, X[i - 1][j] + gxe, Y[i - 1][j] + gxo)
                X[i][j], pX[i][j] = v, p
            if j:
                v, p = _best(M[i][j - 1] + gyo, X[i][j - 1] + gyo, Y[i][j - 1] + gye)
                Y[i][j], pY[i][j] = v, p
    score, state = _best(M[m][n], X[m][n], Y[m][n])
    ops, i, j = [], m, n
    while i or j:
        if state == 0:
            ops.append(3); state = pM[i][j]; i -= 1; j -= 1
        elif state == 1:
            ops.append(1); state = pX[i][j]; i -= 1
        else:
            ops.append(2); state = pY[i][j]; j -= 1
    return ops[::-1], int(score)


def align_interval(seqs, S, go, ge):
    """seqs: sequences of codes 0..3, one per genome slot (empty ones take no part) -> (column masks, sum of the step scores)"""
    cnt, mask, k, total = [], [], 0, 0
    for g, s in enumerate(seqs):
        s = [int(b) for b in s]
        if not s:
            continue
        if k == 0:
            cnt = [[int(b == a) for a in range(4)] for b in s]
            mask = [1 << g] * len(s)
            k = 1
            continue
        ops, sc = profile_step(cnt, k, s, S, go, ge)
        total += sc
        cnt2, mask2, pi, sj = [], [], 0, 0
        for op in ops:
            c, mk = [0, 0, 0, 0], 0
            if op & 1:
                c, mk = list(cnt[pi]), mask[pi]
                pi += 1
            if op & 2:
                c[s[sj]] += 1
                mk |= 1 << g
                sj += 1
            cnt2.append(c)
            mask2.append(mk)
        cnt, mask, k = cnt2, mask2, k + 1
    return mask, total


def sp_score_cols(seqs, cols, S, go, ge):
    """S13: for every pair of non-empty sequences, over the columns at least one of them is in: a column with both scores
    S[base of the lower slot][base of the higher slot], a maximal run of columns with only one of them `open` for its first
    column and `extend` for each further one"""
    total = 0
    for a in range(len(seqs)):
        for b in range(a + 1, len(seqs)):
            if not len(seqs[a]) or not len(seqs[b]):
                continue
            pa = pb = 0
            prev = 0
            for c in cols:
                ha, hb = int(c) >> a & 1, int(c) >> b & 1
                if ha and hb:
                    total += S[int(seqs[a][pa])][int(seqs[b][pb])]
                    prev = 0
                elif ha or hb:
                    side = 1 if ha else 2
                    total += ge if prev == side else go
                    prev = side
                pa += ha
                pb += hb
    return total


def match_sp_scores(genomes, length, start, S, mults=None, mode=0):
    """S11 in numpy: for every column of an ungapped match and every pair x < y of its present components, S[b_x][b_y]; a reverse
    component (negative start) is read from its right end and complemented.  S11d.3 with `mults` (one multiplicity per base) and
    mode 1 (NEGATIVE) / 2 (ZERO): a positive pair score s becomes s (2 - r) / r or s / r, truncated toward zero, with r the larger
    multiplicity of the two positions; scores <= 0 stay"""
    S = np.asarray(S, np.int64)
    start = np.asarray(start, np.int64)
    out = np.zeros(len(length), np.int64)
    for i, L in enumerate(np.asarray(length, np.int64).tolist()):
        comp = []
        for g in range(start.shape[1]):
            st = int(start[i, g])
            if not st:
                continue
            pos = np.arange(st - 1, st - 1 + L) if st > 0 else np.arange(-st - 1 + L - 1, -st - 2, -1)
            b = np.asarray(genomes[g], np.int64)[pos]
            comp.append((3 - b if st < 0 else b, np.asarray(mults[g], np.int64)[pos] if mode else None))
        for x in range(len(comp)):
            for y in range(x + 1, len(comp)):
                s = S[comp[x][0], comp[y][0]]
                if mode:
                    r = np.maximum(comp[x][1], comp[y][1])
                    num = s * (2 - r) if mode == 1 else s
                    s = np.where(s > 0, np.sign(num) * (np.abs(num) // r), s)
                out[i] += int(s.sum())
    return out
