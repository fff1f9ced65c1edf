"""numpy restatement of the range map and the interval-overlap join: the expected value of every device answer in
tests/test_gpu_feature.py, pinned itself in tests/test_feature_cpu.py against the S14 restatement's single-position calls, the column
bits of the fixtures, a host C++ walk (tests/cpp/feature_map_test.cpp) and a per-base brute force.  Independent of the product (no import
of it).  The pieces come from CoordRef (tests/coord_ref.py); the join is the O(n * m) comparison of every query with every table entry.

(a) The pieces of a query (seq, lo, hi) are the intervals in which seq is present and whose [left, right] in seq shares a base with
[lo, hi], by ascending left end.  Per piece: the clip, the columns of its two ends (the smaller one and their distance plus 1), and per
genome the residues in those columns with the smallest and the greatest position among them, negative on a reverse row.
(b) Per query: piece_off, covered = the sum of the clipped lengths, best = the piece of the greatest (clipped length, interval id).
(c) Per query of the join: the table entries of its genome sharing a base with it, the table index of the one sharing the most (ties:
the greater index), that number of bases; ends may be signed, (0, 0) is nothing."""
import numpy as np

PER_QUERY = ("piece_off", "covered", "best")
PER_PIECE = ("piece_query", "piece_iv", "piece_col", "piece_len", "clip_lo", "clip_hi")
PER_ROW = ("n_res", "ext_left", "ext_right")
ARRAYS = PER_QUERY + PER_PIECE + PER_ROW


def map_ranges(R, seq, lo, hi):
    """R: a CoordRef.  -> dict of the twelve arrays of mauve_map_ranges_fetch"""
    seq, lo, hi = np.asarray(seq, np.int64), np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    n, N = len(seq), R.N
    assert np.all((seq >= 0) & (seq < N) & (lo >= 1) & (lo <= hi))
    off, covered, best = [0], [], []
    pq, piv, clo, chi = [], [], [], []
    for q in range(n):
        g, t = int(seq[q]), R.by_left[int(seq[q])]
        hit = t[(R.left[t, g] <= hi[q]) & (R.right[t, g] >= lo[q])]                  # ascending left end: by_left's order
        a, b = np.maximum(R.left[hit, g], lo[q]), np.minimum(R.right[hit, g], hi[q])
        pq += [q] * len(hit)
        piv += hit.tolist()
        clo += a.tolist()
        chi += b.tolist()
        size = b - a + 1
        covered.append(int(size.sum()))
        best.append(off[-1] + max(range(len(hit)), key=lambda k: (size[k], hit[k])) if len(hit) else -1)
        off.append(off[-1] + len(hit))
    pq, piv, clo, chi = (np.array(v, np.int64) for v in (pq, piv, clo, chi))
    P = len(pq)
    s = seq[pq] if P else np.zeros(0, np.int64)
    i1, c1 = R.seqpos_to_column(s, clo)
    i2, c2 = R.seqpos_to_column(s, chi)
    assert np.array_equal(i1, piv) and np.array_equal(i2, piv)
    col, ln = np.minimum(c1, c2), np.abs(c1 - c2) + 1                              # (on a reverse row the two columns swap)
    x0 = R.col_off[piv] + col
    present = R.left[piv] != 0
    r0 = R.cum[x0] - R.cum[R.col_off[piv]]                                         # residues of the interval in front of the range, [P, N]
    n_res = np.where(present, R.cum[x0 + ln] - R.cum[x0], 0)
    first, last = R._signed(piv, r0), R._signed(piv, r0 + n_res - 1)               # in column order
    some = n_res > 0
    rev = R.rev[piv]
    ext_left = np.where(some, np.where(rev, last, first), 0)                        # the smallest position: the last column's on a reverse row
    ext_right = np.where(some, np.where(rev, first, last), 0)
    return dict(piece_off=np.array(off, np.int64), covered=np.array(covered, np.int64).reshape(n), best=np.array(best, np.int64).reshape(n),
                piece_query=pq, piece_iv=piv, piece_col=col, piece_len=ln, clip_lo=clo, clip_hi=chi,
                n_res=n_res.astype(np.int64).reshape(P, N), ext_left=ext_left.astype(np.int64).reshape(P, N), ext_right=ext_right.astype(np.int64).reshape(P, N))


def same(got, want, names=ARRAYS):
    """the names in which two range maps differ (arrays compared by shape, type and value)"""
    return [k for k in names if not (got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]


def range_overlaps(tab, queries):
    """tab, queries: (seq, lo, hi) -> (n_hit, best, overlap) int64 per query"""
    ts, tl, th = (np.asarray(v, np.int64) for v in tab)
    qs, ql, qh = (np.asarray(v, np.int64) for v in queries)
    assert np.all((tl >= 1) & (tl <= th))
    n = len(qs)
    n_hit, best, overlap = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for q in range(n):
        if ql[q] == 0 and qh[q] == 0:
            continue
        assert ql[q] != 0 and qh[q] != 0 and (ql[q] < 0) == (qh[q] < 0)
        a, b = abs(int(ql[q])), abs(int(qh[q]))
        assert a <= b
        shared = np.where(ts == qs[q], np.minimum(th, b) - np.maximum(tl, a) + 1, 0)
        hit = np.flatnonzero(shared > 0)
        if len(hit):
            k = hit[shared[hit] == shared[hit].max()][-1]
            n_hit[q], best[q], overlap[q] = len(hit), k, shared[k]
    return n_hit, best, overlap


def mean_identity(records):
    """[n_pair, 32] pair-statistics records of one range -> the mean of identical / both over the pairs in which both have a residue
    somewhere (in pair order), 0.0 without one"""
    total, count = 0.0, 0
    for s in np.asarray(records, np.int64):
        both = int(s[:25].sum())
        if both > 0:
            total += float(int(s[0] + s[6] + s[12] + s[18] + s[24])) / float(both)
            count += 1
    return total / count if count else 0.0


def ortholog_rows(R, genes, features, pair_records):
    """getOrthologList's row for every gene (seq, lo, hi): its best piece, in every genome the feature of `features` (one (seq, lo, hi)
    table of all genomes) that shares the most bases with the piece's extent, the mean pairwise identity of the piece, the rearranged
    flag.  pair_records(ranges) -> [n_range, n_pair, 32] of all pairs a < b.  -> dict(piece_iv, ortholog [n, N], overlap [n, N],
    identity [n], rearranged [n])"""
    m = map_ranges(R, *genes)
    n, N = len(m["best"]), R.N
    have = np.flatnonzero(m["best"] >= 0)
    b = m["best"][have]
    out = dict(piece_iv=np.full(n, -1, np.int64), ortholog=np.full((n, N), -1, np.int64), overlap=np.zeros((n, N), np.int64), identity=np.zeros(n, np.float64),
               rearranged=(np.diff(m["piece_off"]) > 1).astype(np.int8))
    out["piece_iv"][have] = m["piece_iv"][b]
    qs = np.tile(np.arange(N, dtype=np.int64), len(have))
    _, best, ov = range_overlaps(features, (qs, m["ext_left"][b].reshape(-1), m["ext_right"][b].reshape(-1)))
    out["ortholog"][have], out["overlap"][have] = best.reshape(len(have), N), ov.reshape(len(have), N)
    if len(have):
        rec = pair_records((m["piece_iv"][b], m["piece_col"][b], m["piece_len"][b]))
        out["identity"][have] = [mean_identity(rec[k]) for k in range(len(have))]
    return out
