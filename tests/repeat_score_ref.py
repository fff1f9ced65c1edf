"""The frozen form of DESIGN.md S22 in plain Python: a repeat map scored against a correct alignment of the copies of its repeats.
Written from the text of S22; it calls nothing of the library.

Truth: dict(left, right, reverse [n_iv, nseq], col_off [n_iv + 1], cols [n_cols] uint32) as Context.score_truth takes it; its rows are the
copy slots of a repeat, an interval is one repeat family.  row_offset[nseq]: genome bases in front of every row's origin.
Map: (length [n], mult [n], start_off [n + 1], starts) as mauve_repeat_fetch lays it out.
-> dict(totals, pair_records [nseq, nseq, 4] int64, comp_hit [n] uint32, pair_hit [n_starts] uint32)"""
import numpy as np

TOTALS = ("sp_possible", "sp_truepos", "sp_exact", "components", "components_hit", "component_pairs", "component_pairs_hit", "reserved")
WORDS = 4


def truth_positions(truth, row_offset=None):
    """per interval: int64 [nseq, n_cols of the interval], the genome position of every row at every column (0: gapped or absent) -- S14's
    rule: the k-th residue of a row lies at left + k, of a reverse row at right - k"""
    left, right, rev = (np.asarray(truth[k]) for k in ("left", "right", "reverse"))
    col_off, cols = np.asarray(truth["col_off"], np.int64), np.asarray(truth["cols"], np.uint32)
    n_iv, N = left.shape
    off = np.zeros(N, np.int64) if row_offset is None else np.asarray(row_offset, np.int64)
    out = []
    for iv in range(n_iv):
        c = cols[col_off[iv]:col_off[iv + 1]]
        P = np.zeros((N, len(c)), np.int64)
        for g in range(N):
            if not left[iv, g]:
                continue
            present = ((c >> np.uint32(g)) & np.uint32(1)).astype(bool)
            k = np.cumsum(present) - 1
            P[g] = np.where(present, (right[iv, g] - k if rev[iv, g] else left[iv, g] + k) + off[g], 0)
        out.append(P)
    return out


def score(truth, records, row_offset=None):
    length, mult, off, starts = (np.asarray(a, np.int64) for a in records)
    n = len(length)
    rev = np.asarray(truth["reverse"])
    N = rev.shape[1]
    cover = {}                                       # genome position -> the (record, component) pairs whose extent holds it
    ext = []
    for r in range(n):
        comps = []
        for c in range(int(mult[r])):
            s = int(starts[off[r] + c])
            lo = abs(s)
            hi = lo + int(length[r]) - 1
            comps.append((lo, hi, s < 0))
            for q in range(lo, hi + 1):
                cover.setdefault(q, []).append((r, c))
        ext.append(comps)
    pairs = np.zeros((N, N, WORDS), np.int64)
    comp_hit = np.zeros(n, np.uint32)
    pair_hit = np.zeros(int(off[n]) if n else 0, np.uint32)
    for iv, P in enumerate(truth_positions(truth, row_offset)):
        for x in range(P.shape[1]):
            rows = [g for g in range(N) if P[g, x]]
            for a, i in enumerate(rows):
                for j in rows[a + 1:]:
                    qi, qj = int(P[i, x]), int(P[j, x])
                    same_t = bool(rev[iv, i]) == bool(rev[iv, j])
                    pairs[i, j, 0] += 1
                    sup = exact = False
                    for r, c1 in cover.get(qi, ()):
                        lo1, hi1, neg1 = ext[r][c1]
                        col1 = hi1 - qi if neg1 else qi - lo1
                        for c2, (lo2, hi2, neg2) in enumerate(ext[r]):
                            if c2 == c1 or not lo2 <= qj <= hi2 or (neg1 == neg2) != same_t:
                                continue
                            sup = True
                            exact = exact or (hi2 - qj if neg2 else qj - lo2) == col1
                            comp_hit[r] |= np.uint32((1 << c1) | (1 << c2))
                            pair_hit[off[r] + min(c1, c2)] |= np.uint32(1 << max(c1, c2))
                    pairs[i, j, 1] += sup
                    pairs[i, j, 2] += exact
    pop = lambda a: int(sum(bin(int(v)).count("1") for v in a))
    totals = dict(sp_possible=int(pairs[:, :, 0].sum()), sp_truepos=int(pairs[:, :, 1].sum()), sp_exact=int(pairs[:, :, 2].sum()),
                  components=int(mult.sum()), components_hit=pop(comp_hit), component_pairs=int((mult * (mult - 1) // 2).sum()),
                  component_pairs_hit=pop(pair_hit), reserved=0)
    return dict(totals=totals, pair_records=pairs, comp_hit=comp_hit, pair_hit=pair_hit)


def ppv(t):
    r = lambda a, b: a / b if b else 0.0
    return dict(sensitivity=r(t["sp_truepos"], t["sp_possible"]), exact_sensitivity=r(t["sp_exact"], t["sp_possible"]),
                component_ppv=r(t["components_hit"], t["components"]), pairwise_ppv=r(t["component_pairs_hit"], t["component_pairs"]))
