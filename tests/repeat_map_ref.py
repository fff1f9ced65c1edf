"""Plain-Python restatement of DESIGN.md S20, the repeat matches of one genome (mauve_repeat_matches): families from a dict of
canonical mers, the agreement test offset by offset, clusters, the emit-once rule, the canonical order.  Written from the text of
S20, not from the kernels; nothing here needs a GPU or the oracle."""
import numpy as np

MAX_MULT = 32


def care_offsets(pattern):
    """offsets of the care positions of the seed, leftmost first (S2: bit span-1-t of the pattern is offset t)"""
    span = int(pattern).bit_length()
    return [t for t in range(span) if (int(pattern) >> (span - 1 - t)) & 1], span


def window_valid(L, span, contig_starts=None, invalid=None):
    """S3: a window is valid iff it lies inside one contig and holds no ambiguous base"""
    nw = max(0, L - span + 1)
    ok = [True] * nw
    if invalid is not None:
        bad = [i for i in range(min(L, len(invalid))) if invalid[i]]
        for i in bad:
            for p in range(max(0, i - span + 1), min(nw, i + 1)):
                ok[p] = False
    for b in (contig_starts or []):
        if 0 < b < L:
            for p in range(max(0, b - span + 1), min(nw, b)):      # windows that would run across the join in front of base b
                ok[p] = False
    return ok


def window_mers(codes, pattern):
    """forward and reverse-complement masked mer of every window (S3: care positions, leftmost most significant)"""
    care, span = care_offsets(pattern)
    codes = [int(x) for x in codes]
    nw = max(0, len(codes) - span + 1)
    F, R = [0] * nw, [0] * nw
    for p in range(nw):
        f = r = 0
        for t in care:
            f = f * 4 + codes[p + t]
            r = r * 4 + (3 - codes[p + span - 1 - t])
        F[p], R[p] = f, r
    return F, R, span


def families(codes, pattern, contig_starts=None, invalid=None):
    """canonical mer -> ascending positions of its valid windows; plus F, R, the validity and the strand flags"""
    F, R, span = window_mers(codes, pattern)
    ok = window_valid(len(codes), span, contig_starts, invalid)
    fam = {}
    flag = [0] * len(F)
    for p in range(len(F)):
        flag[p] = 1 if R[p] < F[p] else 0
        if ok[p]:
            fam.setdefault(min(F[p], R[p]), []).append(p)
    return fam, F, R, ok, flag, span


def canonical(records):
    """ascending start of component 0, then multiplicity, then the signed starts, then length"""
    return sorted(records, key=lambda r: (r[1][0], len(r[1]), r[1], r[0]))


def repeat_matches(codes, pattern, min_multi=2, max_multi=MAX_MULT, contig_starts=None, invalid=None, extend=True):
    """-> list of (length, (signed 1-based starts)) in canonical order"""
    assert 2 <= max_multi <= MAX_MULT
    fam, F, R, ok, flag, span = families(codes, pattern, contig_starts, invalid)
    nw = len(F)
    size = [0] * nw
    for P in fam.values():
        for p in P:
            size[p] = len(P)
    lo = max(2, min_multi)
    out = []
    for P in fam.values():
        m = len(P)
        if not (lo <= m <= max_multi):
            continue
        rev = [flag[p] != flag[P[0]] for p in P]

        def at(k):
            return [p - k if r else p + k for p, r in zip(P, rev)]

        def agrees(k):
            Q = at(k)
            if any(q < 0 or q >= nw for q in Q):                            # 1. every window inside the genome
                return False
            for c in range(m):                                              # 2. the position order of k = 0 (opposite directions only)
                for d in range(m):
                    if rev[c] != rev[d] and not rev[c]:
                        if (Q[c] - Q[d] > 0) != (P[c] - P[d] > 0) or Q[c] == Q[d]:
                            return False
            if not all(ok[q] for q in Q):
                return False
            w0 = F[Q[0]]
            return all((R[q] if r else F[q]) == w0 for q, r in zip(Q, rev))

        def is_hit(k):
            """the family at an agreeing offset is a hit of this diagonal: exactly m windows, the diagonal's strand relations"""
            Q = at(k)
            return size[Q[0]] == m and all((flag[q] != flag[Q[0]]) == r for q, r in zip(Q, rev))

        if not extend:
            out.append((span, tuple(-(p + 1) if r else p + 1 for p, r in zip(P, rev))))
            continue
        k_lo, k, dropped = 0, -1, False
        while k >= k_lo - span:                                             # the left walk: agreeing offsets at most span apart
            if agrees(k):
                if is_hit(k):
                    dropped = True                                          # a hit of the diagonal with a lower k emits the cluster
                    break
                k_lo = k
            k -= 1
        if dropped:
            continue
        k_hi, k = 0, 1
        while k <= k_hi + span:
            if agrees(k):
                k_hi = k
            k += 1
        out.append(((k_hi - k_lo) + span, tuple(-(p - k_hi + 1) if r else p + k_lo + 1 for p, r in zip(P, rev))))
    return canonical(out)


def as_csr(records):
    """the records as mauve_repeat_fetch lays them out: length, mult, start_off, starts (int64)"""
    length = np.array([r[0] for r in records], np.int64)
    mult = np.array([len(r[1]) for r in records], np.int64)
    off = np.concatenate([[0], np.cumsum(mult)]).astype(np.int64)
    starts = np.array([s for r in records for s in r[1]], np.int64)
    return length, mult, off, starts


def from_csr(length, mult, off, starts):
    return [(int(length[i]), tuple(int(s) for s in starts[off[i]:off[i + 1]])) for i in range(len(length))]
