"""DESIGN.md S3 (canonical mers, the MEM / UNIQUE / mask rules, anchor, strand relation) and S4 (agreement of an offset, clusters of
agreeing offsets at most `span` apart, one match per cluster and component set, canonical order) restated from the text with numpy
and Python integers.  Nothing here shares code with oracle/, with the product or with tests/bruteforce.py (which pins it on small
inputs, tests/test_seed_cpu.py).

The form is the plain one: per generalized diagonal ONE boolean agreement array over every anchor window, and a scan of it for gaps
of more than `span`.  No rounds, no bitmaps, no tiles, no hash.

find(genomes, pattern, mode, mask, extend, valid) returns a dict:
  length[n], start[n][N]   the matches in canonical order
  matches[n]               per match: mask, comps, diag ((reverse?, d) per component: window of c = d + q, or d - q when reverse, at
                           anchor window q), qlo, qhi (first and last agreeing anchor window), hits (anchor windows of the cluster's
                           hits, ascending: hits[0] is the leftmost), agree (the agreement array from qlo - span to qhi + span,
                           False outside the genome), agree_from (= qlo - span), diagonal (the whole agreement array of the
                           diagonal, over every anchor window; shared by the diagonal's matches)
  hits                     every seed hit: (mask, comps, windows, strands)
  canon[g], strand[g], ok[g]   per genome: canonical mer, strand flag and validity of every window
  table                    (mer, genome, window, strand) of the valid windows, sorted by (mer, genome, window)"""
import numpy as np

MEM, UNIQUE, PAIRWISE = 0, 1, 2


def shape(pattern):
    s = bin(pattern)[2:]
    return [i for i, ch in enumerate(s) if ch == "1"], len(s)


def window_mers(codes, pattern):
    """forward and reverse-complement masked mers of every window (care positions, leftmost most significant)"""
    offs, span = shape(pattern)
    c = np.asarray(codes, dtype=np.uint64)
    nw = max(len(c) - span + 1, 0)
    F, R = np.zeros(nw, np.uint64), np.zeros(nw, np.uint64)
    for t in offs:
        F = F * np.uint64(4) + c[t:t + nw]
        R = R * np.uint64(4) + (np.uint64(3) - c[span - 1 - t:span - 1 - t + nw])
    return F, R


def window_ok(length, span, intervals):
    nw = max(length - span + 1, 0)
    if intervals is None:
        return np.ones(nw, bool)
    ok = np.zeros(nw, bool)
    for lo, hi in intervals:                       # 1-based inclusive: windows lo - 1 .. hi - span
        if hi - span >= lo - 1:
            ok[max(lo - 1, 0):hi - span + 1] = True
    return ok


def _hits_of(canon, gen, win, strand, rule, want):
    """runs of identical mers of a table sorted by (mer, genome, window) -> seed hits"""
    out = []
    if len(canon) == 0:
        return out
    cut = np.flatnonzero(np.concatenate(([True], canon[1:] != canon[:-1], [True])))
    for i in np.flatnonzero(np.diff(cut) >= 2):
        a, b = int(cut[i]), int(cut[i + 1])
        g = gen[a:b].tolist()
        count = {}
        for x in g:
            count[x] = count.get(x, 0) + 1
        if rule == MEM and any(v > 1 for v in count.values()):
            continue
        comps = tuple(sorted(x for x, v in count.items() if v == 1))
        if len(comps) < 2:
            continue
        m = sum(1 << x for x in comps)
        if want and m != want:
            continue
        where = {x: a + k for k, x in enumerate(g)}
        out.append((m, comps, tuple(int(win[where[x]]) for x in comps), tuple(int(strand[where[x]]) for x in comps)))
    return out


def canonical_key(length, start):
    first = next(i for i, s in enumerate(start) if s)
    return (first, abs(start[first]), sum(1 << i for i, s in enumerate(start) if s), tuple(start), length)


def find(genomes, pattern, mode=MEM, mask=0, extend=True, valid=None):
    offs, span = shape(pattern)
    N = len(genomes)
    FR = [window_mers(g, pattern) for g in genomes]
    ok = [window_ok(len(genomes[g]), span, None if valid is None else valid[g]) for g in range(N)]
    canon = [np.minimum(F, R) for F, R in FR]
    strand = [(R < F).astype(np.uint8) for F, R in FR]
    tc = np.concatenate([canon[g][ok[g]] for g in range(N)]) if N else np.zeros(0, np.uint64)
    tg = np.concatenate([np.full(int(ok[g].sum()), g, np.int64) for g in range(N)]) if N else np.zeros(0, np.int64)
    tw = np.concatenate([np.flatnonzero(ok[g]) for g in range(N)]) if N else np.zeros(0, np.int64)
    ts = np.concatenate([strand[g][ok[g]] for g in range(N)]) if N else np.zeros(0, np.uint8)
    order = np.lexsort((tw, tg, tc))
    tc, tg, tw, ts = tc[order], tg[order], tw[order], ts[order]
    if mode == PAIRWISE:
        hits = []
        for i in range(N):
            for j in range(i + 1, N):
                sel = (tg == i) | (tg == j)
                hits += _hits_of(tc[sel], tg[sel], tw[sel], ts[sel], MEM, 0)
    else:
        hits = _hits_of(tc, tg, tw, ts, mode, mask)

    diagonals = {}
    for m, comps, wins, strands in hits:
        diag = tuple((strands[k] ^ strands[0], wins[k] + wins[0] if strands[k] ^ strands[0] else wins[k] - wins[0]) for k in range(len(comps)))
        diagonals.setdefault((m, comps, diag), []).append(wins[0])
    found = []
    for (m, comps, diag), anchors in diagonals.items():
        a = comps[0]
        anchors = sorted(anchors)
        nwa = len(ok[a])
        if not extend:
            clusters = [(q, q, [q]) for q in anchors]
            agree = np.zeros(nwa, bool)
            agree[anchors] = True
        else:
            q = np.arange(nwa, dtype=np.int64)
            agree = ok[a].copy()
            for c, (rev, d) in zip(comps[1:], diag[1:]):
                qc = d - q if rev else d + q
                inside = (qc >= 0) & (qc < len(ok[c]))
                qs = np.where(inside, qc, 0)
                other = FR[c][1] if rev else FR[c][0]
                if len(other) == 0:
                    agree[:] = False
                    break
                agree &= inside & ok[c][qs] & (FR[a][0] == other[qs])
            on = np.flatnonzero(agree)
            gaps = np.flatnonzero(np.diff(on) > span)
            los = on[np.concatenate(([0], gaps + 1))] if len(on) else []
            his = on[np.concatenate((gaps, [len(on) - 1]))] if len(on) else []
            clusters = []
            for lo, hi in zip(los, his):
                inside = [x for x in anchors if lo <= x <= hi]
                if inside:
                    clusters.append((int(lo), int(hi), inside))
        for qlo, qhi, inside in clusters:
            start = [0] * N
            for c, (rev, d) in zip(comps, diag):
                start[c] = -(d - qhi + 1) if rev else d + qlo + 1
            pad = np.zeros(qhi - qlo + 1 + 2 * span, bool)
            lo, hi = max(qlo - span, 0), min(qhi + span + 1, nwa)
            pad[lo - (qlo - span):hi - (qlo - span)] = agree[lo:hi]
            found.append({"length": qhi - qlo + span, "start": start, "mask": m, "comps": comps, "diag": diag, "qlo": qlo, "qhi": qhi,
                          "hits": inside, "agree": pad, "agree_from": qlo - span, "diagonal": agree})
    found.sort(key=lambda f: canonical_key(f["length"], f["start"]))
    return {"length": [f["length"] for f in found], "start": [f["start"] for f in found], "matches": found, "hits": hits,
            "canon": canon, "strand": strand, "ok": ok, "table": (tc, tg, tw, ts), "span": span, "weight": len(offs)}


def as_set(ref):
    return {(l, tuple(s)) for l, s in zip(ref["length"], ref["start"])}
