"""DESIGN.md S9 (guide tree, the walk's structural rules), S11b / S11c (distance factors, breakpoint counts) and S13 (refinement of one
interval) restated from the text in Python integers and numpy.  Nothing here shares code with oracle/ or with the library; the seed
rule comes from tests/seed_ref.py, the DP and the sum-of-pairs objective from tests/dp_ref.py.

Every rule that the text settles by a tie-break or a rounding has a switch that states it wrongly (`wrong=`): the CPU tests run the
planted cases through those too and require a different answer, so a case that does not reach its rule shows up there."""
import numpy as np

from tests import dp_ref as D
from tests import seed_ref as SR

PPM = 1000000


def pair_records(genomes, pattern):
    """the pairwise matches of every genome pair (S9: PairwiseMatchFinder rule, root seed) -> [(length, signed 1-based starts)]"""
    f = SR.find(genomes, pattern, mode=SR.PAIRWISE)
    return [(int(l), tuple(int(x) for x in s)) for l, s in zip(f["length"], f["start"])]


def distances(genomes, records, wrong=None):
    """S9: similarity(i, j) = sum of the match lengths / min(L_i, L_j); distance = 10^6 - min(10^6, floor(10^6 sim)).  wrong: 'longer' (the
    longer genome divides)"""
    N = len(genomes)
    S = [[0] * N for _ in range(N)]
    for ln, st in records:
        a, b = [g for g in range(N) if st[g]]
        S[a][b] += ln
        S[b][a] += ln
    dist = np.zeros((N, N), np.int64)
    for i in range(N):
        for j in range(N):
            if i != j:
                mn = (max if wrong == "longer" else min)(len(genomes[i]), len(genomes[j]))
                dist[i, j] = PPM - min(PPM, PPM * S[i][j] // mn) if mn else PPM
    return dist


def upgma(dist, wrong=None):
    """S9: merge the closest pair of clusters, ties to the lowest ids; the new cluster is N, N + 1, ...; the left child is the lower id;
    d(new, x) = floor((|a| d(a, x) + |b| d(b, x)) / (|a| + |b|)).  wrong: 'ties_high' (ties go to the highest ids), 'round' (the mean is
    rounded to nearest)"""
    N = len(dist)
    M = 2 * N - 1
    d = {(i, j): int(dist[i][j]) for i in range(N) for j in range(N) if i != j}
    size = {i: 1 for i in range(N)}
    left, right = [-1] * M, [-1] * M
    for k in range(N, M):
        ids = sorted(size)
        pairs = [(d[a, b], a, b) for x, a in enumerate(ids) for b in ids[x + 1:]]
        low = min(p[0] for p in pairs)
        tied = [(a, b) for v, a, b in pairs if v == low]
        a, b = max(tied) if wrong == "ties_high" else min(tied)
        left[k], right[k] = a, b
        sa, sb = size.pop(a), size.pop(b)
        for x in size:
            num = sa * d[a, x] + sb * d[b, x]
            d[k, x] = d[x, k] = (2 * num + sa + sb) // (2 * (sa + sb)) if wrong == "round" else num // (sa + sb)
        size[k] = sa + sb
    return np.array(left, np.int32), np.array(right, np.int32)


def upgma_means(dist):
    """the (numerator, denominator) of every size-weighted mean that upgma(dist) floors, in the order it takes them"""
    N = len(dist)
    d = {(i, j): int(dist[i][j]) for i in range(N) for j in range(N) if i != j}
    size = {i: 1 for i in range(N)}
    left, right = upgma(dist)
    out = []
    for k in range(N, 2 * N - 1):
        a, b = int(left[k]), int(right[k])
        sa, sb = size.pop(a), size.pop(b)
        for x in size:
            out.append((sa * d[a, x] + sb * d[b, x], sa + sb))
            d[k, x] = d[x, k] = out[-1][0] // out[-1][1]
        size[k] = sa + sb
    return out


def bp_sorted(records, a, b, min_len, wrong=None):
    """S11c: the records of pair a < b of length >= min_len in the order of genome a, ties by (position in b, strand in b) -> [(pos a,
    pos b, reverse in b)].  wrong: 'floor_strict' (length > min_len)"""
    keep = []
    for ln, st in records:
        if st[a] and st[b] and (ln > min_len if wrong == "floor_strict" else ln >= min_len):
            keep.append((abs(st[a]), abs(st[b]), int(st[b] < 0)))
    return sorted(keep)


def breakpoint_counts(records, N, min_len, wrong=None):
    """S11c: per pair, the adjacencies of consecutive records along a that are not conserved: both on the same strand of b and the rank in b
    (order by position in b, ties by (strand, order along a)) stepping by +1 (forward) or -1 (reverse).  wrong: 'floor_strict';
    'pair_boundary' (the records of all pairs are one list in pair order, and the adjacency of the last record of one pair and the first
    of the next counts as any other: a breakpoint, since their ranks belong to different pairs); 'no_strand' (the strand is ignored: a step
    of +1 or -1 is conserved); 'steps_swapped' (-1 forward, +1 reverse)"""
    bp = np.zeros((N, N), np.int64)
    prev_pair = None
    for a in range(N):
        for b in range(a + 1, N):
            rec = bp_sorted(records, a, b, min_len, wrong)
            order_b = sorted(range(len(rec)), key=lambda i: (rec[i][1], rec[i][2], i))
            rank = [0] * len(rec)
            for r, i in enumerate(order_b):
                rank[i] = r
            broken = 0
            for i in range(len(rec) - 1):
                step, r0, r1 = rank[i + 1] - rank[i], rec[i][2], rec[i + 1][2]
                if wrong == "no_strand":
                    broken += step not in (1, -1)
                elif wrong == "steps_swapped":
                    broken += not ((r0 == 0 and r1 == 0 and step == -1) or (r0 == 1 and r1 == 1 and step == 1))
                else:
                    broken += not ((r0 == 0 and r1 == 0 and step == 1) or (r0 == 1 and r1 == 1 and step == -1))
            if wrong == "pair_boundary" and rec:
                if prev_pair is not None:
                    broken += 1
                prev_pair = (a, b)
            bp[a, b] = bp[b, a] = broken
    return bp


def bp_distance(counts):
    """S11c: d_bp(a, b) = floor(10^6 bp(a, b) / max over the pairs), 0 when no pair has a breakpoint"""
    counts = np.asarray(counts, np.int64)
    mx = int(counts.max()) if counts.size else 0
    return counts * PPM // mx if mx else np.zeros_like(counts)


def leaves(tree, node):
    left, right = tree
    if left[node] < 0:
        return [int(node)]
    return leaves(tree, int(left[node])) + leaves(tree, int(right[node]))


def node_factor(tree, node, dist, bpd, conservation_scale_ppm, bp_dist_scale_ppm=0):
    """S11b, S11c: c = floor(mean d over L x R), factor = max(0, 10^6 - floor(scale c / 10^6)); with a breakpoint scale the same from the
    breakpoint distances, and the product floor(factor f2 / 10^6)"""
    la, lb = leaves(tree, int(tree[0][node])), leaves(tree, int(tree[1][node]))
    pairs = len(la) * len(lb)
    c = sum(int(dist[a][b]) for a in la for b in lb) // pairs
    factor = max(0, PPM - conservation_scale_ppm * c // PPM)
    if bp_dist_scale_ppm > 0 and bpd is not None:
        b = sum(int(bpd[x][y]) for x in la for y in lb) // pairs
        factor = factor * max(0, PPM - bp_dist_scale_ppm * b // PPM) // PPM
    return factor


def scaled_weight(weight, factor, min_scaled_penalty=0):
    return max(min_scaled_penalty, weight * factor // PPM)


def cut_after_stretch(lens, min_recursive_gap, max_gapped_len, wrong=None):
    """S9: a piece is cut at an inter-anchor stretch that >= 2 genomes share and that either exceeds max_gapped_len or is longer than
    min_recursive_gap in at least two but not all genomes of the node.  lens: the stretch's length in every genome of the node.
    wrong: 'gap_ge' (>= min_recursive_gap), 'len_ge' (>= max_gapped_len)"""
    n = len(lens)
    if sum(1 for x in lens if x > 0) < 2:
        return False
    big = sum(1 for x in lens if (x >= min_recursive_gap if wrong == "gap_ge" else x > min_recursive_gap))
    too_long = max(lens) >= max_gapped_len if wrong == "len_ge" else max(lens) > max_gapped_len
    return too_long or 2 <= big < n


_ALIGNED = {}


def _aligned(order_seqs, S, go, ge):
    key = (tuple(bytes(bytearray(int(b) for b in s)) for s in order_seqs), tuple(tuple(r) for r in S), go, ge)
    if key not in _ALIGNED:
        _ALIGNED[key] = D.align_interval(order_seqs, S, go, ge)
    return _ALIGNED[key]


def refine_interval(seqs, rounds, S, go, ge, wrong=None):
    """S13: the interval aligned in genome order (rotation 0) and in the rotated orders r = 1 .. min(rounds, k - 1) of its k non-empty
    sequences (the leading one taken out and added back last, r times); the objective is the sum-of-pairs score of the columns; the highest
    wins, the lowest rotation on ties.  An interval with k < 3 has rotation 0 only.
    -> (columns over the slots of `seqs`, DP score of the kept alignment, winning rotation, objective of every rotation).
    wrong: 'ties_high' (the highest rotation on ties)"""
    nz = [g for g, s in enumerate(seqs) if len(s)]
    k = len(nz)
    cands = []
    for r in range(0, (min(rounds, k - 1) if k >= 3 else 0) + 1):
        order = [nz[(j + r) % k] for j in range(k)]
        cols, score = _aligned([seqs[g] for g in order], S, go, ge)
        back = [sum(1 << order[j] for j in range(k) if c >> j & 1) for c in cols]
        cands.append((back, score, D.sp_score_cols(seqs, back, S, go, ge)))
    obj = [c[2] for c in cands]
    best = max(obj)
    win = max(r for r, o in enumerate(obj) if o == best) if wrong == "ties_high" else obj.index(best)
    return np.array(cands[win][0], np.uint32), cands[win][1], win, obj


def pair_layout(cols, a, b):
    """per column of one interval, for the pair (a, b): 'B' both, 'a' / 'b' one-sided, '.' neither"""
    return "".join("B" if (c >> a & 1) and (c >> b & 1) else "a" if c >> a & 1 else "b" if c >> b & 1 else "." for c in (int(x) for x in cols))


def interval_table(res, multi_only=True):
    """the (genome set, left, right) rows of a result, as the walk cases write them out"""
    left, right = np.asarray(res["left"]), np.asarray(res["right"])
    rows = []
    for i in range(len(left)):
        gs = tuple(int(g) for g in np.flatnonzero(right[i]))
        if multi_only and len(gs) < 2:
            continue
        rows.append((gs, tuple(int(left[i][g]) for g in gs), tuple(int(right[i][g]) for g in gs)))
    return rows


def check_walk(genomes, tree, res):
    """the rules of S9 that can be read off a result: every base lies in exactly one interval; a multi-genome interval's genomes are the
    leaves of a tree node; those intervals come in pre-order of their nodes; the single-genome leftovers come after them, genome by genome,
    in position order; per interval and genome the column bits number right - left + 1"""
    N = len(genomes)
    left, right, col_off, cols = np.asarray(res["left"]), np.asarray(res["right"]), np.asarray(res["col_off"]), np.asarray(res["cols"])
    n_iv = len(left)
    assert col_off[0] == 0 and col_off[n_iv] == len(cols) and np.all(np.diff(col_off) >= 0)
    cover = [np.zeros(len(g) + 2, np.int64) for g in genomes]
    root = 2 * N - 2
    pre, stack = [], [root]
    while stack:
        v = stack.pop()
        if tree[0][v] >= 0:
            pre.append(v)
            stack += [int(tree[1][v]), int(tree[0][v])]
    node_of = {tuple(sorted(leaves(tree, v))): i for i, v in enumerate(pre)}
    seen, single = -1, None
    for i in range(n_iv):
        gs = tuple(int(g) for g in np.flatnonzero(right[i]))
        assert gs, "interval %d holds no genome" % i
        c = cols[col_off[i]:col_off[i + 1]]
        assert np.all(c != 0) and not np.any(c & ~np.uint32(sum(1 << g for g in gs))), "interval %d: a column outside its genomes" % i
        for g in gs:
            lo, hi = int(left[i][g]), int(right[i][g])
            assert 1 <= lo <= hi <= len(genomes[g]), (i, g, lo, hi)
            assert int(np.count_nonzero(c >> np.uint32(g) & 1)) == hi - lo + 1, "interval %d genome %d: bits and extent differ" % (i, g)
            cover[g][lo] += 1
            cover[g][hi + 1] -= 1
        if len(gs) >= 2:
            assert single is None, "multi-genome interval %d after a leftover" % i
            assert gs in node_of, "interval %d: %s is no node of the tree" % (i, gs)
            assert node_of[gs] >= seen, "interval %d: out of pre-order" % i
            seen = node_of[gs]
        else:
            key = (gs[0], int(left[i][gs[0]]))
            assert single is None or key > single, "leftover %d out of order" % i
            single = key
    for g in range(N):
        assert np.all(np.cumsum(cover[g])[1:len(genomes[g]) + 1] == 1), "genome %d: a base in no interval or in two" % g
