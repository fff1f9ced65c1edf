"""The backbone / island rule a third time, from the text of that section alone: plain Python and numpy, nothing of the
library or of the oracle is called, and nothing of their structure is shared -- no chunks, no records, no sweep over region ends.

Per interval and per pair a < b of its genomes the columns are typed (both / only a / only b; neither-columns are left out) and the
typed sequence is run-length encoded: a stretch of equal one-sided type is a gap run (its length counts the one-sided columns only, the
skipped neither-columns lengthen its span, not its count), it is an island above `island_gap`; the runs between two both-stretches are
one gap region, open when it holds an island or has no both-column in front (leading) or behind (trailing).  The open regions are
painted into a (pair, column) table; wherever that table's column differs from the one before, the components of the joined pairs are
made anew by union-find, and a segment is a component that stays from one such column to the next.  Coordinates come from per-genome
prefix counts.

backbone(...) returns the seven tables of mauve_backbone_fetch (same dtypes and shapes as oracle.pyoracle.backbone) and, under "facts",
what the liveness checks of tests/test_backbone_planted_cpu.py read: per (interval, a, b) the regions (first, last, open, why) and the
runs (who, first, last, n, island)."""
import numpy as np

KEYS = ("seg_iv", "seg_col", "seg_len", "seg_mask", "seg_left", "seg_right", "islands")


def pair_walk(m, a, b, island_gap):
    """the pair's gap runs and gap regions in the columns m of one interval -> (runs, regions), both in column order"""
    kind = ((m >> np.uint32(a)) & 1).astype(np.int8) | (((m >> np.uint32(b)) & 1) << 1).astype(np.int8)
    at = np.flatnonzero(kind)                                 # neither-columns are skipped
    runs, regions = [], []
    if len(at) == 0:
        return runs, regions
    kind = kind[at]
    cut = np.flatnonzero(kind[1:] != kind[:-1]) + 1
    start = np.concatenate([[0], cut])
    stop = np.concatenate([cut, [len(kind)]])
    region, seen_both = None, False
    for k, s, e in zip(kind[start].tolist(), start.tolist(), stop.tolist()):
        if k == 3:
            if region is not None:
                regions.append(region)
                region = None
            seen_both = True
            continue
        run = {"who": a if k == 1 else b, "first": int(at[s]), "last": int(at[e - 1]), "n": e - s, "island": e - s > island_gap}
        runs.append(run)
        if region is None:
            region = {"first": run["first"], "why": set() if seen_both else {"leading"}}
        region["last"] = run["last"]
        if run["island"]:
            region["why"].add("island")
    if region is not None:                                    # no both-column behind it
        region["why"].add("trailing")
        regions.append(region)
    for r in regions:
        r["open"] = bool(r["why"])
        r["why"] = tuple(sorted(r["why"]))
    return runs, regions


def _components(S, joined):
    """genome sets (bit masks, two genomes or more) that the joined pairs connect"""
    parent = {g: g for g in S}

    def find(g):
        while parent[g] != g:
            parent[g] = parent[parent[g]]
            g = parent[g]
        return g
    for a, b in joined:
        parent[find(a)] = find(b)
    sets = {}
    for g in S:
        sets[find(g)] = sets.get(find(g), 0) | 1 << g
    return [v for v in sets.values() if v & (v - 1)]


def _signed(lo, hi, rev, k1, k2):
    """the ends of the residues k1 .. k2 (counted from the interval's first column) of a genome lying at lo .. hi"""
    return (-(hi - k2), -(hi - k1)) if rev else (lo + k1, lo + k2)


def backbone(left, right, reverse, col_off, cols, island_gap=20):
    left, right, reverse = np.asarray(left, np.int64), np.asarray(right, np.int64), np.asarray(reverse, np.int64)
    col_off, cols = np.asarray(col_off, np.int64), np.asarray(cols, np.uint32)
    n_iv, N = left.shape
    segs, islands, facts = [], [], {}
    for iv in range(n_iv):
        m = cols[col_off[iv]:col_off[iv + 1]]
        nc = len(m)
        S = [g for g in range(N) if left[iv, g]]
        if len(S) < 2 or nc == 0:
            continue
        prefix = {g: np.concatenate([[0], np.cumsum((m >> np.uint32(g)) & 1, dtype=np.int64)]) for g in S}
        pairs = [(a, b) for i, a in enumerate(S) for b in S[i + 1:]]
        is_open = np.zeros((len(pairs), nc), bool)
        for p, (a, b) in enumerate(pairs):
            runs, regions = pair_walk(m, a, b, island_gap)
            facts[(iv, a, b)] = {"runs": runs, "regions": regions}
            for r in regions:
                if r["open"]:
                    is_open[p, r["first"]:r["last"] + 1] = True
            for r in runs:
                if r["island"]:
                    g = r["who"]
                    k1, k2 = int(prefix[g][r["first"]]), int(prefix[g][r["last"] + 1]) - 1
                    islands.append((iv, a, b, g, r["first"], r["last"]) + _signed(int(left[iv, g]), int(right[iv, g]), reverse[iv, g], k1, k2))
        # columns where some pair's state differs from the column before: only there can the components change
        anew = [0] + (np.flatnonzero((is_open[:, 1:] != is_open[:, :-1]).any(axis=0)) + 1).tolist() + [nc]
        live = {}                                             # component -> its first column
        for c in anew:
            now = _components(S, [pq for p, pq in enumerate(pairs) if not is_open[p, c]]) if c < nc else []
            for comp in [k for k in live if k not in now]:
                c0 = live.pop(comp)
                have = [g for g in S if comp >> g & 1 and prefix[g][c] > prefix[g][c0]]
                if len(have) < 2:
                    continue
                lo, hi = [0] * N, [0] * N
                for g in have:
                    lo[g], hi[g] = _signed(int(left[iv, g]), int(right[iv, g]), reverse[iv, g], int(prefix[g][c0]), int(prefix[g][c]) - 1)
                segs.append((iv, c0, sum(1 << g for g in have), c - c0, lo, hi))
            for comp in now:
                live.setdefault(comp, c)
    segs.sort(key=lambda s: s[:3])                            # interval, first column, genome set
    n = len(segs)
    return {
        "seg_iv": np.array([s[0] for s in segs], np.int64), "seg_col": np.array([s[1] for s in segs], np.int64),
        "seg_len": np.array([s[3] for s in segs], np.int64), "seg_mask": np.array([s[2] for s in segs], np.uint32),
        "seg_left": np.array([s[4] for s in segs], np.int64).reshape(n, N), "seg_right": np.array([s[5] for s in segs], np.int64).reshape(n, N),
        "islands": np.array(islands, np.int64).reshape(len(islands), 8),     # in the order (interval, a, b, first column)
        "facts": facts,
    }


def first_difference(r, e):
    """None when the seven tables of r are those of e, shapes and dtypes included; else a line that says where they part"""
    for k in KEYS:
        if r[k].shape != e[k].shape or r[k].dtype != e[k].dtype:
            return "%s: shape %r %s, expected %r %s" % (k, r[k].shape, r[k].dtype, e[k].shape, e[k].dtype)
        if not np.array_equal(r[k], e[k]):
            at = tuple(np.argwhere(r[k] != e[k])[0].tolist())
            return "%s: first difference at %r: got %r, expected %r" % (k, list(at), r[k][at].tolist(), e[k][at].tolist())
    return None


def masks_at(r, iv, col):
    """the genome sets of the segments that hold column `col` of interval `iv`, ascending"""
    k = (r["seg_iv"] == iv) & (r["seg_col"] <= col) & (col < r["seg_col"] + r["seg_len"])
    return sorted(r["seg_mask"][k].tolist())
