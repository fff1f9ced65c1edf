"""DESIGN.md S8 (recursive anchoring) restated from its text in plain Python integers and numpy: every gap is cut out of the genomes
in LCB orientation and searched ON ITS OWN with tests/seed_ref.py -- no virtual genome, no gap ids, no segment table -- then the
all-forward N-way matches go through tests/chain_ref.py's elimination and its collinear rule, and the survivors' sub-gaps recurse
with the weight just used.  A third statement beside the oracle (oracle/mauve_oracle.c: recurse_gap) and the product
(csrc/recursive.cpp and the segmented instantiations of csrc/seed_pass.hip, csrc/chain_dev.hip), for tests/test_recursion_cpu.py and
tests/test_gpu_recursion.py.  It shares no code with either.

The gaps are visited level by level, in the order the text's work list has them: the gaps of the chains in LCB order first; behind a
level, the sub-gaps of every gap that found anchors, the gaps taken weight class by weight class (ascending) and in work-list order
inside a class, the sub-gaps of one gap from left to right in LCB orientation.  The anchors do not depend on that order; the
batches (one per level and weight) and the layout of their virtual genomes do."""
from tests import chain_ref as C, seed_ref as S


def default_weight(avg_len):
    """S2: w = ceil(log2(avg_len) / 1.5), bumped to odd, clamped to [5, 31] -- in integers: the least w with 8^w >= avg_len^2"""
    if avg_len < 2:
        return 5
    w = 0
    while 8 ** w < avg_len * avg_len:
        w += 1
    if w % 2 == 0:
        w += 1
    return min(max(w, 5), 31)


def rc(x):
    return (3 - x[::-1]).astype(x.dtype)


def gap_of(a, b, g):
    """S6: the interval between anchors a and b = (length, starts) in genome g -> (1-based left end, length, reverse?)"""
    (la, sa), (lb, sb) = a, b
    if sa[g] > 0:
        lo, hi, rev = sa[g] + la, sb[g] - 1, False
    else:
        lo, hi, rev = -sb[g] + lb, -sa[g] - 1, True
    return lo, max(hi - lo + 1, 0), rev


def _mirror(clean, lo, ln, rev):
    """the clean intervals (1-based, inclusive, real) cut to the gap lo .. lo + ln - 1 and carried into gap coordinates (mirrored when
    the genome runs backwards through the gap)"""
    hi, out = lo + ln - 1, []
    for a, b in clean:
        a, b = max(a, lo), min(b, hi)
        if a <= b:
            out.append((hi - b + 1, hi - a + 1) if rev else (a - lo + 1, b - lo + 1))
    return sorted(out)


def _real(l, s, lo, ln, rev):
    """a component of length l at s (signed, 1-based inside the gap, LCB orientation) -> its signed real start: a genome that runs
    backwards through the gap mirrors the component inside it and turns its strand"""
    left = lo + abs(s) - 1 if not rev else (lo + ln - 1) - (abs(s) - 1) - l + 1
    return left if (s > 0) != rev else -left


def search_gap(genomes, a, b, prev_w, pattern_of, span_of, min_gap, clean=None):
    """one gap between the anchors a and b (length, signed real starts) -> its record (see recurse)"""
    N = len(genomes)
    geo = [gap_of(a, b, g) for g in range(N)]
    lens = [ln for _, ln, _ in geo]
    rec = {"a": a, "b": b, "lo": [lo for lo, _, _ in geo], "lens": lens, "rev": [r for _, _, r in geo], "prev_w": prev_w, "weight": 0, "why": None,
           "matches": [], "non_forward": [], "forward": [], "elim": [], "cropped": [], "dead": [], "nodes": 0, "deleted": [], "survivors_local": [],
           "survivors": []}
    if max(lens) <= min_gap:
        rec["why"] = "short"
        return rec
    rec["raw"] = default_weight(sum(lens) // N)
    w = min(rec["raw"], prev_w - 2)
    if w < 5:
        rec["why"] = "w<5"
        return rec
    pat = pattern_of(w)
    if min(lens) < span_of(w):
        rec["why"] = "side<span"
        return rec
    rec["weight"] = w
    subs = []
    for g, (lo, ln, rev) in enumerate(geo):
        x = genomes[g][lo - 1:lo - 1 + ln]
        subs.append(rc(x) if rev else x)
    valid = None if clean is None else [_mirror(clean[g], *geo[g]) for g in range(N)]
    rec["valid"] = valid
    f = S.find(subs, pat, S.MEM, (1 << N) - 1, True, valid)
    found = list(zip(f["length"], [list(s) for s in f["start"]]))
    rec["matches"] = found
    rec["matches_real"] = [(l, [_real(l, s[g], *geo[g]) for g in range(N)]) for l, s in found]
    rec["non_forward"] = [m for m in found if min(m[1]) < 0]
    fwd = [m for m in found if min(m[1]) > 0]
    rec["forward"] = fwd
    if not fwd:
        return rec
    e = C.eliminate_overlaps(*C.canonicalise([l for l, _ in fwd], [s for _, s in fwd]))
    rec["elim"] = list(zip(e["length"], e["start"]))
    rec["cropped"], rec["dead"] = [fwd[i] for i in e["cropped"]], [fwd[i] for i in e["dead"]]
    rec["deleted"], rec["nodes"] = _collinear_deletions(e["length"], e["start"])
    lc = C.compute_lcbs(e["length"], e["start"], 0, collinear=True)
    assert lc["n_nodes"] == rec["nodes"] and lc["removed"] == len(rec["deleted"])
    loc = [(e["length"][i], e["start"][i]) for i in range(len(e["length"])) if lc["match_lcb"][i] >= 0]
    rec["survivors_local"] = loc
    rec["survivors"] = [(l, [_real(l, s[g], *geo[g]) for g in range(N)]) for l, s in loc]
    rec["survivors"].sort(key=lambda m: abs(m[1][0]))
    return rec


def _collinear_deletions(length, start):
    """the collinear rule step by step, told apart from chain_ref.compute_lcbs: the nodes deleted, in order, each as the list of its
    matches (indices into the overlap-free list), and the node count before the first deletion"""
    n, N = len(length), len(start[0])
    alive, deleted, first = [True] * n, [], None
    while True:
        nodes = C.lcb_nodes([length[i] for i in range(n) if alive[i]], [start[i] for i in range(n) if alive[i]])
        idx = [i for i in range(n) if alive[i]]
        if first is None:
            first = len(nodes)
        if len(nodes) <= 1:
            return deleted, first
        k = min(range(len(nodes)), key=lambda q: (nodes[q]["weight"], q))
        gone = [idx[i] for i in nodes[k]["matches"]]
        deleted.append({"matches": gone, "weight": nodes[k]["weight"], "tied": [q for q in range(len(nodes)) if nodes[q]["weight"] == nodes[k]["weight"]]})
        for i in gone:
            alive[i] = False


def recurse(genomes, anchors, lcb, pattern_of, span_of, root_weight, min_gap, clean=None, recursive=True):
    """genomes: uint8 code arrays; anchors: (length, signed starts) in chain order with their LCB ids `lcb`; pattern_of(weight) /
    span_of(weight): the rank-0 seed; clean: None or per genome the 1-based inclusive intervals a window must lie in.
    -> dict: anchor_length, anchor_start, anchor_lcb (chain order), records (one per gap looked at: level, index (place in the level's
    work list), lcb, a, b, lo / lens / rev per genome, prev_w, raw (the weight the mean length wants), weight (0: none, `why` = short | w<5 | side<span), matches (as found,
    N-way; matches_real: in real coordinates), non_forward, forward, elim, cropped, dead, nodes, deleted, survivors_local, survivors (real, genome-0 order)), batches ((level,
    weight) -> the records of that batch in work-list order, in the order the batches run)"""
    chains = {}
    for (l, s), k in zip(anchors, lcb):
        chains.setdefault(k, []).append((int(l), [int(x) for x in s]))
    found = {k: [] for k in chains}
    work = []
    for k in sorted(chains):
        ch = chains[k]
        assert all(abs(x[1][0]) < abs(y[1][0]) for x, y in zip(ch, ch[1:])), "chain order"
        work += [(k, root_weight, x, y) for x, y in zip(ch, ch[1:])]
    records, batches, level = [], {}, 1
    while work and recursive:
        recs = []
        for i, (k, pw, a, b) in enumerate(work):
            r = search_gap(genomes, a, b, pw, pattern_of, span_of, min_gap, clean)
            r.update(level=level, index=i, lcb=k)
            recs.append(r)
        records += recs
        nxt = []
        for w in sorted({r["weight"] for r in recs if r["weight"]}):
            batch = [r for r in recs if r["weight"] == w]
            batches[(level, w)] = batch
            for r in batch:
                sv = r["survivors"]
                if not sv:
                    continue
                # (a reverse genome 0 does not exist: genome 0 is forward in every LCB, so genome-0 order is LCB orientation)
                edge = [r["a"]] + sv + [r["b"]]
                nxt += [(r["lcb"], w, x, y) for x, y in zip(edge, edge[1:])]
                found[r["lcb"]] += sv
        work, level = nxt, level + 1
    out_l, out_s, out_k = [], [], []
    for k in sorted(chains):
        for l, s in sorted(chains[k] + found[k], key=lambda m: abs(m[1][0])):
            out_l.append(l); out_s.append(s); out_k.append(k)
    return {"anchor_length": out_l, "anchor_start": out_s, "anchor_lcb": out_k, "records": records, "batches": batches}


def virtual_layout(batch):
    """the virtual genomes the batched form prescribes for the records of one level and weight: the gaps in work-list order, one after
    the other, no separator -> per genome {"seg": 0-based virtual start of every gap, "total": virtual length}"""
    N = len(batch[0]["lens"])
    out = []
    for g in range(N):
        seg, tot = [], 0
        for r in batch:
            seg.append(tot)
            tot += r["lens"][g]
        out.append({"seg": seg, "total": tot})
    return out


def virtual_genomes(genomes, batch):
    """the bases of those virtual genomes (for the liveness runs of the CPU file: a search over them WITHOUT the segment rule)"""
    import numpy as np
    out = []
    for g in range(len(genomes)):
        parts = []
        for r in batch:
            x = genomes[g][r["lo"][g] - 1:r["lo"][g] - 1 + r["lens"][g]]
            parts.append(rc(x) if r["rev"][g] else x)
        out.append(np.concatenate(parts).astype(np.uint8))
    return out
