"""DESIGN.md S10 (the LCB extension) restated from its text at match level, in plain Python integers: no units, no virtual
genomes, no incremental merges.  A round takes the complement of the LCB extents per genome, keeps the pieces at least one seed
long, searches them with tests/seed_ref.py (MEM, all genomes, windows inside one piece), puts what it finds next to the surviving
anchors, runs the whole elimination and the whole LCB computation of tests/chain_ref.py again, and keeps the result iff the
anchored columns grew.  A third statement beside the oracle (oracle/mauve_oracle.c: orc_align_ex) and the product
(csrc/pipeline.cpp: extend_lcbs, csrc/extend_dev.hip), for tests/test_extend_cpu.py and tests/test_gpu_extension.py.

extend() returns the final anchors in chain order, the LCB table and one record per round; layout() gives the virtual genomes
that the text prescribes for a round's pieces (piece after piece, one separator base between two of them, none behind the
last); rec_gaps() counts the inter-anchor gaps S8 would look at."""
from tests import chain_ref as C, seed_ref as S


def pieces_of(extents, length, span):
    """the complement of the union of (lo, hi) extents (1-based, inclusive) in 1 .. length, pieces of >= span bases, as
    (start, length)"""
    out, cur = [], 1
    for lo, hi in sorted(extents) + [(length + 1, length + 1)]:
        if lo - cur >= span:
            out.append((cur, lo - cur))
        cur = max(cur, hi + 1)
    return out


def layout(pieces):
    """S10's virtual genome of one genome's pieces -> dict: vstart (0-based virtual start of every piece), sep (0-based virtual
    positions of the separator bases), total (virtual length)"""
    vstart, sep, tot = [], [], 0
    for k, (_, ln) in enumerate(pieces):
        vstart.append(tot)
        tot += ln
        if k + 1 < len(pieces):
            sep.append(tot)
            tot += 1
    return {"vstart": vstart, "sep": sep, "total": tot}


def _clip(pieces, clean):
    """pieces as 1-based inclusive intervals, cut to the clean stretches (contigs cut at ambiguous bases) when there are any"""
    iv = [(a, a + n - 1) for a, n in pieces]
    if clean is None:
        return iv
    return [(max(a, lo), min(b, hi)) for a, b in iv for lo, hi in clean if max(a, lo) <= min(b, hi)]


def _extents(ln, st, lcb, n_lcb, N):
    ext = [[None] * N for _ in range(n_lcb)]
    for l, s, k in zip(ln, st, lcb):
        for g in range(N):
            a, b = abs(s[g]), abs(s[g]) + l - 1
            e = ext[k][g]
            ext[k][g] = (a, b) if e is None else (min(e[0], a), max(e[1], b))
    return ext


def root_chain(length, start, min_weight, collinear=False):
    """S5 on the root pass's N-way list -> (anchor lengths, starts, LCB ids) of the survivors in canonical order, n_lcb"""
    cl, cs = C.canonicalise(length, start)
    e = C.eliminate_overlaps(cl, cs)
    lc = C.compute_lcbs(e["length"], e["start"], min_weight, collinear) if e["length"] else {"match_lcb": [], "n_lcb": 0}
    keep = [i for i in range(len(e["length"])) if lc["match_lcb"][i] >= 0]
    return [e["length"][i] for i in keep], [e["start"][i] for i in keep], [lc["match_lcb"][i] for i in keep], lc["n_lcb"]


def extend(genomes, root_length, root_start, pattern_of, seed_weight, lcb_weight=-1, max_extension_iters=4, collinear=False,
           clean=None):
    """genomes: uint8 code arrays; root_length / root_start: the root pass's N-way list; pattern_of(weight) -> the rank-0 seed of
    that weight (0: none); lcb_weight < 0: 3 * seed_weight * N; clean: None, or per genome the 1-based inclusive intervals a window
    must lie in beyond the pieces (contigs cut at ambiguous bases).
    -> dict: anchor_length, anchor_start, anchor_lcb (chain order), lcb_weight, lcb_left, lcb_right, n_lcb, root (the same four
    anchor fields and n_lcb before the first round), rounds (one dict per round entered: weight, span, pattern, pieces[g] as (start,
    length), starved (the genomes without a piece: the rounds end), layout[g], extents (of the LCBs the round met), anchors_before,
    new (the matches found, as found), new_elim (after the elimination among them alone), fate (per new match that survived the
    elimination: found, length / start after the crops, lcb, old = the old LCBs whose anchors share that LCB, how = dropped | new |
    joined | bridged), cols_before / cols_after, kept / dropped, lcb_before / lcb_after, lcb_rechained (the LCB count of the
    recomputation, kept or not), old_died (old anchors that are not in the recomputed LCBs))"""
    N = len(genomes)
    lens = [len(g) for g in genomes]
    minw = lcb_weight if lcb_weight >= 0 else 3 * seed_weight * N
    ln, st, lcb, n_lcb = root_chain(root_length, root_start, minw, collinear)
    root = {"anchor_length": list(ln), "anchor_start": [list(s) for s in st], "anchor_lcb": list(lcb), "n_lcb": n_lcb}
    rounds, w = [], seed_weight
    for it in range(max_extension_iters):
        w -= 2
        if w < 5:
            break
        pat = pattern_of(w)
        if not pat:
            break
        span = S.shape(pat)[1]
        ext = _extents(ln, st, lcb, n_lcb, N)
        pieces = [pieces_of([ext[k][g] for k in range(n_lcb)], lens[g], span) for g in range(N)]
        rec = {"round": it, "weight": w, "span": span, "pattern": pat, "pieces": pieces, "starved": [g for g in range(N) if not pieces[g]],
               "layout": [layout(p) for p in pieces], "lcb_before": n_lcb, "lcb_after": n_lcb, "new": [], "new_elim": [], "kept": False,
               "dropped": False, "cols_before": sum(ln), "cols_after": sum(ln), "fate": [], "old_died": 0, "extents": ext,
               "lcb_rechained": n_lcb, "anchors_before": {"anchor_length": list(ln), "anchor_start": [list(s) for s in st], "anchor_lcb": list(lcb)}}
        rounds.append(rec)
        if rec["starved"]:
            break
        valid = [_clip(pieces[g], None if clean is None else clean[g]) for g in range(N)]
        f = S.find(genomes, pat, S.MEM, (1 << N) - 1, True, valid)
        new = list(zip(f["length"], [list(s) for s in f["start"]]))
        rec["new"] = new
        if not new:
            continue
        en = C.eliminate_overlaps(*C.canonicalise([l for l, _ in new], [s for _, s in new]))
        rec["new_elim"] = list(zip(en["length"], en["start"]))
        al, as_ = ln + [l for l, _ in new], st + [s for _, s in new]
        perm = C.canonical_order(al, as_)
        e = C.eliminate_overlaps([al[i] for i in perm], [as_[i] for i in perm])
        lc = C.compute_lcbs(e["length"], e["start"], minw, collinear)
        src = [perm[i] for i in e["orig"]]                       # survivor -> index in anchors + new
        keep = [i for i in range(len(src)) if lc["match_lcb"][i] >= 0]
        rec["cols_after"] = sum(e["length"][i] for i in keep)
        rec["lcb_rechained"] = lc["n_lcb"]
        old_alive = sum(1 for i in keep if src[i] < len(ln))
        rec["old_died"] = len(ln) - old_alive
        olds = {}                                                 # new LCB -> the old LCBs whose anchors it holds
        for i in keep:
            if src[i] < len(ln):
                olds.setdefault(lc["match_lcb"][i], set()).add(lcb[src[i]])
        for i in range(len(src)):
            if src[i] >= len(ln):
                k = lc["match_lcb"][i]
                rec["fate"].append({"length": e["length"][i], "start": e["start"][i], "found": new[src[i] - len(ln)], "lcb": k,
                                    "old": sorted(olds.get(k, ())) if k >= 0 else [],
                                    "how": "dropped" if k < 0 else ("new", "joined", "bridged")[min(len(olds.get(k, ())), 2)]})
        if rec["cols_after"] > rec["cols_before"]:
            rec["kept"] = True
            rec["lcb_after"] = lc["n_lcb"]
            ln, st, lcb, n_lcb = [e["length"][i] for i in keep], [e["start"][i] for i in keep], [lc["match_lcb"][i] for i in keep], lc["n_lcb"]
        else:
            rec["dropped"] = True
            rec["cols_after_dropped"], rec["cols_after"] = rec["cols_after"], rec["cols_before"]
    order = sorted(range(len(ln)), key=lambda i: (lcb[i], i))
    ext = _extents(ln, st, lcb, n_lcb, N)
    first = {}
    for i in order:
        first.setdefault(lcb[i], i)
    sign = [[-1 if st[first[k]][g] < 0 else 1 for g in range(N)] for k in range(n_lcb)]
    return {"anchor_length": [ln[i] for i in order], "anchor_start": [st[i] for i in order], "anchor_lcb": [lcb[i] for i in order],
            "n_lcb": n_lcb, "lcb_weight": [sum(ln[i] for i in order if lcb[i] == k) * N for k in range(n_lcb)],
            "lcb_left": [[sign[k][g] * ext[k][g][0] for g in range(N)] for k in range(n_lcb)],
            "lcb_right": [[sign[k][g] * ext[k][g][1] for g in range(N)] for k in range(n_lcb)], "root": root, "rounds": rounds}


def rec_gaps(length, start, lcb, min_gap):
    """S8: the gaps between consecutive anchors of one LCB (chain order) whose longest side exceeds min_gap -> [(index of the
    anchor in front, longest side)]"""
    out = []
    for j in range(len(length) - 1):
        if lcb[j] != lcb[j + 1]:
            continue
        mx = 0
        for sa, sb in zip(start[j], start[j + 1]):
            lo, hi = (sa + length[j], sb - 1) if sa > 0 else (-sb + length[j + 1], -sa - 1)
            mx = max(mx, hi - lo + 1)
        if mx > min_gap:
            out.append((j, mx))
    return out
