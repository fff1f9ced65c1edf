"""DESIGN.md S5 restated from its text in plain Python integers: the canonical order of a caller's N-way list, EliminateOverlaps
over the whole list, the LCB nodes and the greedy breakpoint elimination.  No clusters, no tiles, no scans: every pass sorts the
whole list and walks it.  A third statement beside the oracle (oracle/mauve_oracle.c) and the product (chain_host.cpp,
chain_dev.hip), for tests/test_chain_cpu.py and tests/test_gpu_chains.py.

A match is (length, starts): `starts` are signed 1-based, a negative start is a reverse component whose left end is |start|.
A match's columns are numbered along its own direction: a forward component shows column 0 at its left end, a reverse component
shows its LAST column there.

input_facts() describes a list AS GIVEN (orders, overlap clusters); the tests assert from it that a planted case is where it was
meant to be, never from anything the product reports."""


def canonical_order(length, start):
    """permutation of a caller's list into canonical order: |start 0|, the signed starts, the length; the index decides among
    equal records (pipeline.cpp, "the caller's list"; canon_less of host_chain.hpp)"""
    return sorted(range(len(length)), key=lambda i: (abs(int(start[i][0])), tuple(int(x) for x in start[i]), int(length[i]), i))


def canonicalise(length, start):
    p = canonical_order(length, start)
    return [int(length[i]) for i in p], [[int(x) for x in start[i]] for i in p]


def eliminate_overlaps(length, start):
    """-> dict: length / start of the survivors in canonical order of their current records, orig (their indices in the list as
    given), passes[g] (passes of genome g that found an overlap), dead (indices), cropped (indices of survivors that lost columns),
    reordered (the survivors, taken in list order, are no longer ordered along genome 0)"""
    n = len(length)
    N = len(start[0]) if n else 0
    ln = [int(x) for x in length]
    st = [[int(x) for x in r] for r in start]
    alive = [True] * n
    passes = [0] * N
    for g in range(N):
        while True:
            order = sorted((i for i in range(n) if alive[i]), key=lambda i: (abs(st[i][g]), i))
            first = {}                                   # columns asked from a match's first / last column side
            last = {}
            for a, b in zip(order, order[1:]):
                ov = abs(st[a][g]) + ln[a] - abs(st[b][g])
                if ov <= 0:
                    continue
                if ln[a] < ln[b]:                        # a is shorter: it gives on its right side in g
                    side = last if st[a][g] > 0 else first
                    assert a not in side
                    side[a] = ov
                else:                                    # b is shorter, or as long: it gives on its left side in g
                    side = first if st[b][g] > 0 else last
                    assert b not in side
                    side[b] = ov
            if not first and not last:
                break
            passes[g] += 1
            for i in set(first) | set(last):
                cf, cl = first.get(i, 0), last.get(i, 0)
                if cf + cl >= ln[i]:
                    alive[i] = False
                    continue
                ln[i] -= cf + cl
                # the first cf columns leave: a forward component's left end moves right by cf, a reverse component's left end
                # is where its last columns are and moves right by cl
                st[i] = [s + cf if s > 0 else s - cl for s in st[i]]
    surv = [i for i in range(n) if alive[i]]
    reordered = any(abs(st[a][0]) >= abs(st[b][0]) for a, b in zip(surv, surv[1:]))
    surv.sort(key=lambda i: (abs(st[i][0]), tuple(st[i]), ln[i], i))
    return {"length": [ln[i] for i in surv], "start": [st[i] for i in surv], "orig": surv, "passes": passes,
            "dead": [i for i in range(n) if not alive[i]],
            "cropped": [i for i in surv if ln[i] != int(length[i])], "reordered": reordered}


def _runs(ln, st, orders, alive, N):
    """maximal collinear runs of the alive matches in genome-0 order -> list of runs (lists of match indices)"""
    pos = []
    for g in range(N):
        p, r = {}, 0
        for i in orders[g]:
            if alive[i]:
                p[i] = r
                r += 1
        pos.append(p)
    runs, prev = [], None
    for i in orders[0]:
        if not alive[i]:
            continue
        join = prev is not None
        for g in range(1, N):
            if not join:
                break
            if (st[i][g] < 0) != (st[prev][g] < 0):
                join = False
            elif st[i][g] > 0:
                join = pos[g][i] == pos[g][prev] + 1     # forward: the next one in that genome
            else:
                join = pos[g][i] == pos[g][prev] - 1     # reverse: the previous one
        if join:
            runs[-1].append(i)
        else:
            runs.append([i])
        prev = i
    return runs


def _orders(ln, st, N):
    n = len(ln)
    return [sorted(range(n), key=lambda i: (abs(st[i][g]), i)) for g in range(N)]


def lcb_nodes(length, start):
    """the LCB nodes before any greedy step -> list of dicts: matches, weight (sum of length * N), orient (bit g: reverse in g),
    prev[g] / next[g] (node before / behind it in genome g's order, -1 for none)"""
    ln = [int(x) for x in length]
    st = [[int(x) for x in r] for r in start]
    N = len(st[0])
    orders = _orders(ln, st, N)
    runs = _runs(ln, st, orders, [True] * len(ln), N)
    of = {i: k for k, r in enumerate(runs) for i in r}
    nodes = [{"matches": r, "weight": sum(ln[i] for i in r) * N, "orient": sum(1 << g for g in range(N) if st[r[0]][g] < 0),
              "prev": [-1] * N, "next": [-1] * N} for r in runs]
    for g in range(N):
        seq = []
        for i in orders[g]:
            if not seq or seq[-1] != of[i]:
                seq.append(of[i])
        assert len(seq) == len(runs)                      # a node's matches are contiguous in every genome
        for a, b in zip(seq, seq[1:]):
            nodes[a]["next"][g] = b
            nodes[b]["prev"][g] = a
    return nodes


def compute_lcbs(length, start, min_weight, collinear=False):
    """the greedy step on an overlap-free list -> dict like the oracle's compute_lcbs, plus n_nodes (LCBs before the first
    deletion), removed (LCBs deleted) and merged (pairs that re-merged: n_nodes - removed - n_lcb)"""
    ln = [int(x) for x in length]
    st = [[int(x) for x in r] for r in start]
    n = len(ln)
    N = len(st[0])
    orders = _orders(ln, st, N)
    alive = [True] * n
    n_nodes, removed = None, 0
    while True:
        runs = _runs(ln, st, orders, alive, N)
        if n_nodes is None:
            n_nodes = len(runs)
        if not runs:
            break
        w = [sum(ln[i] for i in r) * N for r in runs]
        best = min(range(len(runs)), key=lambda k: (w[k], k))        # the lightest, first in genome-0 order on ties
        if (len(runs) <= 1) if collinear else (w[best] >= min_weight):
            break
        for i in runs[best]:
            alive[i] = False
        removed += 1
    K = len(runs)
    match_lcb = [-1] * n
    for k, r in enumerate(runs):
        for i in r:
            match_lcb[i] = k
    left = [[0] * N for _ in range(K)]
    right = [[0] * N for _ in range(K)]
    for k, r in enumerate(runs):
        for g in range(N):
            lo = min(abs(st[i][g]) for i in r)
            hi = max(abs(st[i][g]) + ln[i] - 1 for i in r)
            sg = -1 if st[r[0]][g] < 0 else 1
            left[k][g], right[k][g] = sg * lo, sg * hi
    ladj = [[-1] * N for _ in range(K)]
    radj = [[-1] * N for _ in range(K)]
    for g in range(N):
        seq = []
        for i in orders[g]:
            k = match_lcb[i]
            if k >= 0 and (not seq or seq[-1] != k):
                seq.append(k)
        for a, b in zip(seq, seq[1:]):
            radj[a][g] = b
            ladj[b][g] = a
    return {"n_lcb": K, "match_lcb": match_lcb, "weight": [sum(ln[i] for i in r) * N for r in runs], "left_end": left,
            "right_end": right, "left_adj": ladj, "right_adj": radj, "n_nodes": n_nodes, "removed": removed,
            "merged": n_nodes - removed - K}


def chain(length, start, min_weight, collinear=False):
    """what Aligner::align's chaining stage leaves of a caller's list: anchors in chain order (LCB by LCB, genome-0 order inside)
    and the LCB table -> dict with anchor_length, anchor_start, anchor_lcb, lcb_weight, lcb_left, lcb_right, elim, lcbs"""
    cl, cs = canonicalise(length, start)
    e = eliminate_overlaps(cl, cs)
    lc = compute_lcbs(e["length"], e["start"], min_weight, collinear)
    keep = sorted((i for i in range(len(e["length"])) if lc["match_lcb"][i] >= 0), key=lambda i: (lc["match_lcb"][i], i))
    return {"anchor_length": [e["length"][i] for i in keep], "anchor_start": [e["start"][i] for i in keep],
            "anchor_lcb": [lc["match_lcb"][i] for i in keep], "lcb_weight": lc["weight"], "lcb_left": lc["left_end"],
            "lcb_right": lc["right_end"], "elim": e, "lcbs": lc}


def input_facts(length, start):
    """Facts about a list as given, per genome g: order[g] (indices by (left end, index)), clusters[g] = list of (first order
    position, size) -- the order cut wherever the running maximum of the right ends is below the next left end."""
    n = len(length)
    N = len(start[0])
    orders, clusters = [], []
    for g in range(N):
        o = sorted(range(n), key=lambda i: (abs(int(start[i][g])), i))
        cl, run = [], 0
        for k, i in enumerate(o):
            le = abs(int(start[i][g]))
            if k == 0 or run < le:
                cl.append([k, 0])
            cl[-1][1] += 1
            run = max(run, le + int(length[i]) - 1)
        orders.append(o)
        clusters.append([tuple(c) for c in cl])
    return {"order": orders, "clusters": clusters}


def cluster_at(facts, g, pos):
    """(first position, size) of the cluster of genome g that holds order position pos"""
    for a, s in facts["clusters"][g]:
        if a <= pos < a + s:
            return a, s
    raise IndexError(pos)
