"""Planted match lists for the chain stage (chain_dev.hip, chain_host.cpp): tile edges of the 1024-entry tiles,
overlap clusters at the per-thread limit, workgroups whose clusters outgrow the LDS pool, ties, LCB graphs with a live greedy
step, wide lists, sort-key widths on both sides of a pass-count change, and larger random dense lists.

A case is a dict: name, N, glen (genome lengths), length[n], start[n][N] (canonical order, tests/chain_ref.py), runs (the
(lcb_weight, collinear) settings it is chained under), device (True: chain_device_graph must chain it; False: it must hand the
list back to the host chain; None: not asserted), small (the GPU test compares with the Python reference directly) and aim
(where the planted spot is, for the liveness assertions of tests/test_chain_cpu.py, which read it against
chain_ref.input_facts, never against the product).

A layout is made genome by genome: perm[g] is the order of the matches along genome g, and every entry sits `gap` bases behind
the largest right end so far (gap 1: abuts, right end = next left end - 1; gap 0: overlaps by one column) or `step` bases
behind the left end of the entry before it."""
import functools
import random

from tests import chain_ref as R

TILE = 1024
CL_MAX = 48
POOL_WORDS = 12 * 1024
WORDS_PER_ENTRY = 8
CLUSTERS_PER_WORKGROUP = 256


def layout(lens, perms, rev, over, rng, base=1):
    """starts of the matches: perms[g] their order along genome g, over[g][k] = ("gap", d) | ("step", s) for order position k
    (default: a gap of 2 .. 4 bases behind everything before it); rev[i][g] -> negative start"""
    n, N = len(lens), len(perms)
    start = [[0] * N for _ in range(n)]
    for g in range(N):
        left, reach = base, base - 1
        for k, i in enumerate(perms[g]):
            kind, v = over[g].get(k, ("gap", rng.randint(2, 4)))
            if k:
                left = reach + v if kind == "gap" else left + v
            start[i][g] = -left if rev[i][g] else left
            reach = max(reach, left + lens[i] - 1)
    return start


def _case(name, N, length, start, glen=None, runs=((0, 0),), device=None, small=False, aim=None, pad=9):
    length, start = R.canonicalise(length, start)
    ends = [max(abs(s[g]) + l - 1 for l, s in zip(length, start)) for g in range(N)]
    glen = list(glen) if glen else [e + pad + g for g, e in enumerate(ends)]
    assert all(l >= 1 for l in length) and all(abs(x) >= 1 for s in start for x in s)
    assert all(e <= gl for e, gl in zip(ends, glen)), name            # every match lies inside its genomes
    return {"name": name, "N": N, "glen": glen, "length": length, "start": start, "runs": tuple(runs), "device": device,
            "small": small, "aim": aim or {}}


def _perms(n, N, rng):
    """a different permutation of the list for every genome (genome 0: the list itself)"""
    out = [list(range(n))]
    for _ in range(1, N):
        p = list(range(n))
        rng.shuffle(p)
        out.append(p)
    return out


def _strands(n, N, rng, frac=0.4):
    return [[g > 0 and rng.random() < frac for g in range(N)] for _ in range(n)]


# ---- tile edges -----------------------------------------------------------------------------------------------------------
def tile_edge(n, N, kind, seed):
    """kind "pair": a cluster of 2 over every tile edge of every genome's order, one column overlapping; "triple": a cluster of 3;
    "abut": the two entries abut (two clusters, nothing cropped).  The last two entries of every order overlap as well: a cluster
    ends on the last entry of the list."""
    rng = random.Random(seed)
    lens = [rng.randint(3, 9) for _ in range(n)]
    perms, rev = _perms(n, N, rng), _strands(n, N, rng)
    over = [{} for _ in range(N)]
    edges = [b for b in range(TILE, n, TILE)]
    spots = []                                             # (genome, first order position, size) of the planted clusters
    for g in range(N):
        for e, b in enumerate(edges):
            if kind == "abut":
                over[g][b] = ("gap", 1)
                spots.append((g, b, None))                 # a cluster starts at b, the one before it ends at b - 1
            elif kind == "pair":
                over[g][b] = ("gap", 0)
                spots.append((g, b - 1, 2))
            else:                                          # b-2, b-1, b or b-1, b, b+1
                lo = b - 1 if (e + g) % 2 == 0 else b
                ks = [k for k in (lo, lo + 1) if k < n]
                for k in ks:
                    over[g][k] = ("gap", 0)
                spots.append((g, lo - 1, 1 + len(ks)))
        if n - 1 not in over[g] and n - 2 not in over[g]:
            over[g][n - 1] = ("gap", 0)
            spots.append((g, n - 2, 2))
    start = layout(lens, perms, rev, over, rng)
    return _case("tile_%s_n%d_N%d" % (kind, n, N), N, lens, start, device=True,
                 aim={"kind": kind, "edges": edges, "spots": spots})


def long_reach(seed=5):
    """One long match at order position 0 of genome 1 reaches past the first entries of tile 2, everything between is short: the
    largest right end of tile 1 is below tile 0's, so what tile 2 sees must come from two tiles back.  Every entry up to there is in
    the long match's cluster, which is far beyond CH_CL_MAX: the device must hand the list back, and the host chain kills them one
    pass after the other."""
    rng = random.Random(seed)
    n, N = 2 * TILE + 60, 2
    lens = [rng.randint(2, 4) for _ in range(n)]
    lens[n - 1] = 7 * (2 * TILE + 4)                       # in genome 0 it is the last entry and overlaps nobody
    perms = [list(range(n)), [n - 1] + list(range(n - 1))]
    rev = [[False, False] for _ in range(n)]
    over = [{}, {k: ("step", 7 if k > 1 else 1) for k in range(1, 2 * TILE + 4)}]
    start = layout(lens, perms, rev, over, rng)
    return _case("long_reach", N, lens, start, device=False, aim={"genome": 1, "reach": 2 * TILE + 3})


# ---- cluster sizes --------------------------------------------------------------------------------------------------------
def _with_clusters(name, N, g_aim, sizes, seed, filler=60, device=None, lo_len=6, hi_len=30, first=False, small=True):
    """clusters of exactly the given sizes in genome g_aim (chains of matches each starting inside the one before), single
    matches around them; in the other genomes the members lie apart"""
    rng = random.Random(seed)
    n = sum(sizes) + filler
    lens = [rng.randint(lo_len, hi_len) for _ in range(n)]
    rev = _strands(n, N, rng)
    perms = _perms(n, N, rng)
    over = [{} for _ in range(N)]
    k = 0 if first else filler // 2
    spots = []
    for s in sizes:
        spots.append((k, s))
        for q in range(1, s):
            over[g_aim][k + q] = ("step", rng.randint(1, lens[perms[g_aim][k + q - 1]] - 1))
        k += s + (0 if first else 1)
    start = layout(lens, perms, rev, over, rng)
    return _case(name, N, lens, start, device=device, small=small, aim={"genome": g_aim, "clusters": spots})


def cluster_sizes():
    out = [_with_clusters("cluster_%d" % s, 2, 1, [s], 100 + s, device=s <= CL_MAX) for s in (47, 48, 49)]
    out.append(_with_clusters("cluster_48_49_genome0", 3, 0, [48, 49], 151, device=False))
    out.append(_with_clusters("cluster_48_49_last_genome", 3, 2, [48, 49], 152, device=False))
    out.append(_with_clusters("cluster_48_48_genome0", 3, 0, [48, 48], 153, device=True))
    return out


def cluster_sizes_cl5():
    """for MAUVE_CH_CL_MAX=5: device is what that process must do"""
    return [_with_clusters("cl5_cluster_5", 2, 1, [5, 5, 4], 161, device=True),
            _with_clusters("cl5_cluster_5_6", 2, 1, [5, 6], 162, device=False)]


# ---- LDS pool ---------------------------------------------------------------------------------------------------------------
def pool_overflow():
    """clusters 0 .. 255 of genome 1 belong to one workgroup of ch_cluster_pass; 8 words an entry from a pool of 12 288 words"""
    a = _with_clusters("pool_300_of_7", 2, 1, [7] * 300, 171, filler=40, device=True, first=True, small=False)
    b = _with_clusters("pool_40_of_48", 2, 1, [48] * 40, 172, filler=40, device=True, first=True, lo_len=10, small=False)
    return [a, b]


def pool_demand(facts, g, cl_max=CL_MAX):
    """per workgroup of genome g: the words its clusters ask of the pool, in cluster order (a cluster of one asks nothing, one
    beyond cl_max neither)"""
    cl = facts["clusters"][g]
    return [[WORDS_PER_ENTRY * s for _, s in cl[w:w + CLUSTERS_PER_WORKGROUP] if 2 <= s <= cl_max]
            for w in range(0, len(cl), CLUSTERS_PER_WORKGROUP)]


# ---- ties -------------------------------------------------------------------------------------------------------------------
# (length, start in genome 0, start in genome 1), coordinates relative to the family's own origin; what must happen is asserted
# from the reference in tests/test_chain_cpu.py under the same name
TIE_FAMILIES = {
    "tie0_equal_length": [(10, 100, 300), (10, 100, 500)],                 # equal left ends in genome 0: the later index dies
    "tie0_second_shorter": [(10, 100, 300), (6, 100, 500)],
    "tie0_first_shorter": [(6, 100, 300), (10, 100, 500)],
    "tie1_equal_length": [(10, 100, 300), (10, 200, 300)],                 # equal left ends in genome 1 only
    "tie1_first_shorter": [(10, 100, 300), (12, 200, 300)],
    "duplicate": [(10, 100, 300), (10, 100, 300)],
    "equal_length_overlap": [(10, 100, 300), (10, 105, 400)],              # the right one gives 5 columns
    "nested": [(20, 100, 300), (5, 105, 400)],
    "both_sides_exact": [(10, 100, 300), (8, 106, 400), (10, 110, 500)],   # 4 + 4 of 8 columns: dies
    "both_sides_one_left": [(10, 100, 300), (9, 106, 400), (10, 111, 500)],   # 4 + 4 of 9 columns: one column stays
    "hidden_overlap": [(30, 100, 900), (5, 105, 310), (20, 500, 300), (20, 600, 315)],   # genome 0 kills (5, 105, 310), which lies between
                                                                                         # the overlapping pair at 300 and 315 of genome 1
}


def survivors_if_exact_deaths_lingered(length, start):
    """NOT S5 -- a wrong rule, stated on its own so that a case can be shown to tell the two apart: a match whose requests sum to
    exactly its length stays in the order with length 0 until its genome is done, instead of leaving at once (one whose requests
    exceed its length leaves as it should).  While it stays it keeps its two neighbours from meeting.  -> sorted (length, starts) of
    what is left."""
    n, N = len(length), len(start[0])
    ln, st, alive = list(length), [list(r) for r in start], [True] * n
    for g in range(N):
        while True:
            order = sorted((i for i in range(n) if alive[i]), key=lambda i: (abs(st[i][g]), i))
            ask = {}                                       # match -> [first columns, last columns]
            for a, b in zip(order, order[1:]):
                ov = abs(st[a][g]) + ln[a] - abs(st[b][g])
                if ov > 0:
                    i, left_side = (a, False) if ln[a] < ln[b] else (b, True)
                    ask.setdefault(i, [0, 0])[0 if (st[i][g] > 0) == left_side else 1] = ov
            if not ask:
                break
            for i, (cf, cl) in ask.items():
                if cf + cl > ln[i]:
                    alive[i] = False
                else:
                    ln[i] -= cf + cl
                    st[i] = [s + cf if s > 0 else s - cl for s in st[i]]
        alive = [alive[i] and ln[i] > 0 for i in range(n)]
    return sorted((ln[i], tuple(st[i])) for i in range(n) if alive[i])


@functools.lru_cache(maxsize=None)
def _searched(what, reverse=False):
    """small dense lists found by a seeded search with the reference: one whose genome 0 needs three passes or more, one in which a
    pass carries a match past its neighbour in genome 0 (S5's last paragraph), one in which a match whose requests sum to exactly its
    length has to leave at once: left in the order for one more pass, it keeps its neighbours apart and the result is another"""
    rng = random.Random({"three_passes": 7, "crossing": 8, "exact_death": 9}[what] + 10 * reverse)
    for _ in range(200000):
        k = rng.randint(3, 6)
        fam = [(rng.randint(1, 24), 100 + rng.randint(0, 30), 300 + 40 * j) for j in range(k)]
        e = R.eliminate_overlaps(*R.canonicalise([f[0] for f in fam], [[f[1], -f[2] if reverse else f[2]] for f in fam]))
        if (what == "three_passes" and e["passes"][0] >= 3 and len(e["orig"]) >= 2) or (what == "crossing" and e["reordered"]):
            return fam
        if what == "exact_death":
            cl, cs = R.canonicalise([f[0] for f in fam], [[f[1], -f[2] if reverse else f[2]] for f in fam])
            if survivors_if_exact_deaths_lingered(cl, cs) != sorted((l, tuple(t)) for l, t in zip(e["length"], e["start"])):
                return fam
    raise AssertionError("no %s list found" % what)


def tie_family(name, reverse=False):
    return TIE_FAMILIES[name] if name in TIE_FAMILIES else _searched(name, reverse)


TIE_NAMES = tuple(TIE_FAMILIES) + ("three_passes", "crossing", "exact_death")


def _family_records(name, reverse, off0=0, off1=0):
    fam = tie_family(name, reverse)
    return [f[0] for f in fam], [[f[1] + off0, -(f[2] + off1) if reverse else f[2] + off1] for f in fam]


def tie_alone(name, reverse):
    ln, st = _family_records(name, reverse)
    return _case("%s_%s" % (name, "rev" if reverse else "fwd"), 2, ln, st, device=True, small=True, runs=((0, 0),))


def ties_mixed(reverse):
    """every family, 1000 bases apart, in the middle of a list of 1100: 1000 single matches in front of them in both genomes, so
    the families lie around the first tile edge of both orders"""
    rng = random.Random(31 + reverse)
    nf = 1000
    lens = [rng.randint(3, 9) for _ in range(nf)]
    perms, rev = _perms(nf, 2, rng), _strands(nf, 2, rng)
    start = layout(lens, perms, rev, [{}, {}], rng)
    top = max(abs(x) for s in start for x in s) + 20
    spans = {}
    for j, name in enumerate(TIE_NAMES):
        ln, st = _family_records(name, reverse, top + 1000 * j, top + 1000 * j)
        spans[name] = (len(lens), len(ln))
        lens += ln
        start += st
    top += 1000 * len(TIE_NAMES) + 1000
    nt = 1100 - len(lens)
    tl = [rng.randint(3, 9) for _ in range(nt)]
    lens += tl
    start += layout(tl, _perms(nt, 2, rng), _strands(nt, 2, rng), [{}, {}], rng, base=top)
    return _case("ties_mixed_%s" % ("rev" if reverse else "fwd"), 2, lens, start, device=True, small=False,
                 aim={"first_family": nf, "n_family": sum(v[1] for v in spans.values())})


# ---- LCB graphs ---------------------------------------------------------------------------------------------------------------
def graph(name, N, sizes, node_perms, orient, seed, weight, lens=None, small=False):
    """an overlap-free list made of nodes: sizes[k] matches in node k (genome-0 order), node_perms[g] the order of the nodes along
    genome g, orient[k][g] True = node k is reverse in genome g (its matches then run backwards there)"""
    rng = random.Random(seed)
    first, n = [], 0
    for s in sizes:
        first.append(n)
        n += s
    lens = lens or [rng.randint(5, 12) for _ in range(n)]
    perms, rev = [], [[False] * N for _ in range(n)]
    for g in range(N):
        p = []
        for k in node_perms[g]:
            ms = list(range(first[k], first[k] + sizes[k]))
            if orient[k][g]:
                ms.reverse()
                for i in ms:
                    rev[i][g] = True
            p += ms
        perms.append(p)
    start = layout(lens, perms, rev, [{} for _ in range(N)], rng)
    return _case(name, N, lens, start, device=True, small=small, runs=((0, 0), (weight, 0), (0, 1)),
                 aim={"n_nodes": len(sizes), "first": first})


def _interleaved(n_big, light_every, seed, N=2):
    """genome 0: A1 x1 A2 x2 ...; genome 1: the A's, then the x's: every match is a node of its own, and deleting an x lets its
    two neighbours merge.  Every light_every-th x is light (3 columns), the others weigh as much as an A."""
    rng = random.Random(seed)
    sizes = [1] * (2 * n_big)
    lens = []
    for k in range(n_big):
        lens += [rng.randint(20, 30), 3 if k % light_every == 0 else rng.randint(20, 30)]
    order1 = list(range(0, 2 * n_big, 2)) + list(range(1, 2 * n_big, 2))
    node_perms = [list(range(2 * n_big)), order1] + [list(range(2 * n_big))] * (N - 2)
    orient = [[False] * N for _ in sizes]
    return sizes, node_perms, orient, lens


def tie_minima_gadget():
    """nodes R p q T U in genome 0 and R q U T p in genome 1, p and q equally light: deleting p (the first in genome-0 order) lets q
    merge with R and survive; deleting q first would leave p to be deleted as well"""
    sizes = [3, 1, 1, 3, 3]
    lens = [30] * 3 + [4, 4] + [30] * 6
    return graph("graph_tie_minima", 2, sizes, [[0, 1, 2, 3, 4], [0, 2, 4, 3, 1]], [[False, False]] * 5, 41, 4 * 2 + 1, lens=lens,
                 small=True)


def graphs():
    out = [tie_minima_gadget()]
    f3 = [[False] * 3]
    out.append(graph("graph_one_run", 3, [2 * TILE + 500], [[0]] * 3, f3, 42, 50))
    out.append(graph("graph_one_run_reverse", 3, [2 * TILE + 52], [[0]] * 3, [[False, True, False]], 43, 50))
    s, p, o, l = _interleaved(550, 25, 44)
    out.append(graph("graph_every_match_a_node", 2, s, p, o, 44, 3 * 2 + 1, lens=l))
    # breaks exactly at matches 1023 | 1024 and 2047 | 2048 of the genome-0 order, and one match off each; light nodes of 1 match
    # between heavy ones that are collinear but for them, two of them equally light
    for name, cut in (("graph_breaks_at_edges", (TILE, 2 * TILE)), ("graph_breaks_before_edges", (TILE - 1, 2 * TILE - 1)),
                      ("graph_breaks_behind_edges", (TILE + 1, 2 * TILE + 1))):
        sizes = [cut[0], cut[1] - cut[0], 500, 1, 300, 1, 200]
        # nodes 1, 4 and 6 are reverse in genome 1 (4 and 6 in "previous" order there: they merge once node 5 is gone), node 2 in genome 2
        perms = [list(range(7)), [1, 0, 2, 6, 4, 5, 3], [0, 1, 3, 5, 2, 4, 6]]
        orient = [[False, k in (1, 4, 6), k == 2] for k in range(7)]
        n = sum(sizes)
        lrng = random.Random(45)
        lens = [lrng.randint(5, 12) for _ in range(n)]
        lens[cut[1] + 500] = lens[cut[1] + 801] = 4          # the two single-match nodes, equally light
        out.append(graph(name, 3, sizes, perms, orient, 46 + cut[0], 4 * 3 + 1, lens=lens))
    # collinear in all genomes but one: genome 1 follows genome 0, genome 2 has the nodes in another order
    sizes = [300, 2, 400, 2, 396]
    out.append(graph("graph_all_but_one_genome", 3, sizes, [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 2, 4, 3, 1]], [[False] * 3] * 5, 47,
                     2 * 12 * 3 + 1))
    return out


# ---- width and key size -------------------------------------------------------------------------------------------------------
def wide(N, seed, overlaps):
    rng = random.Random(seed)
    n = 1100
    lens = [rng.randint(3, 9) for _ in range(n)]
    perms, rev = _perms(n, N, rng), _strands(n, N, rng)
    over = [{} for _ in range(N)]
    if overlaps:
        for g in range(N):
            for k in rng.sample(range(1, n), 60) + [TILE]:
                over[g][k] = ("gap", rng.randint(-1, 1))
    return _case("wide_N%d" % N, N, lens, layout(lens, perms, rev, over, rng), device=True, runs=((0, 0), (5 * N, 0)))


def key_width(longest, seed):
    """genome 1 is `longest` bases long and a match of length 1 sits on its last base: pos_bits + 1 = 8 | 9, 16 | 17, 24 | 25 bits of
    sort key on the two sides of 2^k, i.e. an odd or an even number of 8-bit passes"""
    rng = random.Random(seed)
    n = 18 if longest < 1000 else 1100
    lens = [rng.randint(1, 3) for _ in range(n)]
    perms, rev = _perms(n, 2, rng), _strands(n, 2, rng)
    over = [{}, {}]
    for g in range(2):
        for k in rng.sample(range(1, n - 1), n // 6):
            over[g][k] = ("gap", rng.randint(-1, 1))
    start = layout(lens, perms, rev, over, rng)
    # stretch genome 1 over its whole length, keeping the order and what overlaps: the entries behind a random cut move up
    last = perms[1][-1]
    lens[last] = 1
    room = longest - max(abs(s[1]) + l - 1 for l, s in zip(lens, start))
    assert room >= 0
    cut = abs(start[perms[1][n // 2]][1])
    for i in range(n):
        v = abs(start[i][1])
        if v >= cut:
            v += room
            start[i][1] = -v if start[i][1] < 0 else v
    assert abs(start[last][1]) == longest
    glen = [max(abs(s[0]) + l - 1 for l, s in zip(lens, start)) + 5, longest]
    return _case("key_width_%d" % longest, 2, lens, start, glen=glen, device=True, small=n < 100,
                 aim={"last_base": longest})


KEY_WIDTHS = (127, 128, 32767, 32768, 8388607, 8388608)


# ---- random dense lists ---------------------------------------------------------------------------------------------------------
def random_dense(count=40, seed=3):
    """the lists of tests/test_gpu_chain_upfront.py at n = 900 .. 2300, ties kept"""
    rng = random.Random(seed)
    out = []
    for c in range(count):
        N, n, span = rng.randint(2, 4), rng.randint(900, 2300), rng.randint(200, 4000)
        lens = [rng.randint(1, 59) for _ in range(n)]
        start = [[(-1 if g and rng.random() < 0.4 else 1) * rng.randint(1, span - 1) for g in range(N)] for _ in range(n)]
        out.append(_case("dense_%02d" % c, N, lens, start, glen=[span + 64] * N))
    return out


def random_scaled(count=24, seed=4):
    """The same lists with the span growing with the list: 15 .. 90 bases of genome per match.  At 900 matches and more the lists
    above are one overlap cluster each (mean depth n * 30 / span >= 7) and the device hands every one of them back; here the mean
    depth c is 0.33 .. 2.  The clusters are the busy periods of that coverage: a cluster goes on past a member with probability
    about 1 - exp(-c), so the largest of ~1000 clusters has about ln 1000 / -ln(1 - exp(-c)) members -- 15 at c = 1 (30 bases per
    match, four fifths of the range), 46 at c = 2.  Most lists therefore stay within CH_CL_MAX = 48 in every genome and are chained
    on the device over one to three tiles, random strands and ties included; the densest may still go back."""
    rng = random.Random(seed)
    out = []
    for c in range(count):
        N, n = rng.randint(2, 4), rng.randint(900, 2300)
        span = int(n * rng.uniform(15, 90))
        lens = [rng.randint(1, 59) for _ in range(n)]
        start = [[(-1 if g and rng.random() < 0.4 else 1) * rng.randint(1, span - 1) for g in range(N)] for _ in range(n)]
        out.append(_case("scaled_%02d" % c, N, lens, start, glen=[span + 64] * N))
    return out


# ---- the gapped case ------------------------------------------------------------------------------------------------------------
def gapped_case(seed=9):
    """N = 3 on 5000-base genomes: collinear matches with short gaps, all forward, and in front of them the `crossing` family (a
    pass carries a match past its neighbour in genome 0, so the chain order is not the list order)"""
    rng = random.Random(seed)
    fam = tie_family("crossing")
    lens = [f[0] for f in fam]
    start = [[f[1] - 90, f[2] - 290, f[2] - 280] for f in fam]
    base = max(max(s) for s in start) + 80
    n = 300
    tl = [rng.randint(6, 10) for _ in range(n)]
    ident = list(range(n))
    start += layout(tl, [ident, ident, ident], [[False] * 3] * n, [{}, {}, {}], rng, base=base)
    return _case("gapped", 3, lens + tl, start, glen=[5000] * 3, device=True)


def genomes(case, seed=1):
    """random bases for the genomes of a case (the gapped run reads them; the others only need their lengths)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, gl, dtype=np.uint8) for gl in case["glen"]]


FAMILY_NAMES = ("tile", "cluster", "cluster_cl5", "pool", "ties", "graph", "wide", "key", "dense", "dense_scaled")


@functools.lru_cache(maxsize=None)
def family(name):
    """the cases of one family; made once per process"""
    if name == "tile":
        return [tile_edge(n, N, kind, 1000 + n + N) for n in (1023, 1024, 1025, 2047, 2048, 2049, 4097) for N in (2, 3)
                for kind in ("pair", "triple", "abut")] + [long_reach()]
    if name == "ties":
        return [tie_alone(t, r) for t in TIE_NAMES for r in (False, True)] + [ties_mixed(False), ties_mixed(True)]
    if name == "wide":
        return [wide(5, 51, False), wide(17, 52, True), wide(32, 53, False)]
    if name == "key":
        return [key_width(g, 60 + k) for k, g in enumerate(KEY_WIDTHS)]
    return {"cluster": cluster_sizes, "cluster_cl5": cluster_sizes_cl5, "pool": pool_overflow, "graph": graphs,
            "dense": random_dense, "dense_scaled": random_scaled}[name]()


def families():
    return {name: family(name) for name in FAMILY_NAMES}
