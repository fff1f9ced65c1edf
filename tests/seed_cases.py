"""Planted genome sets for the seed pass (csrc/seed_pass.hip): buckets of the partially sorted list at the limits
of join_hash, the routes of seed_plan, hits at the tile and wave edges of mum_runs, junctions and the phase-3 shape, the walks of
mum_extend (repeat-led and repeat-tailed matches, gaps of span - 1 and span offsets, genome ends, many components, contigs and
ambiguous bases), caller-made patterns, and the hit sets handed to mauve_extend_hits.

A case is a dict: name, family, genomes (uint8 codes), pattern, mode, mask, extend, contigs / invalid (None, or what set_genomes
takes) and aim -- where the planted spot is, as data that tests/test_seed_cpu.py checks against the facts of tests/seed_ref.py and
the geometry below, never against the product.

The device form's geometry, as csrc/seed_pass.hip has it (the tests state it; they do not read it from the library):"""
import functools

import numpy as np

from tests import seed_ref as R

CHUNK = 2048            # join_hash: a workgroup owns the buckets that start in its chunk of the partially sorted list
RANGE_CAP = 3072        # ... and takes its range iff it ends at or before chunk start + 3072
PROBE = 64              # chunk_bound: 4 probes of 64 entries behind a chunk edge, then a binary search
OVERFLOW_RANGES = 4096  # more declined ranges than this: the whole list goes back
BUCKET_TARGET = 512     # SeedPlan::low_bits: 8-bit passes until the list length >> sorted bits is <= 512
TINY_MAX = 9216         # tiny_join: up to this many windows (and <= 16 genomes, 2 * weight <= 32)
TILE = 4096             # mum_runs: positions per tile,
HALO = 64               # ... the halo in front of it,
ROUND = 64              # mum_extend: offsets per round of a walk (and positions per wave in mum_runs)
MEM, UNIQUE, PAIRWISE = 0, 1, 2


# ---- geometry of the hash join, from the reference's key table ---------------------------------------------------------------
def low_bits(entries, full_bits):
    G = 0
    while G < full_bits and (entries >> G) > BUCKET_TARGET:
        G += 8
    return full_bits - min(G, full_bits)


def join_geometry(canon, weight):
    """canon: per genome the canonical mer of every window (all windows are in the list of an unmasked set) -> the partially
    sorted list's high parts, the chunk bounds and the ranges join_hash declines"""
    keys = np.concatenate(canon) if len(canon) else np.zeros(0, np.uint64)
    n = len(keys)
    L = low_bits(n, 2 * weight)
    order = np.argsort(keys >> np.uint64(L), kind="stable")      # list position -> global window (the partial sort is stable)
    high = (keys >> np.uint64(L))[order]
    edges = np.concatenate(([0], np.flatnonzero(high[1:] != high[:-1]) + 1, [n])) if n else np.array([0])
    nchunk = (n + CHUNK - 1) // CHUNK
    bound = [0] + [int(edges[np.searchsorted(edges, c * CHUNK)]) if c * CHUNK < n else n for c in range(1, nchunk + 1)]
    ranges = [(bound[c], bound[c + 1]) for c in range(nchunk)]
    declined = [(c, lo, hi) for c, (lo, hi) in enumerate(ranges) if lo < hi and hi > c * CHUNK + RANGE_CAP]
    return {"n": n, "L": L, "high": high, "order": order, "keys": keys, "edges": edges, "bound": bound, "ranges": ranges, "declined": declined}


def geometry_of(case):
    pat = case["pattern"]
    canon = []
    for g in case["genomes"]:
        F, Rv = R.window_mers(g, pat)
        canon.append(np.minimum(F, Rv))
    return join_geometry(canon, len(R.shape(pat)[0]))


def windows_of(case):
    span = R.shape(case["pattern"])[1]
    return sum(max(len(g) - span + 1, 0) for g in case["genomes"])


def takes_hash_join(case, no_tiny):
    """seed_plan: the hash join, unless the pass is pairwise or tiny"""
    w = len(R.shape(case["pattern"])[0])
    tiny = not no_tiny and windows_of(case) <= TINY_MAX and len(case["genomes"]) <= 16 and 2 * w <= 32
    return case["mode"] != PAIRWISE and not tiny


def takes_tiny(case, no_tiny):
    return case["mode"] != PAIRWISE and not takes_hash_join(case, no_tiny)


# ---- patterns ------------------------------------------------------------------------------------------------------------------
def solid(span):
    return (1 << span) - 1


def palindrome(span, weight, seed=0):
    """a palindromic pattern of that span and weight with both ends set (odd weight: odd span, the middle set)"""
    assert weight >= 2 and (weight % 2 == 0 or span % 2 == 1) and weight <= span
    rng = np.random.default_rng(1000 * span + weight + seed)
    bits = [0] * span
    bits[0] = bits[-1] = 1
    if weight % 2:
        bits[span // 2] = 1
    free = list(range(1, span // 2))
    rng.shuffle(free)
    for i in free[:(weight - 2) // 2]:
        bits[i] = bits[span - 1 - i] = 1
    assert sum(bits) == weight, (span, weight)
    return int("".join(map(str, bits)), 2)


def seed_table(w, rank=0):
    from oracle import pyoracle as O            # (the table of DESIGN.md S2 is data: csrc/seed_table.inc = oracle/seed_table.inc)
    return O.get_seed(w, rank)


SOLID = {("solid", s): solid(s) for s in (1, 2, 3, 4, 5, 8, 16)}
SPACED = {("spaced", s, w): palindrome(s, w) for s, w in ((7, 3), (9, 5), (15, 11), (17, 13), (31, 12), (32, 12), (33, 13), (48, 14), (49, 15))}
SPAN49 = {("span49", 31): palindrome(49, 31), ("span49", 5): palindrome(49, 5)}


def walk_patterns():
    """the patterns heavy enough (weight >= 9) for a genome pair of some ten thousand windows to hold unique mers"""
    out = [("table", w, seed_table(w)) for w in (11, 15, 16, 17, 31)]
    out += [("solid", 16, solid(16))] + [(k[0], k[1], p) for k, p in SPACED.items() if k[2] >= 9] + [("span49", 31, SPAN49[("span49", 31)])]
    return out


# ---- building blocks -----------------------------------------------------------------------------------------------------------
def rc(x):
    return (3 - np.asarray(x, np.uint8))[::-1].copy()


def other(x):
    """a different base (A <-> C, G <-> T: stays inside a two-letter alphabet)"""
    return np.asarray(x, np.uint8) ^ 1


def _case(name, family, genomes, pattern, mode=MEM, mask=0, extend=True, aim=None, contigs=None, invalid=None):
    return {"name": name, "family": family, "genomes": [np.ascontiguousarray(g, dtype=np.uint8) for g in genomes], "pattern": int(pattern),
            "mode": mode, "mask": mask, "extend": extend, "aim": aim or {}, "contigs": contigs, "invalid": invalid}


def valid_intervals(case):
    """the 1-based inclusive intervals a window must lie in: the contigs, cut at every ambiguous base (None: no table)"""
    if case["contigs"] is None and case["invalid"] is None:
        return None
    out = []
    for g, x in enumerate(case["genomes"]):
        starts = list(case["contigs"][g]) if case["contigs"] else [0]
        bad = np.asarray(case["invalid"][g], bool) if case["invalid"] else np.zeros(len(x), bool)
        iv = []
        for a, b in zip(starts, starts[1:] + [len(x)]):
            cur = a
            for p in list(np.flatnonzero(bad[a:b]) + a) + [b]:
                if p > cur:
                    iv.append((cur + 1, int(p)))
                cur = p + 1
        out.append(iv)
    return out


def _tune(build, measure, target, start, tries=40):
    v = start
    for _ in range(tries):
        case = build(v)
        got = measure(case)
        if got == target:
            return case
        v += target - got
        assert v >= 0, "the planted run cannot be made that short"
    raise AssertionError("the planted size was not reached")


# ---- bucket edges (join_hash) --------------------------------------------------------------------------------------------------
def _bucket_set(seed, a_run, c_run, alphabet=4, core=6000, w=11, n_genomes=2, ac_run=0, pattern=None):
    """genome 0: a random core; genome 1 (and 2): the core with a substitution every 150 bases, then runs of A, of C and of AC
    (each fills one or two mers' buckets with its window count), set apart by random bases"""
    rng = np.random.default_rng(seed)
    draw = (lambda n: rng.integers(0, 4, n, dtype=np.uint8)) if alphabet == 4 else (lambda n: rng.integers(0, 2, n, dtype=np.uint8))
    S = draw(core)
    gs = [S]
    for g in range(1, n_genomes):
        x = S.copy()
        x[70 * g::150] ^= 1
        tail = [draw(40), np.zeros(a_run, np.uint8), draw(40), np.ones(c_run, np.uint8), draw(40)]
        if ac_run:
            tail += [np.tile(np.array([0, 1], np.uint8), ac_run // 2), draw(40)]
        gs.append(np.concatenate([x] + tail) if g == 1 else x)
    return gs, (pattern or seed_table(w))


def _bucket_of(case, geo, base):
    """start and end in the list of the bucket that holds the windows of a run of `base`"""
    w = len(R.shape(case["pattern"])[0])
    key = sum(base << (2 * i) for i in range(w))
    key = min(key, sum((3 - base) << (2 * i) for i in range(w)))
    h = np.uint64(key >> geo["L"])
    return int(np.searchsorted(geo["high"], h, "left")), int(np.searchsorted(geo["high"], h, "right"))


def bucket_limit(place, delta, n_genomes=2, seed=5):
    """the range of one chunk ends at chunk start + 3072 + delta.  place: "first" (the bucket of the A run is the first of the list,
    chunk 0), "mid" (the bucket of the C run starts in the middle of a later chunk), "last" (two-letter genomes: the bucket of the
    C run is the last of the list and the range ends at n)"""
    def measure(case):
        geo = geometry_of(case)
        s, e = _bucket_of(case, geo, 0 if place == "first" else 1)
        c = s // CHUNK
        case["aim"] = {"chunk": c, "lo": geo["bound"][c], "hi": geo["bound"][c + 1], "bucket": (s, e), "delta": delta, "place": place}
        return geo["bound"][c + 1] - c * CHUNK
    if place == "first":
        build = lambda v: _case("limit_first%+d_n%d" % (delta, n_genomes), "bucket", *_bucket_set(seed, v, 0, n_genomes=n_genomes))
    elif place == "mid":
        build = lambda v: _case("limit_mid%+d_n%d" % (delta, n_genomes), "bucket", *_bucket_set(seed, 0, v, n_genomes=n_genomes))
    else:
        build = lambda v: _case("limit_last%+d_n%d" % (delta, n_genomes), "bucket", *_bucket_set(seed, 0, v, alphabet=2, w=15, n_genomes=n_genomes))
    return _tune(build, measure, RANGE_CAP + delta, 2600)


def bucket_spanning(seed=6):
    """a bucket that starts in one chunk and covers the next two: they own nothing"""
    case = _case("limit_spanning", "bucket", *_bucket_set(seed, 0, 7000))
    geo = geometry_of(case)
    s, e = _bucket_of(case, geo, 1)
    case["aim"] = {"chunk": s // CHUNK, "lo": geo["bound"][s // CHUNK], "hi": e, "bucket": (s, e), "place": "spanning"}
    return case


def bound_distance(d, seed=7):
    """the first bucket boundary behind a chunk edge lies d entries behind it (the C run's bucket, 700 entries and more, reaches
    over the edge; the A run in front of it shifts it).  The entry AT the boundary -- the first of the next bucket, which a bound
    one too far cuts off from it -- is a window of a hit: its mer is held twice in all, once by each of two genomes"""
    for sd in range(seed, seed + 60):
        state = {}

        def measure(case):
            geo = geometry_of(case)
            s, e = _bucket_of(case, geo, 1)
            if "edge" not in state:
                state["edge"] = (e // CHUNK + 1) * CHUNK
            case["aim"] = {"edge": state["edge"], "distance": d, "bucket": (s, e)}
            return e - state["edge"]
        case = _tune(lambda v: _case("bound_%d" % d, "bucket", *_bucket_set(sd, v, 700)), measure, d, 100)
        geo = geometry_of(case)
        at = int(geo["order"][state["edge"] + d])
        same = np.flatnonzero(geo["keys"] == geo["keys"][at])
        nw0 = len(case["genomes"][0]) - R.shape(case["pattern"])[1] + 1
        if len(same) == 2 and same[0] < nw0 <= same[1]:
            case["aim"]["boundary_window"] = at
            return case
    raise AssertionError("no draw with a hit at the boundary")


def bound_at_n(seed=8):
    """the last bucket reaches over the last chunk edge and ends the list 100 entries behind it: a probe of chunk_bound runs into n"""
    def measure(case):
        geo = geometry_of(case)
        s, e = _bucket_of(case, geo, 1)
        case["aim"] = {"edge": (s // CHUNK + 1) * CHUNK, "distance": "n", "bucket": (s, e)}
        return e - (s // CHUNK + 1) * CHUNK
    return _tune(lambda v: _case("bound_n", "bucket", *_bucket_set(seed, 0, v, alphabet=2, w=15)), measure, 100, 1500)


def list_length(k, delta, seed=9):
    """a list of 2048 k + delta entries"""
    rng = np.random.default_rng(seed)
    pat = seed_table(11)
    span = R.shape(pat)[1]
    S = rng.integers(0, 4, 5000, dtype=np.uint8)
    L1 = CHUNK * k + delta - (5000 - span + 1) + span - 1
    x = np.concatenate([S, rng.integers(0, 4, L1 - 5000, dtype=np.uint8)])
    x[70:5000:150] ^= 1
    return _case("length_%dk%+d" % (k, delta), "bucket", [S, x], pat, aim={"entries": CHUNK * k + delta})


def several_overflows(w, seed=10):
    """three runs, each beyond the limit, in one pass: 2 w key bits = an odd or an even number of radix passes over a slice"""
    case = _case("overflows_w%d" % w, "bucket", *_bucket_set(seed + w, 3500, 3500, w=w, ac_run=7400))
    case["aim"] = {"several": True}
    return case


def width(n_genomes, mode, seed=11):
    """a mer held once by genomes 0 and N - 1; another held once by genomes 0 and 1 and twice by genome N - 1 (its bit in the
    `multi` half of the narrow table is bit 31 for N = 16; N = 17 takes the wide table)"""
    rng = np.random.default_rng(seed + n_genomes)
    pat = seed_table(11)
    U, V = rng.integers(0, 4, 60, dtype=np.uint8), rng.integers(0, 4, 60, dtype=np.uint8)
    gs = [rng.integers(0, 4, 620, dtype=np.uint8) for _ in range(n_genomes)]
    gs[0] = np.concatenate([gs[0][:200], U, gs[0][200:400], V, gs[0][400:]])
    gs[1] = np.concatenate([gs[1][:300], V, gs[1][300:]])
    last = gs[-1]
    gs[-1] = np.concatenate([last[:100], V, last[100:250], U, last[250:500], V, last[500:]])
    return _case("width_n%d_%s" % (n_genomes, "mem" if mode == MEM else "unique"), "bucket", gs, pat, mode=mode,
                 aim={"once": (0, n_genomes - 1), "once_at": 210, "twice_in": n_genomes - 1, "others": (0, 1), "others_at": 470})


def self_complementary(table_seed, reverse, seed=12):
    """a window whose masked mer is its own reverse complement (even weight), shared by two genomes"""
    rng = np.random.default_rng(seed)
    pat = seed_table(16) if table_seed else solid(16)
    offs, span = R.shape(pat)
    S = rng.integers(0, 4, 5200, dtype=np.uint8)
    W = rng.integers(0, 4, span, dtype=np.uint8)
    for i in range(span // 2):
        W[span - 1 - i] = 3 - W[i]
    S[3000:3000 + span] = W
    x = S.copy()
    x[70::170] ^= 1
    x[3000:3000 + span] = W
    return _case("selfrc_%s_%s" % ("table" if table_seed else "solid", "rev" if reverse else "fwd"), "bucket", [S, rc(x) if reverse else x], pat,
                 aim={"window": 3000})


@functools.lru_cache(None)
def bucket_cases():
    out = [bucket_limit(place, delta) for place in ("first", "mid", "last") for delta in (-1, 0, 1)]
    out += [bucket_limit("first", 1, n_genomes=3), bucket_limit("mid", 0, n_genomes=3), bucket_spanning()]
    out += [bound_distance(d) for d in (0, 1, 63, 64, 255, 256, 257)] + [bound_at_n()]
    out += [list_length(5, delta) for delta in (-1, 0, 1)]
    out += [several_overflows(w) for w in (11, 16, 17, 21)]
    out += [width(n, mode) for n in (16, 17) for mode in (MEM, UNIQUE)]
    out += [self_complementary(t, r) for t in (False, True) for r in (False, True)]
    # once more without extension: every hit is a match of its own, so a hit lost inside a cluster shows
    out += [dict(c, name=c["name"] + "_noext", extend=False) for c in out]
    return out


# ---- routes (seed_plan) ----------------------------------------------------------------------------------------------------------
def _pair(rng, length, other_length=None, every=170):
    S = rng.integers(0, 4, length, dtype=np.uint8)
    x = S.copy()
    x[70::every] ^= 1
    if other_length is not None:
        x = np.concatenate([x, rng.integers(0, 4, max(other_length - length, 0), dtype=np.uint8)])[:other_length]
    return S, x


@functools.lru_cache(None)
def route_cases():
    out = []
    rng = np.random.default_rng(21)
    pat = seed_table(11)
    span = R.shape(pat)[1]
    for P in (TINY_MAX - 1, TINY_MAX, TINY_MAX + 1):
        S, x = _pair(rng, 4700, P - (4700 - span + 1) + span - 1)
        out.append(_case("windows_%d" % P, "route", [S, x], pat, aim={"windows": P, "tiny": P <= TINY_MAX}))
    for n in (16, 17):
        S = rng.integers(0, 4, 400, dtype=np.uint8)
        gs = []
        for g in range(n):
            x = S.copy()
            x[17 * g % 60 + 30::60] ^= 1
            gs.append(x)
        out.append(_case("genomes_%d" % n, "route", gs, pat, mode=UNIQUE, aim={"windows": n * (400 - span + 1), "tiny": n <= 16}))
    for w in (15, 16, 17):
        p = seed_table(w)
        S, x = _pair(rng, 3000)
        out.append(_case("weight_%d" % w, "route", [S, x], p, aim={"windows": 2 * (3000 - R.shape(p)[1] + 1), "tiny": w <= 16}))
    # rows of tiny_join: global windows 1023 | 1024 of genome 0 and 9215, the last window of genome 1, are hits (extend = 0: every hit is a match)
    S = rng.integers(0, 4, 4700, dtype=np.uint8)
    L1 = TINY_MAX - (4700 - span + 1) + span - 1
    x = np.concatenate([rng.integers(0, 4, L1 - 1500, dtype=np.uint8), S[900:2400]])
    for ext in (False, True):
        out.append(_case("tiny_rows_ext%d" % ext, "route", [S, x], pat, extend=ext, aim={"windows": TINY_MAX, "tiny": True, "hit_windows": (1023, 1024, TINY_MAX - 1)}))
    S, x = _pair(rng, 2000)
    out.append(_case("short_between", "route", [S, rng.integers(0, 4, span - 1, dtype=np.uint8), x], pat, aim={"windows": 2 * (2000 - span + 1), "tiny": True}))
    out.append(_case("empty_first", "route", [np.zeros(0, np.uint8), S, x], pat, aim={"windows": 2 * (2000 - span + 1), "tiny": True}))
    out.append(_case("empty_last", "route", [S, x, np.zeros(0, np.uint8)], pat, aim={"windows": 2 * (2000 - span + 1), "tiny": True}))
    # a component set asked for (MaskedMemHash::SetMask) while hits of other sets lie around: three genomes, each with its own substitutions
    for length in (2000, 3400):
        S = rng.integers(0, 4, length, dtype=np.uint8)
        gs = [S.copy() for _ in range(3)]
        for g in range(3):
            gs[g][40 + 23 * g::97] ^= 1
        for want in (3, 5, 6, 7):
            for mode in (MEM, UNIQUE):
                out.append(_case("mask_%d_%d_%s" % (want, length, "mem" if mode == MEM else "unique"), "route", gs, pat, mode=mode, mask=want,
                                 aim={"windows": 3 * (length - span + 1), "tiny": length == 2000, "mask": want}))
    return out


# ---- tile and wave edges of mum_runs -----------------------------------------------------------------------------------------------
def _others(S, n_genomes, rng):
    """genomes 2 .. : the core with their own substitutions far from the planted spots (every 1000 bases from 500 + 100 g on)"""
    out = []
    for g in range(2, n_genomes):
        x = S.copy()
        x[500 + 100 * g::1000] ^= 1
        out.append(x)
    return out


def junction(edge, d, reverse, n_genomes=2, pattern=None, mode=MEM, seed=31):
    """genome 1 = the core up to the window at edge - 1, a spacer, the core from the window at edge - 1 + d on: the last window of
    the first copy and the first of the second are hits d apart on different diagonals (d = 0: no junction, one diagonal)"""
    rng = np.random.default_rng(seed + edge + 7 * d)
    pat = pattern or seed_table(11)
    span = R.shape(pat)[1]
    S = rng.integers(0, 4, max(edge + 1200, 9000 if edge > 4096 else 5300), dtype=np.uint8)
    q1 = edge - 1
    if d:
        spacer = rng.integers(0, 4, 3, dtype=np.uint8)
        spacer[0] = other(S[q1 + span]) if q1 + span < len(S) else spacer[0]
        spacer[-1] = other(S[q1 + d - 1])
        x = np.concatenate([S[:q1 + span], spacer, S[q1 + d:]])
    else:
        x = S.copy()
    gs = [S, rc(x) if reverse else x] + _others(S, n_genomes, rng)
    name = "junction_s%d_e%d_d%d_%s_n%d%s" % (span, edge, d, "rev" if reverse else "fwd", n_genomes, "_pw" if mode == PAIRWISE else "")
    return _case(name, "tile", gs, pat, mode=mode, aim={"hits": (q1, q1 + d), "d": d, "edge": edge})


def transposition(p, d, reverse, seed=36, mode=MEM, extend=True):
    """genome 0 holds a stretch of span + d bases with period 2 d at window p - d; genome 1 holds, in the same place, the stretch
    turned by d (d = span: two windows X Y against Y X, no period needed).  The windows at p - d and p are same-mask hits d apart
    whose genome-1 windows lie d apart the WRONG way round: the neighbour's at +d where a hit of p's diagonal has it at -d (a
    forward component; mirrored for a reversed one).  Two diagonals, a match each, and p is the leftmost hit of its own."""
    pat = seed_table(11)
    span = R.shape(pat)[1]
    q = p - d
    for s in range(seed, seed + 60):
        rng = np.random.default_rng(s + p + 7 * d)
        S = rng.integers(0, 4, p + 1200, dtype=np.uint8)
        period = rng.integers(0, 4, 2 * d, dtype=np.uint8)
        S[q:q + span + d] = np.resize(period, span + d)
        x = S.copy()
        x[q:q + span + d] = np.resize(np.roll(period, -d), span + d)
        name = "transposed_p%d_d%d_%s%s%s" % (p, d, "rev" if reverse else "fwd", "_pw" if mode == PAIRWISE else "", "" if extend else "_noext")
        case = _case(name, "tile", [S, rc(x) if reverse else x], pat, mode=mode, extend=extend, aim={"hits": (q, p), "d": d, "reverse": reverse})
        if not _held_once(S, x, pat, [q, p]):
            continue
        # (a flank's first base may go on like the period: then a window beside the stretch is a hit of one of the two diagonals too)
        near = [h for h in R.find([S, x], pat)["hits"] if q - span <= h[2][0] <= p + span and h[2][1] != h[2][0]]
        if sorted(h[2] for h in near) == [(q, p), (p, q)]:
            return case
    raise AssertionError("no draw with the two transposed hits alone")


def hit_gap(edge, dist, seed=32, mode=MEM):
    """hits at edge - 1 and edge - 1 + dist on one diagonal with no hit between: the windows between also lie in a second copy
    behind genome 1 (held twice: no hits, yet they agree, so S4 has one match)"""
    rng = np.random.default_rng(seed + edge + dist)
    pat = seed_table(11)
    span = R.shape(pat)[1]
    S = rng.integers(0, 4, max(edge + 1200, 5300), dtype=np.uint8)
    q1 = edge - 1
    x = np.concatenate([S, rng.integers(0, 4, 30, dtype=np.uint8), S[q1 + 1:q1 + dist - 1 + span], rng.integers(0, 4, 30, dtype=np.uint8)])
    x[len(S) + 29] = other(S[q1])
    x[len(S) + 30 + dist - 2 + span] = other(S[q1 + dist - 1 + span])
    return _case("hitgap_e%d_%d%s" % (edge, dist, "_pw" if mode == PAIRWISE else ""), "tile", [S, x], pat, mode=mode,
                 aim={"gap": (q1, q1 + dist), "edge": edge})


def interleaved(k, seed=33):
    """N = 4, UNIQUE: stretches of 16 positions whose hits have k different component sets follow each other inside one wave's 64
    positions (a repeat of the stretch in one genome takes that genome out of its hits)"""
    rng = np.random.default_rng(seed + k)
    pat = seed_table(11)
    span = R.shape(pat)[1]
    S = rng.integers(0, 4, 5300, dtype=np.uint8)
    gs = [S.copy() for _ in range(4)]
    sets = []
    for i in range(k):
        lo = 4096 + 16 * i                              # windows lo .. lo + 15 - span would need a stretch longer than the span: whole windows
        drop = 1 + i % 3
        if i:                                           # (stretch 0 keeps all four genomes)
            gs[drop] = np.concatenate([gs[drop], rng.integers(0, 4, 25, dtype=np.uint8), S[lo:lo + 16 + span - 1]])
            sets.append((lo, 15 ^ (1 << drop)))
        else:
            sets.append((lo, 15))
    return _case("interleaved_%d" % k, "tile", gs, pat, mode=UNIQUE, aim={"sets": sets})


def phase3(p, seed=34, mode=MEM):
    """spaced seed: hit p; the window at p - 1 of genome 0 is broken on p's diagonal (a substitution under its first care position,
    which no window from p on reads and which the window at p - d2 does not care about) and sits once more behind genome 1 -- a
    same-mask hit on another diagonal; the hit at p - d2 is on p's diagonal.  One match through p - d2 and p."""
    rng = np.random.default_rng(seed + p)
    pat = seed_table(11)
    offs, span = R.shape(pat)
    d2 = 1 + next(z for z in range(1, span) if z not in offs)
    S = rng.integers(0, 4, p + 1200, dtype=np.uint8)
    x = S.copy()
    x[p - 1] = other(x[p - 1])
    x = np.concatenate([x, rng.integers(0, 4, 30, dtype=np.uint8), S[p - 1:p - 1 + span], rng.integers(0, 4, 30, dtype=np.uint8)])
    x[len(S) + 29] = other(S[p - 2])
    x[len(S) + 30 + span] = other(S[p - 1 + span])
    return _case("phase3_p%d%s" % (p, "_pw" if mode == PAIRWISE else ""), "tile", [S, x], pat, mode=mode, aim={"p": p, "d1": 1, "d2": d2})


def slice_edge(back, seed=35):
    """MODE_PAIRWISE, N = 3: genome 0 so long that the last hit of the pair (0, 1)'s anchor positions lies `back` positions in
    front of the first window of genome 1 -- the start `lo` of the next genome's slice"""
    rng = np.random.default_rng(seed + back)
    pat = seed_table(11)
    span = R.shape(pat)[1]
    S = rng.integers(0, 4, 3000, dtype=np.uint8)
    g0 = np.concatenate([S, rng.integers(0, 4, back - 1, dtype=np.uint8)]) if back > 1 else S
    x = S.copy()
    x[70:2900:170] ^= 1
    y = S.copy()
    y[110:2900:170] ^= 1
    return _case("slice_edge_%d" % back, "tile", [g0, x, y], pat, mode=PAIRWISE, aim={"last_hit": len(S) - span, "back": back})


@functools.lru_cache(None)
def tile_cases():
    out = []
    span = R.shape(seed_table(11))[1]
    for edge in (4096, 8192, 64 + 4096):
        out += [junction(edge, d, False) for d in (0, 1, 2, span - 1, span, span + 1)]
        out += [hit_gap(edge, span), hit_gap(edge, span + 1)]
    out += [junction(4096, d, True) for d in (1, 2, span - 1, span, span + 1)]
    out += [junction(64, d, False) for d in (0, 1, span)] + [junction(4096, 1, False, n_genomes=n) for n in (3, 4)]
    out += [junction(4096, d, False, pattern=SPACED[("spaced", 33, 13)]) for d in (1, 32, 33, 34)]
    out += [interleaved(3), interleaved(4)]
    out += [phase3(p) for p in (5000, 4096, 4097, 4096 + 64)]
    # the same under MODE_PAIRWISE: N = 2 (full sort, mum_join) and N = 3 (run_summary, join_pair_group, mum_runs_group)
    out += [junction(4096, d, r, mode=PAIRWISE) for d in (1, span, span + 1) for r in (False, True)]
    out += [junction(4096, d, False, n_genomes=3, mode=PAIRWISE) for d in (0, 1, span, span + 1)]
    out += [hit_gap(4096, span, mode=PAIRWISE), hit_gap(4096, span + 1, mode=PAIRWISE), phase3(4096, mode=PAIRWISE), phase3(5000, mode=PAIRWISE)]
    out += [slice_edge(b) for b in (1, 2, 63, 64)]
    # transposed windows: the one shape in which the neighbour's other-genome window lies d windows on the far side (at a tile edge --
    # the neighbour in the halo -- and off it; d = span, and smaller d with a period of 2 d)
    out += [transposition(p, d, r) for p in (4096, 5000) for d in (span, 2) for r in (False, True)]
    out += [transposition(4096, d, False) for d in (1, span - 1)] + [transposition(4096 + 64, span, True), transposition(4096, span, False, mode=PAIRWISE)]
    # without extension every hit is a candidate and a match of its own
    out += [dict(c, name=c["name"] + "_noext", extend=False) for c in (junction(4096, 1, False), junction(4096, span, True), phase3(4096))]
    out.append(transposition(4096, span, False, extend=False))
    return out


# ---- walks of mum_extend -------------------------------------------------------------------------------------------------------------
GAP = 50


def _blocks_case(name, family, pat, blocks, rng, reverse=False, **kw):
    """blocks: (piece of genome 0, piece of genome 1, aim with windows relative to the piece).  GAP bases (longer than any span) set
    the pieces apart; they differ between the genomes throughout, and from aim["not_before"] / aim["not_behind"] next to a piece"""
    g0, g1, aims = [], [], []
    n = 0
    for i, (a, b, aim) in enumerate(blocks + [(np.zeros(0, np.uint8), np.zeros(0, np.uint8), {})]):
        s0 = rng.integers(0, 4, GAP, dtype=np.uint8)
        s1 = other(s0)                                   # (every base differs: no window that reads one under a care position agrees)
        avoid = int(aim.get("not_before", 0))
        s0[-1], s1[-1] = avoid ^ 2, avoid ^ 3
        if i:
            avoid = int(blocks[i - 1][2].get("not_behind", 0))
            s0[0], s1[0] = avoid ^ 1, avoid ^ 2
        assert len(a) == len(b)
        g0 += [s0, a]
        g1 += [s1, b]
        n += GAP
        if i < len(blocks):
            aims.append(dict(aim, at=n))
        n += len(a)
    g0, g1 = np.concatenate(g0), np.concatenate(g1)
    if not _held_once(g0, g1, pat, [b["at"] + b["hit"] for b in aims]):
        return None                                      # (a planted hit's mer occurs once more by chance: the caller draws again)
    return _case(name, family, [g0, rc(g1) if reverse else g1], pat, aim={"blocks": aims, "reverse": reverse}, **kw)


def _held_once(g0, g1, pat, windows):
    """every one of these windows of genome 0 holds a mer that both genomes hold exactly once"""
    canon = [np.sort(np.minimum(*R.window_mers(g, pat))) for g in (g0, g1)]
    mine = np.minimum(*R.window_mers(g0, pat))[windows]
    return all(((np.searchsorted(c, mine, "right") - np.searchsorted(c, mine, "left")) == 1).all() for c in canon)


def _drawn(build, seed):
    for s in range(seed, seed + 4000, 100):
        case = build(s)
        if case is not None:
            return case
    raise AssertionError("no draw without a chance repeat of a planted hit")


def repeat_lengths(span):
    return sorted({r for r in list(range(62, 67)) + list(range(126, 131)) + list(range(64 - span - 1, 64 - span + 2)) + [200] if r >= 1})


def repeat_walks(tag, pat, reverse=False, extend=True, seed=41, lengths=None, part=""):
    return _drawn(lambda s: _repeat_walks(tag, pat, reverse, extend, s, lengths, part), seed)


def _repeat_walks(tag, pat, reverse, extend, seed, lengths=None, part=""):
    """per r and side: a shared unique stretch with a shared two-copy repeat of r whole windows directly in front of it (led) or
    behind it (tailed); the other copy of the repeat lies GAP bases away.  The repeat's windows agree and are no hits."""
    offs, span = R.shape(pat)
    rng = np.random.default_rng(seed + span + len(offs))
    blocks = []
    for r in lengths or repeat_lengths(span):
        for side in ("led", "tailed"):
            U = rng.integers(0, 4, (100 if lengths is None else 20) + span, dtype=np.uint8)
            rep = rng.integers(0, 4, r + span - 1, dtype=np.uint8)
            f0 = rng.integers(0, 4, GAP, dtype=np.uint8)
            f1 = other(f0)
            if side == "led":                               # rep U f rep: the stretch starts with the repeat's windows
                a, b = np.concatenate([rep, U, f0, rep]), np.concatenate([rep, U, f1, rep])
                aim = {"side": side, "r": r, "hit": r, "not_behind": U[0]}
            else:                                           # rep f U rep
                a, b = np.concatenate([rep, f0, U, rep]), np.concatenate([rep, f1, U, rep])
                aim = {"side": side, "r": r, "hit": len(rep) + GAP + len(U) - 1, "not_before": U[-1]}
            blocks.append((a, b, aim))
    name = "repeat_%s_%s%s%s%s" % (tag[0], tag[1], part, "_rev" if reverse else "", "" if extend else "_noext")
    case = _blocks_case(name, "walk", pat, blocks, rng, reverse=reverse, extend=extend)
    if case is not None:
        case["aim"]["lengths"] = sorted(lengths or repeat_lengths(span))
    return case


@functools.lru_cache(None)
def gap_substitutions(pat, k):
    """bases (relative to the run's first window) of substitutions under which, with this pattern, windows 0 .. k - 1 disagree, windows
    -1 and k agree, and every other run of disagreeing windows is shorter than k.  A base may be substituted iff neither window -1
    nor window k reads it under a care position; of those, greedily the ones that cover the most windows still uncovered.
    -> (bases, first disagreeing window, last disagreeing window), or None (a solid seed has no run of span - 1)"""
    offs, span = R.shape(pat)
    care = set(offs)
    allowed = [b for b in range(0, k + span - 1) if (b + 1) not in care and (b - k) not in care]
    covers = {b: {b - o for o in offs if 0 <= b - o < k} for b in allowed}
    left, subs = set(range(k)), []
    while left:
        v = min(left)
        pick = max((b for b in allowed if v in covers[b]), key=lambda b: len(covers[b] & left), default=None)
        if pick is None:
            return None
        subs.append(pick)
        left -= covers[pick]
    bad = sorted({b - o for b in subs for o in offs})
    runs, cur = [], [bad[0], bad[0]]
    for v in bad[1:]:
        if v == cur[1] + 1:
            cur[1] = v
        else:
            runs.append(cur)
            cur = [v, v]
    runs.append(cur)
    assert [0, k - 1] in runs
    if any(r[1] - r[0] + 1 >= k for r in runs if r != [0, k - 1]):
        return None
    return tuple(sorted(subs)), bad[0], bad[-1]


def gap_offsets(span):
    return sorted({f for f in list(range(64 - span - 2, 64 - span + 3)) + list(range(60, 67)) if f >= 1})


def gap_walks(tag, pat, reverse=False, seed=42, extend=True, offsets=None, part=""):
    return _drawn(lambda s: _gap_walks(tag, pat, reverse, s, extend, offsets, part), seed)


def _gap_walks(tag, pat, reverse, seed, extend=True, offsets=None, part=""):
    """a run of exactly span - 1 (it chains) and of exactly span (it splits) disagreeing offsets at f offsets from the leftmost
    hit: to the right, inside the unique stretch (the run's first offset is hit + f); to the left, mirrored, inside the first copy
    of a two-copy repeat that leads the stretch (the run's last offset is hit - f)"""
    offs, span = R.shape(pat)
    rng = np.random.default_rng(seed + span + len(offs))
    blocks = []
    for k in (span - 1, span):
        found = gap_substitutions(pat, k)
        if found is None:                                     # (a solid seed has no run of span - 1: one substitution breaks span windows)
            continue
        subs, lo, hi = found
        for f in offsets or gap_offsets(span):
            if f + lo < 1:                                    # (an earlier, shorter run would reach the leftmost hit itself)
                continue
            for side in ("right", "left"):
                lead = f + hi + 2 * span + 10 if side == "left" else 0      # the repeat's whole windows in front of the stretch
                rep = rng.integers(0, 4, lead + span - 1, dtype=np.uint8) if lead else np.zeros(0, np.uint8)
                U = rng.integers(0, 4, (f + hi + 3 * span + 20 if side == "right" else 60 + span), dtype=np.uint8)
                f0 = rng.integers(0, 4, GAP, dtype=np.uint8)
                f1 = other(f0)
                a = np.concatenate([rep, U, f0, rep])
                b = np.concatenate([rep, U, f1, rep])
                hit = lead
                if side == "right":
                    first = hit + f
                    where = [first + s for s in subs]
                else:
                    first = hit - f - k + 1
                    where = [first + (k - 1) + (span - 1) - s for s in subs]
                    assert min(where) >= 0 and max(where) < lead + span - 1
                b[where] = other(b[where])
                blocks.append((a, b, {"side": side, "k": k, "f": f, "hit": hit, "run": (first, first + k - 1), "not_behind": U[0]}))
    name = "gap_%s_%s%s%s%s" % (tag[0], tag[1], part, "_rev" if reverse else "", "" if extend else "_noext")
    return _blocks_case(name, "walk", pat, blocks, rng, reverse=reverse, extend=extend)


def genome_end(which, side, residue, pat, tag, seed=43, extend=True):
    """N = 3, genome 2 reverse-complemented.  The shared stretch starts on the first base (side "first") or ends on the last base
    ("last") of genome `which`; every genome's length is = residue (mod 64); in the other genomes the stretch starts at base 32, 63
    or 31 (leftmost hits at windows = 0 and 31 mod 32)"""
    offs, span = R.shape(pat)
    rng = np.random.default_rng(seed + 64 * which + residue + span)
    U = rng.integers(0, 4, 150 + span, dtype=np.uint8)
    out = []
    for g in range(3):
        s = side if g != 2 else {"first": "last", "last": "first"}[side]     # (genome 2 is built as its reverse complement)
        if g == which and s == "first":
            front, back = 0, 40 + (residue - len(U) - 40) % 64
        elif g == which:
            front, back = 32 + (residue - len(U) - 32) % 64, 0
        else:
            front = (32, 63, 31)[(g + residue) % 3]
            back = 40 + (residue - front - len(U) - 40) % 64
        f, b = rng.integers(0, 4, front, dtype=np.uint8), rng.integers(0, 4, back, dtype=np.uint8)
        if front:
            f[-1] = g                                          # (three different bases in front of and behind the stretch)
        if back:
            b[0] = g
        x = np.concatenate([f, U, b])
        assert len(x) % 64 == residue
        out.append(rc(x) if g == 2 else x)
    name = "end_%s_%s_g%d_%s_mod%d%s" % (tag[0], tag[1], which, side, residue, "" if extend else "_noext")
    return _case(name, "walk", out, pat, extend=extend, aim={"end": (which, side), "residue": residue, "components": 3})


def many_components(n, mode, seed=44, extend=True):
    """n genomes share a stretch; every third one is reverse-complemented; in component n - 1 (>= 8: the second or a later round of
    eight) the stretch ends on the genome's last base (first base for a reversed one)"""
    rng = np.random.default_rng(seed + n)
    pat = seed_table(11)
    U = rng.integers(0, 4, 120, dtype=np.uint8)
    gs = []
    for g in range(n):
        f = rng.integers(0, 4, 20 + (g * 13) % 50, dtype=np.uint8)
        b = rng.integers(0, 4, 0 if g == n - 1 else 30 + (g * 7) % 40, dtype=np.uint8)
        x = np.concatenate([f, U, b])
        gs.append(rc(x) if g % 3 == 2 else x)
    return _case("components_%d_%s%s" % (n, "mem" if mode == MEM else "unique", "" if extend else "_noext"), "walk", gs, pat, mode=mode,
                 mask=(1 << n) - 1 if mode == MEM else 0, extend=extend, aim={"end": (n - 1, "first" if (n - 1) % 3 == 2 else "last"), "components": n})


def masked_stop(kind, dist, side, reverse, at_round, pat, tag, seed=45, extend=True):
    """a shared stretch of genomes 0 and 1 whose first n windows agree.  dist > 0: from the base behind them on genome 1 is the
    complement of genome 0 (nothing agrees any more), and an ambiguous base ("amb") or a contig start ("contig") lies dist bases
    beyond the last base of the last agreeing window.  dist = 0: the stretch goes on unchanged and the ambiguous base / contig
    start itself, right behind that window, ends the run of valid windows (the match stops there; behind a contig start it goes on
    after span - 1 invalid windows).  side "left": all of it mirrored.  Component 1 forward or reverse-complemented.
    at_round: the last agreeing window is 63 offsets from the leftmost hit"""
    offs, span = R.shape(pat)
    rng = np.random.default_rng(seed + dist + span + 2 * reverse)
    n_agree = 64 if at_round else 40                       # agreeing windows 0 .. n_agree - 1 of the stretch
    body = n_agree + span - 1
    U = rng.integers(0, 4, body + 3 * span, dtype=np.uint8)
    a, b = U.copy(), U.copy()
    if dist:
        b[body:] = other(b[body:])
    spot = body - 1 + max(dist, 1)
    f0 = rng.integers(0, 4, 35, dtype=np.uint8)
    f1 = other(f0)
    g0, g1 = np.concatenate([f0, a, f0[::-1]]), np.concatenate([f1, b, f1[::-1]])
    spot += 35
    first_window = 35
    if side == "left":
        first_window = len(g0) - 35 - span
        g0, g1, spot = g0[::-1].copy(), g1[::-1].copy(), len(g1) - 1 - spot
    invalid = [np.zeros(len(g0), bool), np.zeros(len(g1), bool)]
    contigs = [[0], [0]]
    spot_fwd = spot
    if kind == "amb":
        invalid[1][spot] = True
        g1[spot] = 0
    else:
        contigs[1] = [0, spot if side == "right" else spot + 1]
    if reverse:
        g1 = rc(g1)
        invalid[1] = invalid[1][::-1].copy()
        contigs[1] = [0] + [len(g1) - c for c in contigs[1][1:]]
    name = "masked_%s_%s_%s%d_%s_%s%s%s" % (tag[0], tag[1], kind, dist, side, "rev" if reverse else "fwd", "_round" if at_round else "", "" if extend else "_noext")
    chains = kind == "contig" and not dist
    return _case(name, "walk", [g0, g1], pat, contigs=contigs, invalid=invalid, extend=extend,
                 aim={"kind": kind, "dist": max(dist, 1), "side": side, "spot": spot_fwd, "agree": len(U) - span + 1 if chains else n_agree,
                      "holes": span - 1 if chains else 0, "window": first_window, "reverse": reverse})


def self_complementary_lead(table_seed, n_genomes=2, seed=46):
    """genome 1 reverse-complemented; the shared stretch STARTS with a window whose masked mer is its own reverse complement (even
    weight).  That window agrees on the stretch's reverse diagonal and is a same-set hit -- of the forward diagonal (equal strand
    flags).  The stretch's leftmost hit is the next window, its left walk meets that hit one offset on, and the match must still be
    made (S4: each cluster is emitted once by its leftmost hit; the oracle and mum_extend used to drop it: the match was lost)"""
    rng = np.random.default_rng(seed + n_genomes)
    pat = seed_table(16) if table_seed else solid(16)
    offs, span = R.shape(pat)
    W = rng.integers(0, 4, span, dtype=np.uint8)
    for i in range(span // 2):
        W[span - 1 - i] = 3 - W[i]
    U = np.concatenate([W, rng.integers(0, 4, 90, dtype=np.uint8)])
    f0, t0 = rng.integers(0, 4, 60, dtype=np.uint8), rng.integers(0, 4, 45, dtype=np.uint8)
    gs = [np.concatenate([f0, U, t0])]
    for g in range(1, n_genomes):
        f, t = f0 ^ np.uint8(g), t0 ^ np.uint8(g)
        x = np.concatenate([f, U, t])
        gs.append(rc(x) if g == 1 else x)
    return _case("selfrc_leads_%s_n%d" % ("table" if table_seed else "solid", n_genomes), "walk", gs, pat, aim={"window": 60, "components": n_genomes})


@functools.lru_cache(None)
def walk_cases():
    out = []
    for i, (kind, s, pat) in enumerate(walk_patterns()):
        tag = (kind, s)
        out.append(repeat_walks(tag, pat))
        out.append(gap_walks(tag, pat))
        if i % 4 == 0:
            out.append(repeat_walks(tag, pat, reverse=True))
            out.append(gap_walks(tag, pat, reverse=True))
    out.append(repeat_walks(("table", 11), seed_table(11), extend=False))
    out.append(gap_walks(("table", 11), seed_table(11), extend=False))
    # a light solid seed (span < 11: walk_round's doubling loop has its shortest form) on pairs small enough for 32 k canonical mers
    s8 = 64 - 8
    for i, rs in enumerate(((s8 - 1, s8, s8 + 1, 62), (63, 64, 65, 66))):
        out.append(repeat_walks(("solid", 8), solid(8), lengths=rs, part="_%d" % i, reverse=i == 1))
    for i, fs in enumerate(((s8 - 2, s8 - 1, s8), (s8 + 1, s8 + 2, 60), (61, 62, 63), (64, 65, 66))):
        out.append(gap_walks(("solid", 8), solid(8), offsets=fs, part="_%d" % i, reverse=i == 2))
    for tag, pat in ((("table", 11), seed_table(11)), (("spaced", 49), SPACED[("spaced", 49, 15)])):
        for residue in (0, 1, 31, 32, 33, 63):
            out += [genome_end(which, side, residue, pat, tag) for which in (0, 1, 2) for side in ("first", "last")]
    out.append(genome_end(2, "first", 0, seed_table(11), ("table", 11), extend=False))
    out += [self_complementary_lead(t, n) for t in (False, True) for n in (2, 3)]
    out += [many_components(n, mode) for n in (9, 12, 32) for mode in (MEM, UNIQUE)] + [many_components(12, MEM, extend=False)]
    for tag, pat in ((("table", 11), seed_table(11)), (("spaced", 33), SPACED[("spaced", 33, 13)])):
        span = R.shape(pat)[1]
        for kind in ("amb", "contig"):
            for dist in (0, span - 1, span, span + 1):
                for side in ("right", "left"):
                    out += [masked_stop(kind, dist, side, rev, False, pat, tag) for rev in (False, True)]
            out += [masked_stop(kind, dist, side, rev, True, pat, tag) for dist in (0, span) for side, rev in (("right", False), ("left", True))]
            out.append(masked_stop(kind, 0, "right", kind == "amb", False, pat, tag, extend=False))
    return out


# ---- caller-made patterns on genomes small enough for them -----------------------------------------------------------------------
@functools.lru_cache(None)
def pattern_cases():
    """every caller-made pattern on a pair (and a reverse-complemented pair) of genomes small enough to hold unique mers of its
    weight: 4^weight / 3 bases, at least span + 1, two substitutions in genome 1"""
    out = []
    for key, pat in list(SOLID.items()) + list(SPACED.items()) + list(SPAN49.items()):
        offs, span = R.shape(pat)
        w = len(offs)
        L = max(min(4 ** w // 3, 3000), span + 1 + w)
        for reverse in (False, True):
            for seed in range(200):
                rng = np.random.default_rng(7 * seed + span)
                S = rng.integers(0, 4, L, dtype=np.uint8)
                x = S.copy()
                if L > 4 * span:
                    x[L // 3] ^= 1
                    x[2 * L // 3] ^= 1
                if R.find([S, x], pat)["length"]:
                    break
            name = "pattern_%s%s" % ("_".join(map(str, key)), "_rev" if reverse else "")
            out.append(_case(name, "pattern", [S, rc(x) if reverse else x], pat, aim={"matches": True}))
    # without extension: one lightest, one widest, one of 64-bit keys
    out += [dict(c, name=c["name"] + "_noext", extend=False) for c in out if c["name"] in ("pattern_solid_3", "pattern_spaced_48_14_rev", "pattern_span49_31")]
    return out


# ---- the host callback seam ----------------------------------------------------------------------------------------------------------
def callback_cases():
    span = R.shape(seed_table(11))[1]
    return [junction(4096, span, True), junction(4096, 1, False, n_genomes=3), repeat_walks(("table", 11), seed_table(11)),
            repeat_walks(("spaced", 33), SPACED[("spaced", 33, 13)], reverse=True)]


FAMILIES = {"bucket": bucket_cases, "route": route_cases, "tile": tile_cases, "walk": walk_cases, "pattern": pattern_cases}


def family(name):
    return FAMILIES[name]()


def all_cases():
    return [c for f in FAMILIES for c in family(f)]
