"""Caller alignments for mauve_backbone_alignment, built to put the backbone stage on the edges of its device form:
words of 64, batches of 256 and chunks of 4096 interval-relative columns (bb_pair_gaps, bb_chunk_last), rank tiles of 4096 and
quarter-tiles of 1024 absolute columns (bb_rank), 64 grid rows of pairs.  tests/test_backbone_planted_cpu.py shows from the facts of
tests/backbone_ref.py that every case is where it was aimed and holds the oracle to that reference; tests/test_gpu_backbone_planted.py
runs them on the device.

A case: name, family, aln = (left, right, reverse, col_off, cols), gaps = the island_gap values it is run at, in this order, on one
context; aim = {island_gap: checks}; sequence (island limit cases) = (g, g + 1), which gaps must equal: both tests assert it.
A check is a tuple whose last entry says in words what it is for:
  ("run", iv, a, b, first, last, n, island, why)           the pair has this gap run, and it is / is not an island
  ("region", iv, a, b, first, last, open, reasons, why)    the pair has this gap region, exactly once, open for these reasons
  ("regions", iv, a, b, count, why)                        the pair has this many gap regions
  ("chunks", iv, a, b, first, count, why)                  the region that starts at `first` lies in this many chunks
  ("segments", count, why)                                 the whole alignment has this many segments
  ("masks", iv, col, [masks], why)                         the segments over this column have these genome sets
  ("islands", count, why)                                  the whole alignment has this many islands
  ("pair_islands", iv, a, b, count, why)                   the pair has this many islands
  ("edge", what, end, absolute column, why)                a segment ("seg") or island ("isl") starts ("first") or ends ("last") here
Masks below: with the pair (0, 1) under test, BOTH = 3, A = 1 (only genome 0), B = 2 (only genome 1), Z = 4 (a third genome alone:
a neither-column of the pair)."""
import functools

import numpy as np

BOTH, A, B, Z = 3, 1, 2, 4
CHUNK = 4096
LIMITS = (0, 1, 2, 3, 20, 62, 63, 64, 65, 127, 128, 500, 4096)
FAMILIES = ("limit", "ownership", "startup", "components", "coordinates")


def interval(pieces, N, rev=None, base=1000):
    """pieces: (mask, count) in column order -> (left, right, reverse, cols) of one interval; genome g lies at base * (g + 1) ..."""
    cols = np.concatenate([np.full(n, m, np.uint32) for m, n in pieces if n > 0])
    left, right = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for g in range(N):
        cnt = int(np.count_nonzero(cols >> np.uint32(g) & 1))
        if cnt:
            left[g] = base * (g + 1) + 7 * g + 1
            right[g] = left[g] + cnt - 1
    rv = np.zeros(N, np.int8) if rev is None else np.array(rev, np.int8)
    return left, right, rv * (left != 0), cols


def alignment(ivs):
    off = np.concatenate([[0], np.cumsum([len(i[3]) for i in ivs])]).astype(np.int64)
    return np.array([i[0] for i in ivs]), np.array([i[1] for i in ivs]), np.array([i[2] for i in ivs], np.int8), off, np.concatenate([i[3] for i in ivs])


def case(name, family, ivs, aim, **kw):
    return dict(name=name, family=family, aln=alignment(ivs), gaps=tuple(aim), aim=aim, **kw)


def at(pieces):
    """first column of every piece"""
    return np.concatenate([[0], np.cumsum([n for _, n in pieces])]).tolist()


# ------------------------------------------------------------------------------------------------------------------ island limit
def _limit_cases():
    out = []
    for g in LIMITS:
        lim = "a run of %d is no island and one of %d is, at island_gap %d" % (g, g + 1, g)
        if g <= 61:                                           # (a) each run inside one full word that starts and ends with a both-column
            p = [(BOTH, 1), (A, g), (BOTH, 63 - g), (BOTH, 1), (B, g + 1), (BOTH, 62 - g), (BOTH, 10)]
            aim = {g: [("run", 0, 0, 1, 65, 65 + g, g + 1, True, lim + " (inside one full word: the has_run path)"),
                       ("region", 0, 0, 1, 65, 65 + g, True, ("island",), "the run of %d opens its region" % (g + 1)), ("islands", 1, lim)],
                   g + 1: [("run", 0, 0, 1, 65, 65 + g, g + 1, False, "the run of %d is no island at island_gap %d" % (g + 1, g + 1)), ("islands", 0, lim)]}
            if g:
                aim[g] += [("run", 0, 0, 1, 1, g, g, False, lim), ("region", 0, 0, 1, 1, g, False, (), "the run of %d leaves its region closed" % g)]
            out.append(case("limit_word_g%d" % g, "limit", [interval(p, 2)], aim, sequence=(g, g + 1)))
        # (b) the run of g + 1 across column 63 | 64, 255 | 256, 4095 | 4096 of an interval each, the run of g across the same border 2 chunks on
        ivs, aim = [], {g: [], g + 1: []}
        for k, X in enumerate((64, 256, 4096)):
            s1 = X - max(1, min((g + 1) // 2, X - 1))
            s0 = X + 2 * CHUNK - max(1, g // 2)
            p = [(BOTH, s1), (A, g + 1), (BOTH, s0 - s1 - g - 1), (B, g), (BOTH, 77)]
            ivs.append(interval(p, 2, rev=(k == 1, k == 2)))
            aim[g] += [("run", k, 0, 1, s1, s1 + g, g + 1, True, lim + " (across column %d | %d)" % (X - 1, X)),
                       ("region", k, 0, 1, s1, s1 + g, True, ("island",), "the region of the run across %d | %d is reported once" % (X - 1, X))]
            aim[g + 1] += [("run", k, 0, 1, s1, s1 + g, g + 1, False, "no island at island_gap %d" % (g + 1))]
            if g:
                aim[g] += [("run", k, 0, 1, s0, s0 + g - 1, g, False, lim + " (across column %d | %d)" % (X + 2 * CHUNK - 1, X + 2 * CHUNK))]
        aim[g].append(("islands", 3, lim))
        aim[g + 1].append(("islands", 0, lim))
        out.append(case("limit_border_g%d" % g, "limit", ivs, aim, sequence=(g, g + 1)))
        # (c) neither-columns of a third genome inside both runs: the count stays, the span grows, the word is not a fast-path word
        def holed(mask, n):
            return [(Z, 2), (mask, n - n // 2), (Z, 5), (mask, n // 2), (Z, 2)]
        p = [(BOTH, 3)] + holed(A, g + 1) + [(BOTH, 70)] + holed(B, g) + [(BOTH, 9)]
        c = at(p)
        aim = {g: [("run", 0, 0, 1, c[2], c[2] + g + (5 if g else 0), g + 1, True, lim + ": neither-columns inside the run do not count")],
               g + 1: [("run", 0, 0, 1, c[2], c[2] + g + (5 if g else 0), g + 1, False, "no island at island_gap %d" % (g + 1)),
                       ("pair_islands", 0, 0, 1, 0, "neither run is an island at island_gap %d" % (g + 1))]}
        aim[g].append(("pair_islands", 0, 0, 1, 1, lim))
        if g:
            aim[g + 1].append(("run", 0, 0, 1, c[8], c[8] + g - 1 + (5 if g > 1 else 0), g, False, "the run of %d is no island at island_gap %d either" % (g, g + 1)))
            aim[g].append(("run", 0, 0, 1, c[8], c[8] + g - 1 + (5 if g > 1 else 0), g, False, lim + ": neither-columns inside the run do not count"))
        out.append(case("limit_holes_g%d" % g, "limit", [interval(p, 3)], aim, sequence=(g, g + 1)))
        # (d) only-a x g directly followed by only-b x g: two runs, no island, a closed region
        if g:
            p = [(BOTH, 10), (A, g), (B, g), (BOTH, 20)]
            aim = {g: [("run", 0, 0, 1, 10, 9 + g, g, False, "only-a x %d then only-b x %d are two runs of %d, not one of %d" % (g, g, g, 2 * g)),
                       ("run", 0, 0, 1, 10 + g, 9 + 2 * g, g, False, "the only-b run of %d is a run of its own" % g),
                       ("region", 0, 0, 1, 10, 9 + 2 * g, False, (), "a region of two runs of %d is closed at island_gap %d" % (g, g)),
                       ("islands", 0, "no island"), ("masks", 0, 10 + g, [3], "one segment goes through the closed region")]}
            out.append(case("limit_two_runs_g%d" % g, "limit", [interval(p, 2)], aim))
    # (e) the largest island_gap: accepted, nothing is an island
    p = [(BOTH, 50), (A, 5000), (BOTH, 10), (B, 61), (BOTH, 3)]
    big = 2 ** 31 - 1
    out.append(case("limit_largest_gap", "limit", [interval(p, 2)],
                    {big: [("islands", 0, "island_gap 2^31 - 1 is accepted and nothing is an island"), ("masks", 0, 2000, [3], "one segment over everything")]}))
    return out


# --------------------------------------------------------------------------------------------------------------- region ownership
def _ownership_cases():
    out = []
    for F in (4095, 4096, 4097):                              # an island-holding region that starts on / next to the chunk border
        p = [(BOTH, F), (A, 30), (BOTH, 9000 - F - 30)]
        out.append(case("own_first_%d" % F, "ownership", [interval(p, 2)],
                        {20: [("region", 0, 0, 1, F, F + 29, True, ("island",), "a region whose first column is %d belongs to one chunk only" % F), ("islands", 1, "one island")]}))
    for L in (4094, 4095, 4096):                              # ... that ends there: its closing both-column is at 4095, 4096, 4097
        p = [(BOTH, L - 29), (B, 30), (BOTH, 9000 - L - 1)]
        out.append(case("own_last_%d" % L, "ownership", [interval(p, 2)],
                        {20: [("region", 0, 0, 1, L - 29, L, True, ("island",), "a region closed by the both-column %d is reported once" % (L + 1)), ("islands", 1, "one island")]}))
    for span in (2, 3, 66):                                   # regions over several chunks: the chunks behind the first find `skipping` in the bytes
        last = 4000 + (span - 1) * CHUNK + 10
        p = [(BOTH, 4000), (A, 30), (B, 7), (A, last - 4000 - 36), (BOTH, 300)]
        out.append(case("own_span_%d" % span, "ownership", [interval(p, 2)],
                        {20: [("region", 0, 0, 1, 4000, last, True, ("island",), "a region over %d chunks is reported once, by the chunk it starts in" % span),
                              ("regions", 0, 0, 1, 1, "one region"), ("islands", 2, "its two long runs"), ("chunks", 0, 0, 1, 4000, span, "the region spans %d chunks" % span)]}))
    p = [(BOTH, 5), (A, 3), (BOTH, 2), (B, 25), (BOTH, 40)]
    out.append(case("own_two_in_a_word", "ownership", [interval(p, 2)],
                    {20: [("region", 0, 0, 1, 5, 7, False, (), "the first of two regions in one word stays closed"), ("region", 0, 0, 1, 10, 34, True, ("island",), "the second is open"),
                          ("masks", 0, 6, [3], "the segment goes through the closed region")],
                     2: [("region", 0, 0, 1, 5, 7, True, ("island",), "both regions of the word are open"), ("region", 0, 0, 1, 10, 34, True, ("island",), "both regions of the word are open")]}))
    p = [(BOTH, 4090), (A, 10), (BOTH, 1), (B, 10), (BOTH, 500)]
    out.append(case("own_close_then_open", "ownership", [interval(p, 2)],
                    {3: [("region", 0, 0, 1, 4090, 4099, True, ("island",), "the region of chunk 0 closes in the first word of chunk 1"),
                         ("region", 0, 0, 1, 4101, 4110, True, ("island",), "the region right behind it is chunk 1's own"), ("regions", 0, 0, 1, 2, "each once"), ("islands", 2, "each once")]}))
    return out


# ----------------------------------------------------------------------------------------------------------------- start-up state
def _startup_cases():
    out = []
    for z in (0, 1, 5000):                                    # the pair's first column is one-sided: leading, open at any island_gap
        p = [(Z, z), (A, 1), (BOTH, 100), (Z, 3)]
        aim = {g: [("region", 0, 0, 1, z, z, True, ("leading",), "a one-sided first column behind %d neither-columns is a leading region, open at any island_gap" % z),
                   ("masks", 0, z, [], "no segment over the leading column"), ("masks", 0, z + 1, [3], "the segment starts behind it")] for g in (0, 20, 500)}
        aim[0][0] = ("region", 0, 0, 1, z, z, True, ("island", "leading"), "leading, and an island at island_gap 0")
        out.append(case("start_leading_z%d" % z, "startup", [interval(p, 3)], aim))
    p = [(BOTH, 100), (B, 1), (Z, 50)]
    out.append(case("start_trailing", "startup", [interval(p, 3)],
                    {20: [("region", 0, 0, 1, 100, 100, True, ("trailing",), "a one-column overhang followed by neither-columns to the interval's end is a trailing region"),
                          ("masks", 0, 99, [3], "the segment ends in front of it"), ("masks", 0, 100, [], "nothing over the overhang")]}))
    p = [(A, 10), (B, 10), (A, 5)]
    out.append(case("start_never_both", "startup", [interval(p, 2)],
                    {20: [("region", 0, 0, 1, 0, 24, True, ("leading", "trailing"), "a pair without a both-column is one open region: never joined"), ("islands", 0, "no island")]}))
    for k in (1, 63, 64, 65):                                 # k chunks without a column of the pair in front of the chunk under test
        for front in ("both", "one"):
            for first in ("one", "both"):
                p = [(BOTH, 100), (A, 2 if front == "one" else 0)]
                p += [(Z, (k + 1) * CHUNK - sum(n for _, n in p))]
                p += [(A, 25), (BOTH, 50)] if first == "one" else [(BOTH, 50)]
                s = (k + 1) * CHUNK
                why = "%d chunks without a column of the pair, behind a %s-column, in front of a chunk that starts with a %s-column" % (k, front, first)
                if front == "both" and first == "one":
                    a20 = [("region", 0, 0, 1, s, s + 24, True, ("island",), why + ": the region is that chunk's own")]
                elif front == "one" and first == "one":
                    a20 = [("region", 0, 0, 1, 100, s + 24, True, ("island",), why + ": the region began %d chunks earlier" % (k + 1)), ("regions", 0, 0, 1, 1, why)]
                elif front == "one":
                    a20 = [("region", 0, 0, 1, 100, 101, False, (), why + ": the region of two columns closes there")]
                else:
                    a20 = [("regions", 0, 0, 1, 0, why + ": no region at all")]
                a1 = [("region", 0, 0, 1, 100, 101, True, ("island",), why)] if (front, first) == ("one", "both") else list(a20)
                out.append(case("start_back_%d_%s_%s" % (k, front, first), "startup", [interval(p, 3)], {20: a20, 1: a1}))
    for n in (CHUNK, CHUNK + 1):                              # an interval of exactly one chunk, and of one column more
        p = [(BOTH, 4090), (A, 3), (BOTH, 3), (B, n - CHUNK)]
        aim = [("region", 0, 0, 1, 4090, 4092, True, ("island",), "an interval of %d columns" % n), ("masks", 0, 4095, [3], "the last segment reaches column 4095")]
        if n > CHUNK:
            aim.append(("region", 0, 0, 1, 4096, 4096, True, ("island", "trailing"), "the only column of the second chunk is a trailing region"))
        out.append(case("start_interval_%d" % n, "startup", [interval(p, 2)], {0: aim}))
    return out


# --------------------------------------------------------------------------------------------------------------------- components
def _component_cases():
    out = []
    # 0-1, 1-2, 2-3 joined, every other pair never in one column: transitivity makes {0, 1, 2, 3}
    p = [(3, 1), (6, 1), (12, 1)] * 30
    out.append(case("comp_chain", "components", [interval(p, 4)],
                    {3: [("masks", 0, 45, [15], "0-1, 1-2 and 2-3 joined and no other pair: one component of all four"),
                         ("region", 0, 0, 2, 0, 89, True, ("leading", "trailing"), "0-2 is never joined"), ("region", 0, 0, 3, 0, 89, True, ("leading", "trailing"), "0-3 is never joined"),
                         ("region", 0, 1, 3, 0, 89, True, ("leading", "trailing"), "1-3 is never joined"), ("region", 0, 0, 1, 43, 43, False, (), "0-1 is joined at column 45"),
                         ("region", 0, 2, 3, 43, 43, False, (), "2-3 is joined at column 45")]}))
    # {0, 1, 2} through 0-1, 1-2 up to column 24 and through 0-1, 0-2 from column 25: one segment; the region of 0-2 closes at 24, that of 1-2 opens at 25
    p = [(7, 20), (3, 1), (1, 1), (3, 1), (1, 1), (6, 1), (5, 1), (4, 1), (5, 1), (4, 1), (7, 20)]
    out.append(case("comp_same_set_other_pairs", "components", [interval(p, 3, rev=(0, 1, 0))],
                    {3: [("region", 0, 0, 2, 20, 24, True, ("island",), "the open region of 0-2 closes at column 24"), ("region", 0, 1, 2, 25, 28, True, ("island",), "that of 1-2 opens at column 25"),
                         ("masks", 0, 24, [7], "all three through 0-1 and 1-2"), ("masks", 0, 25, [7], "all three through 0-1 and 0-2"), ("segments", 1, "the same genome set through other pairs is one segment")]}))
    # component {0, 1, 3} over columns 10 .. 18 where genome 1 has no base: reported as {0, 3}
    p = [(15, 10), (4, 5), (9, 3), (4, 1), (15, 10)]
    out.append(case("comp_member_without_base", "components", [interval(p, 4, rev=(1, 0, 0, 1))],
                    {4: [("masks", 0, 9, [15], "all four in front"), ("masks", 0, 12, [9], "genome 1 belongs to the component and has no base in it: dropped from the set"),
                         ("masks", 0, 19, [15], "all four behind"), ("segments", 3, "three segments")]}))
    # component {0, 1} over columns 10 .. 22 where only genome 0 has bases: no segment
    p = [(7, 10), (4, 5), (1, 3), (4, 5), (7, 10)]
    out.append(case("comp_left_with_one", "components", [interval(p, 3)],
                    {4: [("masks", 0, 11, [], "a component left with one genome that has bases is no segment"), ("region", 0, 0, 1, 15, 17, False, (), "0-1 stays joined"), ("segments", 2, "two segments")]}))
    # 12 genomes: 66 pairs on 64 grid rows; pairs 63, 64, 65 are (9, 10), (9, 11), (10, 11)
    full = (1 << 12) - 1
    p = [(full, 100), (full & ~(1 << 10), 30), (full, 70), (full & ~(1 << 11), 30), (full, 70), (full & ~(1 << 9), 30), (full, 3760), (full & ~(1 << 10), 30), (full, 900)]
    out.append(case("comp_66_pairs", "components", [interval(p, 12, rev=[g % 3 == 1 for g in range(12)], base=100000)],
                    {20: [("region", 0, 9, 10, 100, 129, True, ("island",), "pair 63 of 66"), ("region", 0, 9, 10, 300, 329, True, ("island",), "pair 63 of 66"),
                          ("region", 0, 9, 11, 200, 229, True, ("island",), "pair 64 of 66"), ("region", 0, 10, 11, 4090, 4119, True, ("island",), "pair 65 of 66, across the chunk border"),
                          ("masks", 0, 110, [full & ~(1 << 10)], "genome 10 is out"), ("islands", 44, "11 pairs per stretch")]}))
    # 32 genomes: an interval of genomes 30 and 31 alone with one island, and one of all 32 (496 pairs)
    allg = 0xFFFFFFFF
    p1 = [(3 << 30, 70), (1 << 31, 25), (3 << 30, 40)]
    p2 = [(allg, 40), (allg & ~(1 << 31), 25), (allg, 30), (allg & ~1, 2), (allg, 30)]
    out.append(case("comp_32_genomes", "components", [interval(p1, 32, rev=[0] * 31 + [1]), interval(p2, 32, base=200000)],
                    {20: [("region", 0, 30, 31, 70, 94, True, ("island",), "the one island of pair (30, 31)"), ("islands", 32, "one, and 31 in the interval of all genomes"),
                          ("masks", 1, 50, [allg >> 1], "genome 31 is out"), ("masks", 1, 96, [allg], "a gap of two joins")]}))
    return out


# -------------------------------------------------------------------------------------------------------------------- coordinates
def _coordinate_cases():
    out = []
    for front in (1, 4095, 4096):                             # the planted interval starts at absolute column front
        for rev in ((0, 0), (1, 0), (0, 1), (1, 1)):
            total = 3 * CHUNK                                 # the last segment ends on the array's last column: its query is n_cols
            isl = [(5095, A), (5121, B), (8167, B), (8193, A)]                       # absolute first columns of islands of 25
            p, c = [], front
            for s, m in isl:
                p += [(BOTH, s - c), (m, 25)]
                c = s + 25
            p.append((BOTH, total - c))
            name = "coord_front%d_%d%d" % (front, rev[0], rev[1])
            aim = [("edge", "isl", "last", 5119, "an island ends on absolute column 5119 = 4096 + 1023"), ("edge", "seg", "first", 5120, "a segment of one column at 5120"),
                   ("edge", "seg", "last", 5120, "a segment of one column at 5120"), ("edge", "isl", "first", 5121, "an island starts at 5121"),
                   ("edge", "isl", "last", 8191, "an island ends at 8191"), ("edge", "seg", "first", 8192, "a segment of one column at 8192"),
                   ("edge", "seg", "last", 8192, "a segment of one column at 8192"), ("edge", "isl", "first", 8193, "an island starts at 8193"),
                   ("edge", "seg", "last", total - 1, "the last segment ends on the last column of an array of 3 x 4096"), ("islands", 4, "four islands"), ("segments", 6, "the front interval's and five")]
            out.append(case(name, "coordinates", [interval([(BOTH, front)], 2, base=50), interval(p, 2, rev=rev, base=70000)], {20: aim}))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = _limit_cases() + _ownership_cases() + _startup_cases() + _component_cases() + _coordinate_cases()
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def family(name):
    return [c for c in all_cases() if c["family"] == name]
