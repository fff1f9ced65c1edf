"""Planted genome sets for the LCB extension (csrc/extend_dev.hip, extend_lcbs of csrc/pipeline.cpp): pieces of
exactly one seed length, separators on word, wave and block edges, matches that the separator has to cut, rounds that keep, drop
and renumber, LCB weights on the limit, kept matches slipped into anchor lists of 255 .. 513 at block edges, recursion gaps
of exactly min_recursive_gap, 2 .. 32 genomes, and the inputs that must keep the host form.

A case is a dict: name, family, N, genomes (uint8 codes), params (seed_weight, lcb_weight, max_extension_iters, collinear,
lcb_scoring, recursive, min_recursive_gap), contigs / invalid (None, or what set_genomes takes), pos (per genome: name -> (1-based
start, length, reverse?) of every shared stretch), device (may the device form take it?), full (also run gapped, against the
oracle) and aim -- what the case was planted for, as data that tests/test_extend_cpu.py checks against tests/extend_ref.py's
records and the geometry below, never against the product.

Genomes are built from LCB blocks (300 shared random bases, one root match each at seed weight 15), spacers (random bases,
unrelated between genomes: the pieces) and planted stretches inside the spacers.  The stretch length picks the round that can
first see it: the rank-0 seeds of weight 13 / 11 / 9 / 7 span 19 / 15 / 13 / 9 bases.  Spaced seeds find a stretch one or two bases
short of the span a round early when a flank base agrees by chance, so the 6 bases on each side of every shared stretch are made
to differ between genome 0 and genome 1 (every pattern in use has a care position in any 6 consecutive offsets: asserted in
tests/test_extend_cpu.py from the seed table).

The device form's geometry, as csrc/extend_dev.hip has it (the tests state it; they do not read it from the library):"""
import functools

import numpy as np

SEPARATORS = 1          # one separator base (code 0) between two pieces of a virtual genome, none behind the last piece
WORD = 32               # bases per packed word
WAVE = 64               # bases per wave of ext_gather (two words by ballots)
GATHER_BLOCK = 256      # bases per block of ext_gather
MERGE_BLOCK = 256       # threads per block of ext_merge / ext_count_rec / ext_flag_rec (one anchor each)
TINY_MAX = 9216         # windows up to which the seed pass over the virtual genomes is one workgroup (tiny_join)
FLANK = 6
ROOT_W = 15
SPAN = {15: 21, 13: 19, 11: 15, 9: 13, 7: 9, 6: 9, 5: 7}      # rank-0 seed spans (asserted against the seed table in the CPU file)
ROUND_LEN = (19, 15, 13, 9)                                   # the stretch length that round k (from seed weight 15) first sees
BLOCK = 300


def pieces_K(pieces):
    """K of a round: the largest piece count of any genome (vstart is padded to K + 1 entries per genome)"""
    return max(len(p) for p in pieces)


def rc(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


class Builder:
    """genomes from segments: ("s", n) a spacer of n random bases; (name, +1 | -1) the shared stretch `name`, forward or reverse
    complemented; ("lit", codes) fixed bases that are neither; ("tail", name, +1 | -1, k) the stretch without the first k bases of
    that copy -- they are the last k bases of what stands in front of it, so the stretch is there whole, overlapping its neighbour"""

    def __init__(self, N, seed):
        self.N, self.rng, self.content, self.layouts = N, np.random.default_rng(seed), {}, [None] * N

    def shared(self, name, n):
        self.content[name] = self.rng.integers(0, 4, n, dtype=np.uint8)
        return self.content[name]

    def differ(self, a, ia, b, ib, n=FLANK, reverse=False):
        """content b[ib ...] made to mismatch content a[ia ...] over n bases (slices given as start offsets; negative: from the
        end); reverse: b is read reverse-complemented against a, so b's slice is the complement, reversed"""
        A, Bc = self.content[a], self.content[b]
        sa = A[ia:ia + n] if ia >= 0 else A[len(A) + ia:len(A) + ia + n]
        want = (sa + 1) % 4
        if reverse:
            want = rc(want)
        lo = ib if ib >= 0 else len(Bc) + ib
        Bc[lo:lo + n] = want

    def genome(self, g, segs):
        self.layouts[g] = list(segs)

    def all(self, segs, but=()):
        for g in range(self.N):
            if g not in but:
                self.layouts[g] = list(segs)

    def build(self):
        gen, free, pos = [], [], []
        for g in range(self.N):
            parts, fr, p, at = [], [], {}, 0
            for seg in self.layouts[g]:
                if seg[0] == "s":
                    x, f = self.rng.integers(0, 4, seg[1], dtype=np.uint8), True
                elif seg[0] == "lit":
                    x, f = np.asarray(seg[1], np.uint8), False
                elif seg[0] == "tail":
                    c = self.content[seg[1]]
                    x, f = (c if seg[2] > 0 else rc(c))[seg[3]:], False
                    assert np.array_equal(np.concatenate(parts)[-seg[3]:], (c if seg[2] > 0 else rc(c))[:seg[3]])
                    p[seg[1]] = (at + 1 - seg[3], len(c), seg[2] < 0)
                else:
                    c = self.content[seg[0]]
                    x, f = (c if seg[1] > 0 else rc(c)), False
                    assert seg[0] not in p, "a shared stretch once per genome"
                    p[seg[0]] = (at + 1, len(c), seg[1] < 0)
                parts.append(x)
                fr.append(np.full(len(x), f))
                at += len(x)
            gen.append(np.concatenate(parts).astype(np.uint8))
            free.append(np.concatenate(fr))
            pos.append(p)
        self._flanks(gen, free, pos)
        return gen, pos

    @staticmethod
    def _flanks(gen, free, pos):
        """the FLANK bases on each side of every stretch that genome 0 and genome 1 share are made to disagree (by the strand
        relation of the two copies), by changing spacer bases only: genome 0's where genome 1 has none there, then genome 1's"""
        if len(gen) < 2:
            return
        pairs = []
        for name, (s1, n, r1) in pos[1].items():
            if name not in pos[0]:
                continue
            s0, _, r0 = pos[0][name]
            s0 -= 1; s1 -= 1
            rel = r0 != r1
            for k in range(FLANK):
                for right1 in (False, True):
                    p1 = s1 + n + k if right1 else s1 - 1 - k
                    right0 = right1 != rel
                    p0 = s0 + n + k if right0 else s0 - 1 - k
                    if 0 <= p1 < len(gen[1]) and 0 <= p0 < len(gen[0]):
                        pairs.append((p0, p1, rel))
        for first in (True, False):
            forbid = {}
            for p0, p1, rel in pairs:
                if first and not free[1][p1] and free[0][p0]:
                    forbid.setdefault(p0, set()).add(int(3 - gen[1][p1]) if rel else int(gen[1][p1]))
                if not first and free[1][p1]:
                    forbid.setdefault(p1, set()).add(int(3 - gen[0][p0]) if rel else int(gen[0][p0]))
            x = gen[0] if first else gen[1]
            for p, bad in forbid.items():
                if int(x[p]) in bad:
                    x[p] = min(v for v in range(4) if v not in bad)


def _case(name, family, b, aim, device=True, full=False, contigs=None, invalid=None, **params):
    gen, pos = b.build()
    p = {"seed_weight": ROOT_W, "lcb_weight": -1, "max_extension_iters": 4, "collinear": 0, "lcb_scoring": 0, "recursive": 0, "min_recursive_gap": 200}
    p.update(params)
    return {"name": name, "family": family, "N": b.N, "genomes": gen, "pos": pos, "params": p, "aim": aim, "device": device, "full": full,
            "contigs": contigs, "invalid": invalid}


def _blocks(b, names, n=BLOCK):
    for x in names:
        b.shared(x, n)


def found(name, rnd, how, **kw):
    return dict(name=name, round=rnd, how=how, **kw)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def _exact_piece(k, delta, N=2):
    """a piece of span + delta bases between two one-anchor LCBs in every genome (other LCBs in genome 1), filled by a planted
    stretch; every block an LCB of its own (alternating strands in the last genome); lcb_weight = the stretch's weight, so it is
    kept as an LCB of its own exactly at the limit"""
    L = ROUND_LEN[k] + delta
    b = Builder(N, 100 + 10 * k + delta + 1000 * N)
    _blocks(b, "ABCD")
    b.shared("P", L)
    b.differ("A", -FLANK, "C", -FLANK)                       # in front of P: A's end in genome 0, C's end in the last genome
    b.differ("B", 0, "D", -FLANK, reverse=True)              # behind P: B's head in genome 0, the head of rc(D) in the last genome
    b.all([("s", 40), ("A", 1), ("P", 1), ("B", 1), ("s", 70), ("C", 1), ("s", 50), ("D", 1), ("s", 45)])
    b.genome(1, [("s", 33), ("C", 1), ("P", 1), ("D", -1), ("s", 61), ("B", -1), ("s", 44), ("A", 1), ("s", 52)])
    aim = {"lcbs_root": 4}
    if delta < 0:
        aim.update(absent=["P"], no_piece=[(g, k, "P") for g in range(N)], rounds=k + 1)
    else:
        aim.update(found=[found("P", k, "new")], piece=[(g, k, "P", 0, 0) for g in range(N)])
    return _case("piece_%+d_round%d_n%d" % (delta, k, N), "pieces", b, aim, lcb_weight=L * N if delta >= 0 else (L + 1) * N,
                 max_extension_iters=k + 1)


def _ends_case(lead, tail):
    """a stretch in the piece at base 1 and one in the piece that ends on the genome's last base; lead / tail = False: genome 0
    begins / ends with an LCB and has no such piece"""
    b = Builder(2, 300 + 2 * lead + tail)
    _blocks(b, "AB")
    b.shared("P", 19); b.shared("Q", 20)
    g0 = ([("P", 1), ("s", 30)] if lead else []) + [("A", 1), ("s", 60)] + ([] if lead else [("P", 1), ("s", 20)]) + \
         ([] if tail else [("Q", 1), ("s", 25)]) + [("B", -1)] + ([("s", 31), ("Q", 1)] if tail else [])
    b.genome(0, g0)
    b.genome(1, [("P", 1), ("s", 37), ("A", 1), ("s", 50), ("B", 1), ("s", 41), ("Q", 1)] if lead and tail else
                [("s", 9), ("A", 1), ("s", 20), ("P", 1), ("s", 37), ("Q", 1), ("s", 50), ("B", 1), ("s", 41)])
    aim = {"found": [found("P", 0, None), found("Q", 0, None)], "lcbs_root": 2,
           "piece": ([(0, 0, "P", 0, 30)] if lead else []) + ([(0, 0, "Q", 31, 0)] if tail else []),
           "first_piece_at": [(0, 0, 1 if lead else None)], "last_piece_ends": [(0, 0, tail)]}
    return _case("ends_lead%d_tail%d" % (lead, tail), "pieces", b, aim, lcb_weight=38)


def _lcb_border(rev, many):
    """P ends on the last base in front of LCB X of genome 0, Q starts on the first base behind it; X is forward or reverse in
    genome 1 and has one anchor or three (30-base blocks with 6 disagreeing bases between them).  In genome 1 both stretches lie
    inside spacers."""
    b = Builder(2, 400 + 2 * rev + many)
    _blocks(b, "AB")
    names = ["X0", "X1", "X2"] if many else ["X0"]
    for x in names:
        b.shared(x, BLOCK if not many else 120)
    b.shared("P", 19); b.shared("Q", 20)
    X = []
    for i, x in enumerate(names):
        X += ([("s", FLANK)] if i else []) + [(x, 1)]
    Xr = []
    for i, x in enumerate(reversed(names)):
        Xr += ([("s", FLANK)] if i else []) + [(x, -1)]
    b.genome(0, [("s", 30), ("A", 1), ("s", 40), ("P", 1)] + X + [("Q", 1), ("s", 35), ("B", 1), ("s", 20)])
    o = 1 if rev else -1                                           # (A and B on the other strand than X: three LCBs)
    b.genome(1, [("s", 30), ("B", o), ("s", 20), ("P", 1), ("s", 25)] + (Xr if rev else X) + [("s", 22), ("Q", 1), ("s", 30), ("A", o), ("s", 20)])
    aim = {"found": [found("P", 0, None), found("Q", 0, None)], "touch": [(0, "P", "X0", "front"), (0, "Q", names[-1], "behind")],
           "lcb_of": [("X0", names[-1], len(names), rev)], "lcbs_root": 3}
    return _case("lcb_border_%s_%s" % ("rev" if rev else "fwd", "many" if many else "one"), "pieces", b, aim, lcb_weight=38)


def _separator_at(v, g_edge):
    """genome g_edge: piece 0 of exactly v bases (so the first separator sits at virtual position v), P on its last bases, Q on the
    first bases of piece 1; in the other genome both lie inside spacers"""
    b = Builder(2, 500 + v + 7 * g_edge)
    _blocks(b, "ABC")
    b.shared("P", 19); b.shared("Q", 19)
    edge = [("s", v - 19), ("P", 1), ("A", 1), ("Q", 1), ("s", 50), ("B", -1 if g_edge else 1), ("s", 44), ("C", 1), ("s", 30)]
    other = [("s", 41), ("P", 1), ("s", 28), ("B", 1 if g_edge else -1), ("s", 37), ("A", 1), ("s", 23), ("Q", 1), ("s", 30), ("C", 1), ("s", 30)]
    b.genome(g_edge, edge)
    b.genome(1 - g_edge, other)
    aim = {"found": [found("P", 0, None), found("Q", 0, None)], "sep": [(g_edge, 0, v)], "piece": [(g_edge, 0, "P", v - 19, 0)],
           "piece_starts_with": [(g_edge, 0, "Q")]}
    return _case("separator_at_%d_g%d" % (v, g_edge), "pieces", b, aim, lcb_weight=38)


def _total(T):
    """genome 0's virtual length in round 0 is exactly T bases (the last word, the `w0 + lane < dst_words` guard); P ends on the
    virtual genome's last base"""
    b = Builder(2, 600 + T)
    _blocks(b, "AB")
    b.shared("P", 19); b.shared("Q", 19)
    a, c = 40, 50
    last = T - 2 - a - c                                           # three pieces, two separators
    b.genome(0, [("s", a), ("A", 1), ("s", c - 19), ("Q", 1), ("B", -1), ("s", last - 19), ("P", 1)])
    b.genome(1, [("s", 35), ("A", 1), ("s", 30), ("Q", 1), ("s", 20), ("P", 1), ("s", 27), ("B", 1), ("s", 33)])
    aim = {"found": [found("P", 0, None), found("Q", 0, None)], "total": [(0, 0, T)], "npieces": [(0, [3, 3])]}
    return _case("total_%d" % T, "pieces", b, aim, lcb_weight=38)


def _unequal_pieces():
    """genome 0 has one piece (it begins with an LCB and its blocks abut, 6 disagreeing bases apart), genome 1 has nine: K = 9;
    P lies in genome 1's last piece, Q (a second case) in its first"""
    out = []
    for which in ("last", "first"):
        b = Builder(2, 700 + (which == "first"))
        names = ["B%d" % i for i in range(8)]
        _blocks(b, names, 120)
        b.shared("P", 19)
        g0 = []
        for i, x in enumerate(names):
            g0 += [(x, 1), ("s", FLANK)]
        b.genome(0, g0 + [("s", 40), ("P", 1), ("s", 30)])
        g1 = [("s", 30)] + ([("P", 1), ("s", 25)] if which == "first" else [])
        for i, x in enumerate(names):
            g1 += [(x, 1 if i % 2 == 0 else -1), ("s", 30 + i)]
        b.genome(1, g1 + ([("P", 1), ("s", 21)] if which == "last" else []))
        aim = {"found": [found("P", 0, None)], "npieces": [(0, [1, 9])],
               "in_piece": [(1, 0, "P", 8 if which == "last" else 0)]}
        out.append(_case("unequal_pieces_%s" % which, "pieces", b, aim, lcb_weight=38))
    return out


SEPARATOR_RULE_SEED = {(3, 0, 2): 2003}                                           # (k, rev, N) -> a seed other than the default, where chance matches of the light seeds met the planted ones


def _separator_rule(k, rev, N):
    """genome 0: ... X . B2 . Y ..., the others: ... X a Y ... with B2 elsewhere and a = A, the separator's code (the last genome
    holds the copy reverse-complemented when rev).  In virtual coordinates X and Y lie on one diagonal, span + 1 windows apart:
    two matches, unless the separator's flag is lost"""
    L = ROUND_LEN[k]
    b = Builder(N, SEPARATOR_RULE_SEED.get((k, rev, N), 800 + 10 * k + rev + 100 * N))
    _blocks(b, ["B1", "B2", "B3"])
    b.shared("X", L); b.shared("Y", L)
    b.content["B2"][0] = 1 + b.content["B2"][0] % 3               # B2[0] != A, B2[-1] != A
    b.content["B2"][-1] = 1 + b.content["B2"][-1] % 3
    lit = ("lit", np.array([0], np.uint8))
    b.all([("s", 30), ("B1", 1), ("s", 40), ("X", 1), lit, ("Y", 1), ("s", 45), ("B3", 1), ("s", 38), ("B2", -1), ("s", 30)])
    b.genome(0, [("s", 30), ("B1", 1), ("s", 40), ("X", 1), ("B2", 1), ("Y", 1), ("s", 45), ("B3", 1), ("s", 30)])
    if rev:
        b.genome(N - 1, [("s", 30), ("B1", 1), ("s", 40), ("Y", -1), ("lit", np.array([3], np.uint8)), ("X", -1), ("s", 45), ("B3", 1), ("s", 38), ("B2", -1), ("s", 30)])
    how = "new" if rev else "joined"
    aim = {"found": [found("X", k, how), found("Y", k, how)], "piece": [(0, k, "X", None, 0)], "piece_starts_with": [(0, k, "Y")],
           "adjacent_pieces": [(0, k, "X", "Y")], "same_diagonal": [("X", "Y", L + 1)]}
    return _case("separator_rule_round%d_%s_n%d" % (k, "rev" if rev else "fwd", N), "pieces", b, aim, lcb_weight=L * N, max_extension_iters=k + 1)


def _same_diagonal_twin(k):
    """X m B m' Y in both genomes (m, m': 6 disagreeing bases each): X and Y lie on one diagonal in real and in virtual
    coordinates, farther apart than the span in both; B is an LCB of its own (A and C are reverse in genome 1) and both join it"""
    L = ROUND_LEN[k]
    b = Builder(2, 900 + k)
    _blocks(b, ["A", "B", "C"])
    b.shared("X", L); b.shared("Y", L)
    mid = [("X", 1), ("s", FLANK), ("B", 1), ("s", FLANK), ("Y", 1)]
    b.genome(0, [("s", 30), ("A", 1), ("s", 40)] + mid + [("s", 40), ("C", 1), ("s", 30)])
    b.genome(1, [("s", 30), ("A", -1), ("s", 40)] + mid + [("s", 40), ("C", -1), ("s", 30)])
    aim = {"found": [found("X", k, "joined"), found("Y", k, "joined")], "lcbs_root": 3, "same_diagonal": [("X", "Y", L + 2 * FLANK + BLOCK)]}
    return _case("same_diagonal_twin_round%d" % k, "pieces", b, aim, max_extension_iters=k + 1)


def _starved(twin):
    """genome 1's every stretch outside the LCBs is shorter than round 0's span (18 bases): the rounds stop there, although a
    15-base stretch P waits for round 1; the twin has one piece of exactly 19 bases and goes on to find P"""
    b = Builder(2, 950 + twin)
    _blocks(b, "ABC")
    b.shared("P", 15)
    b.genome(0, [("s", 40), ("A", 1), ("s", 30), ("P", 1), ("s", 30), ("B", 1), ("s", 50), ("C", 1), ("s", 33)])
    b.genome(1, [("s", 18), ("A", -1), ("s", 1), ("P", 1), ("s", 2), ("B", 1), ("s", 19 if twin else 18), ("C", -1), ("s", 17)])
    aim = {"starved": None if twin else (0, 1), "rounds": 2 if twin else 1, "lcbs_root": 3}
    if twin:
        aim.update(found=[found("P", 1, "joined", joins="B")], npieces=[(0, [4, 1])])
    else:
        aim.update(absent=["P"])
    return _case("starved_twin" if twin else "starved", "pieces", b, aim, lcb_weight=30, max_extension_iters=2)


# ---- rounds ------------------------------------------------------------------------------------------------------------------------
def _rounds_builder(seed, which, N=2, mixed=False, lens=ROUND_LEN, gap=30):
    """four one-anchor LCBs (A, C forward, B, D reverse in the last genome); R<k> is a stretch that round k first sees, forward
    behind A (joins A's LCB); when mixed there is also V<k>, in front of B in the forward genomes and reverse behind rc(B) in the
    last genome (joins B's LCB, which is reverse there)"""
    b = Builder(N, seed)
    _blocks(b, "ABCD")
    for k in which:
        b.shared("R%d" % k, lens[k])
    # (a stretch that joins an LCB carries the LCB's extent to itself: the stretches of the earlier rounds stand nearest to their
    #  LCB, so that the later ones still lie outside every extent when their round comes)
    fwd = sorted(k for k in which)
    rev = sorted(k for k in which if mixed)
    g0, gl = [("s", gap + 10), ("A", 1), ("s", gap + 5)], [("s", gap), ("A", 1), ("s", gap + 11)]
    for k in fwd:
        g0 += [("R%d" % k, 1), ("s", gap + k)]
        gl += [("R%d" % k, 1), ("s", gap - 4 + k)]
    for k in reversed(rev):
        b.shared("V%d" % k, lens[k])
        g0 += [("V%d" % k, 1), ("s", gap + 1 + k)]
    g0 += [("B", 1), ("s", gap + 20), ("C", 1), ("s", gap + 15), ("D", 1), ("s", gap + 10)]
    gl += [("B", -1), ("s", gap + 3)]
    for k in rev:
        gl += [("V%d" % k, -1), ("s", gap - 1 + k)]
    gl += [("C", 1), ("s", gap + 17), ("D", -1), ("s", gap + 8)]
    b.all(g0)
    b.genome(N - 1, gl)
    return b


def _rounds_cases():
    out = []
    for k in range(4):
        b = _rounds_builder(1100 + k, [k], N=3)
        out.append(_case("round%d_alone" % k, "rounds", b, {"found": [found("R%d" % k, k, "joined")], "lcbs_root": 4}))
    for iters in (0, 1, 2, 4, 6):
        b = _rounds_builder(1110, [0, 1, 2, 3], N=3)
        seen = [found("R%d" % k, k, "joined") for k in range(min(iters, 4))]
        aim = {"found": seen, "absent_new": ["R%d" % k for k in range(min(iters, 4), 4)], "rounds": min(iters, 5), "lcbs_root": 4}
        out.append(_case("rounds_all_iters%d" % iters, "rounds", b, aim, max_extension_iters=iters))
    # lighter root seeds: weight 8 -> one round at 6, weight 7 -> one round at 5, weight 6 -> none (4 < 5); blocks of 300 are found
    # by every root seed; the stretch of 9 / 8 bases is what the one round sees
    for w, L in ((8, 9), (7, 8), (6, 8)):
        b = Builder(3, 1123 + w)
        _blocks(b, "AB")
        b.shared("P", L)
        b.all([("s", 20), ("A", 1), ("s", 12), ("P", 1), ("s", 11), ("B", 1), ("s", 20)])
        b.genome(2, [("s", 20), ("A", 1), ("s", 13), ("P", 1), ("s", 12), ("B", -1), ("s", 20)])
        aim = {"rounds": 0 if w == 6 else 1, "round_weight": None if w == 6 else (0, w - 2)}
        aim.update({"absent_new": ["P"]} if w == 6 else {"found": [found("P", 0, "joined")]})
        out.append(_case("root_weight_%d" % w, "rounds", b, aim, seed_weight=w, max_extension_iters=6))
    # round 0 finds a match and drops it (light, collinear with nothing), round 1 finds a keepable one
    b = _rounds_builder(1130, [1])
    b.shared("Z", 19)
    b.layouts[0].insert(-1, ("Z", 1)); b.layouts[0].insert(-1, ("s", 30))                  # behind D in genome 0 ...
    b.layouts[1].insert(1, ("Z", 1)); b.layouts[1].insert(2, ("s", 25))                    # ... in front of A in genome 1
    out.append(_case("dropped_round_then_kept", "rounds", b, {"found": [found("Z", 0, "dropped"), found("R1", 1, "joined")],
                                                              "kept": {0: False, 1: True}, "refound": [("Z", 1, "dropped")]}))
    # round 0: M (19 * 2 = lcb_weight) becomes a NEW LCB between B and C; round 1: J joins that LCB (added_lcb re-mapped, and every
    # LCB id behind M moved by one in round 0)
    b = Builder(2, 1140)
    _blocks(b, "ABCD")
    b.shared("M", 19); b.shared("J", 15)
    b.genome(0, [("s", 40), ("A", 1), ("s", 50), ("B", 1), ("s", 30), ("M", 1), ("s", 22), ("J", 1), ("s", 30), ("C", 1), ("s", 45), ("D", 1), ("s", 40)])
    b.genome(1, [("s", 30), ("M", -1), ("s", 30), ("A", 1), ("s", 41), ("B", -1), ("s", 33), ("C", 1), ("s", 47), ("D", -1), ("s", 38)])
    b.layouts[1][0:0] = [("s", 25), ("J", -1), ("s", 21)]
    out.append(_case("new_lcb_then_joined", "rounds", b, {"found": [found("M", 0, "new"), found("J", 1, "joined", joins="M")], "lcbs": [(0, 4, 5), (1, 5, 5)],
                                                          "ids_move": 0}, lcb_weight=38))
    # round 0: X0 becomes a new LCB in front of every old one, round 1: X1 another in front of that, and J joins D's LCB: every old id
    # moves in both rounds (cur_of_orig composed over two rounds, added_lcb of X0 re-mapped).  (A new match that BRIDGES two old LCBs
    # does not exist: two old LCBs that a match between them could join are adjacent and collinear in every genome, and so were one
    # LCB already -- DESIGN.md section 9.)
    b = Builder(2, 1150)
    _blocks(b, "ABCD")
    b.shared("X0", 19); b.shared("X1", 15); b.shared("J", 15)
    b.genome(0, [("s", 25), ("X1", 1), ("s", 25), ("X0", 1), ("s", 25), ("A", 1), ("s", 50), ("B", 1), ("s", 45), ("C", 1), ("s", 40), ("D", 1), ("s", 24), ("J", 1), ("s", 40)])
    b.genome(1, [("s", 30), ("A", 1), ("s", 28), ("B", -1), ("s", 33), ("C", 1), ("s", 47), ("J", -1), ("s", 30), ("D", -1), ("s", 38), ("X0", -1), ("s", 30), ("X1", 1), ("s", 22)])
    out.append(_case("ids_move_in_two_rounds", "rounds", b, {"found": [found("X0", 0, "new"), found("X1", 1, "new"), found("J", 1, "joined", joins="D")], "lcbs_root": 4,
                                                             "lcbs": [(0, 4, 5), (1, 5, 6)], "ids_move": 1}, lcb_weight=30, max_extension_iters=2))
    # a big one: the pieces of a round hold more windows than the one-workgroup pass takes (the virtual genomes go through the hash join)
    b = _rounds_builder(1160, [0, 1], N=3, gap=1100, lens=(20, 18, 14, 12))
    out.append(_case("rounds_big", "rounds", b, {"found": [found("R0", 0, "joined", joins="A"), found("R1", 1, "joined", joins="A")],
                                                 "windows_beyond_tiny": [0, 1]}, max_extension_iters=2))
    return out


# ---- weights -----------------------------------------------------------------------------------------------------------------------
def _weights_cases():
    out = []
    for N in (2, 3):
        for short in (0, 1):                                      # a lone new match of len * N = lcb_weight, and of lcb_weight - N
            b = Builder(N, 1200 + 2 * N + short)
            _blocks(b, "AB")
            b.shared("P", 20 - short)
            b.all([("s", 30), ("A", 1), ("s", 40), ("P", 1), ("s", 40), ("B", 1), ("s", 30)])
            b.genome(N - 1, [("s", 30), ("P", -1), ("s", 35), ("A", 1), ("s", 40), ("B", -1), ("s", 30)])
            out.append(_case("lone_%s_n%d" % ("short" if short else "exact", N), "weights", b,
                             {"found": [found("P", 0, "dropped" if short else "new")], "kept": {0: not short}}, lcb_weight=20 * N, max_extension_iters=1))
    for short in (0, 1):                                          # three light collinear matches that reach the weight together
        b = Builder(2, 1220 + short)
        _blocks(b, "AB")
        for x, n in (("P", 19), ("Q", 20), ("R", 20 - short)):
            b.shared(x, n)
        trio = [("P", 1), ("s", 15), ("Q", 1), ("s", 17), ("R", 1)]
        trio_r = [("R", -1), ("s", 16), ("Q", -1), ("s", 14), ("P", -1)]
        b.genome(0, [("s", 30), ("A", 1), ("s", 40)] + trio + [("s", 40), ("B", 1), ("s", 30)])
        b.genome(1, [("s", 30)] + trio_r + [("s", 35), ("A", 1), ("s", 40), ("B", -1), ("s", 30)])
        how = "dropped" if short else "new"
        out.append(_case("trio_%s" % ("short" if short else "exact"), "weights", b,
                         {"found": [found(x, 0, how) for x in "PQR"], "kept": {0: not short}, "lcbs": [(0, 2, 2)] if short else [(0, 2, 3)]},
                         lcb_weight=118, max_extension_iters=1))
    # a light match that joins an LCB which is forward / reverse in genome 1 / reverse in the last of three genomes
    for tag, N, rev_g in (("fwd", 2, None), ("rev1", 2, 1), ("rev_last3", 3, 2)):
        b = Builder(N, 1230 + N + (rev_g or 0))
        _blocks(b, "ABC")
        b.shared("P", 19)
        b.all([("s", 30), ("A", 1), ("s", 40), ("B", 1), ("s", 25), ("P", 1), ("s", 30), ("C", 1), ("s", 30)])
        if rev_g is not None:
            b.genome(rev_g, [("s", 30), ("A", 1), ("s", 44), ("P", -1), ("s", 27), ("B", -1), ("s", 38), ("C", 1), ("s", 30)])
        else:
            b.genome(1, [("s", 30), ("A", -1), ("s", 44), ("B", 1), ("s", 27), ("P", 1), ("s", 38), ("C", -1), ("s", 30)])
        out.append(_case("joins_%s" % tag, "weights", b, {"found": [found("P", 0, "joined", joins="B")], "weight_up": ("B", 19 * N)}, max_extension_iters=1))
    # a light match P that is collinear with the LCB of A only after its lighter neighbour Z is gone: Z (19 bases, reverse in genome 1)
    # stands between A and P in genome 0 and far away in genome 1; the greedy step deletes Z first, the lightest, and P (20) joins A
    b = Builder(2, 1250)
    _blocks(b, "AB")
    b.shared("P", 20); b.shared("Z", 19)
    b.genome(0, [("s", 30), ("A", 1), ("s", 30), ("Z", 1), ("s", 30), ("P", 1), ("s", 40), ("B", 1), ("s", 30)])
    b.genome(1, [("s", 30), ("A", 1), ("s", 33), ("P", 1), ("s", 40), ("B", -1), ("s", 30), ("Z", -1), ("s", 30)])
    out.append(_case("joins_after_the_greedy_step", "weights", b, {"found": [found("Z", 0, "dropped"), found("P", 0, "joined", joins="A")], "lcbs": [(0, 2, 2)],
                                                                   "between": ("A", "Z", "P")}, max_extension_iters=1))
    # two new matches that overlap in genome 1 only (Q is reverse there, so they are not collinear: each stands on its own weight), by 1
    # column and by all but 1 of the shorter: the elimination among the new matches crops Q, and Q falls below the weight it met whole
    for tag, ov in (("by1", 1), ("allbut1", 18)):
        b = Builder(2, 1240 + ov)
        _blocks(b, "AB")
        b.shared("P", 20); b.shared("Q", 19)
        b.content["Q"][19 - ov:] = rc(b.content["P"][20 - ov:])     # genome 1 holds P and rc(Q) overlapped: P's tail is rc(Q)'s head
        b.genome(0, [("s", 30), ("A", 1), ("s", 40), ("P", 1), ("s", 33), ("Q", 1), ("s", 40), ("B", 1), ("s", 30)])
        b.genome(1, [("s", 30), ("A", -1), ("s", 40), ("P", 1), ("tail", "Q", -1, ov), ("s", 40), ("B", -1), ("s", 30)])
        out.append(_case("overlap_%s" % tag, "weights", b, {"found": [found("P", 0, "new"), found("Q", 0, "dropped", cropped=19 - ov)], "overlap": ("P", "Q", ov, 1),
                                                            "kept": {0: True}}, lcb_weight=38, max_extension_iters=1))
    return out


# ---- merge -------------------------------------------------------------------------------------------------------------------------
def _merge_builder(na, split, seed, N=2):
    """na root anchors from 30-base blocks with 6 disagreeing bases between them, in two LCBs: blocks [0, split) forward, the rest
    reverse in genome 1 (one reverse LCB); spacers in front, between the two halves and behind"""
    b = Builder(N, seed)
    names = ["b%d" % i for i in range(na)]
    _blocks(b, names, 30)
    h1, h2, h2r = [], [], []
    for i in range(split):
        h1 += ([("s", FLANK)] if i else []) + [(names[i], 1)]
    for i in range(split, na):
        h2 += ([("s", FLANK)] if i > split else []) + [(names[i], 1)]
    for i in reversed(range(split, na)):
        h2r += ([("s", FLANK)] if i < na - 1 else []) + [(names[i], -1)]
    return b, h1, h2, h2r


def _merge_case(na, where, tag):
    """where: the kept matches, as "front" (before anchor 0), "mid" (between anchors split - 1 | split), "back" (behind the last
    anchor); all are 19 or 20 bases and survive on lcb_weight = 38 or by joining"""
    split = 256 if na > 256 else 128
    b, h1, h2, h2r = _merge_builder(na, split, 1300 + na + len(where) * 7)
    seg = {"front": [("s", 30)], "mid": [("s", 30)], "back": [("s", 30)]}
    seg1 = {"front": [("s", 31)], "mid": [("s", 29)], "back": [("s", 33)]}
    names = []
    for i, w in enumerate(where):
        x = "K%d" % i
        b.shared(x, 19 + i % 2)
        names.append(x)
        seg[w] += [(x, 1), ("s", 20 + i)]
        seg1[w] += [(x, 1), ("s", 22 + i)]
    b.genome(0, seg["front"] + h1 + seg["mid"] + h2 + seg["back"])
    b.genome(1, seg1["front"] + h1 + seg1["mid"] + h2r + seg1["back"])
    ins = {"front": 0, "mid": split, "back": na}
    aim = {"na": na, "found": [found(x, 0, None) for x in names], "insert": [(x, ins[w]) for x, w in zip(names, where)], "lcbs_root": 2}
    return _case("merge_na%d_%s" % (na, tag), "merge", b, aim, lcb_weight=38, max_extension_iters=1, full=True)


def _rec_gap_case(plus, rev, recursive):
    """P joins A's LCB; the gap between A and P is exactly min_recursive_gap (+ plus) bases in the longest genome: genome 0, or
    (rev) genome 1 where both are reverse"""
    G = 40 + plus
    b = Builder(2, 1400 + 2 * plus + rev)
    _blocks(b, "AB")
    b.shared("P", 19)
    if rev:
        b.genome(0, [("s", 30), ("A", 1), ("s", 25), ("P", 1), ("s", 30), ("B", 1), ("s", 30)])
        b.genome(1, [("s", 30), ("B", 1), ("s", 35), ("P", -1), ("s", G), ("A", -1), ("s", 30)])
    else:
        b.genome(0, [("s", 30), ("A", 1), ("s", G), ("P", 1), ("s", 30), ("B", 1), ("s", 30)])
        b.genome(1, [("s", 30), ("A", 1), ("s", 25), ("P", 1), ("s", 35), ("B", -1), ("s", 30)])
    aim = {"found": [found("P", 0, "joined", joins="A")], "rec_gap": (40, plus, G)}
    return _case("rec_gap_%d_%s_rec%d" % (G, "rev" if rev else "fwd", recursive), "merge", b, aim, recursive=recursive, min_recursive_gap=40,
                 max_extension_iters=1, full=True)


# ---- width -------------------------------------------------------------------------------------------------------------------------
def _width_case(N):
    """N genomes; per round seed one forward stretch (joins A's LCB) and one that is reverse in the last genome (joins B's LCB, which
    is reverse there: the strand mask's top bit at N = 32)"""
    b = _rounds_builder(1503 + N, [0, 1, 2, 3], N=N, mixed=True, lens=(20, 18, 14, 12), gap=16)
    aim = {"found": [found("R%d" % k, k, "joined", joins="A") for k in range(4)] + [found("V%d" % k, k, "joined", joins="B") for k in range(4)],
           "lcbs_root": 4}
    return _case("width_n%d" % N, "width", b, aim)


# ---- host-only rules ---------------------------------------------------------------------------------------------------------------
def _collinear_case():
    """collinear = 1: two root LCBs, L1 = {A} (150 bases) heavier than L2 = {c0, c1} (2 x 60, reverse in genome 1): the greedy step
    leaves L1 alone.  Round 0 re-finds c0, c1 in the freed stretch together with the planted E0 .. E3 (4 x 19 bases, collinear with
    them): L2' = 196 columns outweighs L1, and the old anchor A dies in a round that is kept"""
    b = Builder(2, 1600)
    b.shared("A", 150)
    names = ["c0", "E0", "E1", "c1", "E2", "E3"]
    for x in names:
        b.shared(x, 60 if x[0] == "c" else 19)
    chain, chain_r = [], []
    for i, x in enumerate(names):
        chain += ([("s", 12)] if i else []) + [(x, 1)]
    for i, x in enumerate(reversed(names)):
        chain_r += ([("s", 13)] if i else []) + [(x, -1)]
    b.genome(0, [("s", 30), ("A", 1), ("s", 40)] + chain + [("s", 30)])
    b.genome(1, [("s", 30), ("A", 1), ("s", 40)] + chain_r + [("s", 30)])
    return b


def _host_cases():
    out = []
    b = _collinear_case()
    out.append(_case("collinear_old_anchor_dies", "host", b, {"old_died": 0, "lcbs": [(0, 1, 1)], "kept": {0: True}}, device=False, collinear=1,
                     max_extension_iters=1))
    b = _rounds_builder(1610, [0, 1])
    out.append(_case("lcb_scoring_is_not_extended", "host", b, {"absent_new": ["R0", "R1"], "rounds": 0, "lcbs_root": 4}, device=False, lcb_scoring=1,
                     lcb_weight=90))
    # an ambiguous base / a contig start right behind a planted stretch of 20 bases (round 0 finds it whole) and inside one, 15 bases
    # in: round 0 finds nothing there, round 1 (span 15) finds the 15 bases in front of the cut, the 4 or 5 behind it are lost
    for kind in ("invalid", "contig"):
        for where in ("behind", "inside"):
            b = _rounds_builder(1620, [0])
            b.shared("T", 20)
            for g in (0, 1):
                at = b.layouts[g].index(("R0", 1))
                b.layouts[g][at:at + 1] = [("T", 1)]
            gen, pos = b.build()
            s, n, _ = pos[0]["T"]
            p0 = (s - 1 + n) if where == "behind" else (s - 1 + 15)              # 0-based base in genome 0
            inv = con = None
            if kind == "invalid":
                inv = [np.zeros(len(x), bool) for x in gen]
                inv[0][p0] = True
            else:
                con = [[0, p0] if g == 0 else [0] for g in range(2)]
            c = _case("%s_%s_a_stretch" % (kind, where), "host", b, {"cut": ("T", where, kind, p0)}, device=False, contigs=con, invalid=inv, max_extension_iters=2)
            c["genomes"], c["pos"] = gen, pos                                   # (the build the position was taken from)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def _all():
    cases = []
    for k in range(4):
        for d in (-1, 0, 1):
            cases.append(_exact_piece(k, d))
    cases.append(_exact_piece(0, 0, N=3))
    cases += [_ends_case(True, True), _ends_case(False, False)]
    cases += [_lcb_border(r, m) for r in (0, 1) for m in (0, 1)]
    edges = [e + d for e in (WORD, WAVE, GATHER_BLOCK) for d in (-1, 0, 1)]                     # 31 .. 257
    cases += [_separator_at(v, 0) for v in edges] + [_separator_at(v, 1) for v in (WORD, WAVE, GATHER_BLOCK)]
    cases += [_total(T) for T in (WORD * 8, WORD * 8 + 1, WAVE * 5, WAVE * 5 + 1, GATHER_BLOCK * 2, GATHER_BLOCK * 2 + 1)]
    cases += _unequal_pieces()
    cases += [_separator_rule(k, r, N) for k in range(4) for r in (0, 1) for N in (2, 3)]
    cases += [_same_diagonal_twin(k) for k in (0, 3)]
    cases += [_starved(False), _starved(True)]
    cases += _rounds_cases()
    cases += _weights_cases()
    for na in [k * MERGE_BLOCK + d for k in (1, 2) for d in (-1, 0, 1)]:                        # 255 .. 513
        cases.append(_merge_case(na, ["front", "mid", "mid", "mid", "back"], "five_spread"))
    cases.append(_merge_case(256, ["mid"] * 5, "five_mid"))
    cases.append(_merge_case(255, ["front"], "one_front"))          # na + nx reaches 256
    cases.append(_merge_case(255, ["back", "back"], "two_back"))    # ... and crosses it
    cases.append(_merge_case(511, ["front", "back"], "two_ends"))
    cases.append(_merge_case(512, ["back"], "one_back"))
    cases += [_rec_gap_case(plus, rev, rec) for plus in (0, 1) for rev in (0, 1) for rec in (1, 0)]
    cases += [_width_case(N) for N in (2, 3, 5, 17, 32)]
    cases += _host_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:                                                 # one whole-path run per family besides the merge cases
        if c["name"] in ("separator_rule_round0_fwd_n2", "rounds_all_iters4", "trio_exact", "width_n5", "collinear_old_anchor_dies"):
            c["full"] = True
    return cases


FAMILIES = ("pieces", "rounds", "weights", "merge", "width", "host")


def family(name):
    return [c for c in _all() if c["family"] == name]


def all_cases():
    return list(_all())


def clean_intervals(case):
    """per genome the 1-based inclusive intervals a window must lie in: contigs cut at every ambiguous base (None: plain genomes)"""
    if case["contigs"] is None and case["invalid"] is None:
        return None
    out = []
    for g, x in enumerate(case["genomes"]):
        starts = list(case["contigs"][g]) if case["contigs"] else [0]
        bad = np.asarray(case["invalid"][g], bool) if case["invalid"] else np.zeros(len(x), bool)
        iv = []
        for a, e in zip(starts, starts[1:] + [len(x)]):
            cur = a
            for p in list(np.flatnonzero(bad[a:e]) + a) + [e]:
                if p > cur:
                    iv.append((cur + 1, int(p)))
                cur = p + 1
        out.append(iv)
    return out


def pattern_of(w):
    from oracle import pyoracle as O            # (the table of DESIGN.md S2 is data: csrc/seed_table.inc = oracle/seed_table.inc)
    return O.get_seed(w, 0) if w >= 3 else 0


@functools.lru_cache(maxsize=None)
def _reference(name):
    from tests import extend_ref as R, seed_ref as S
    case = next(c for c in _all() if c["name"] == name)
    p, N = case["params"], case["N"]
    clean = clean_intervals(case)
    root = S.find(case["genomes"], pattern_of(p["seed_weight"]), S.MEM, (1 << N) - 1, True, clean)
    iters = p["max_extension_iters"] if p["lcb_scoring"] == 0 else 0        # (score-weighted LCBs are not extended)
    ref = R.extend(case["genomes"], root["length"], root["start"], pattern_of, p["seed_weight"], p["lcb_weight"], iters, bool(p["collinear"]), clean)
    ref["mums"] = (root["length"], root["start"])
    return ref


def reference(case):
    """tests/extend_ref.py on the case, from the root list that tests/seed_ref.py finds (computed once per process)"""
    return _reference(case["name"])


def planted(case, name):
    """(length, signed starts) of the shared stretch `name` as a match"""
    n = case["pos"][0][name][1]
    r0 = case["pos"][0][name][2]
    return n, [(-s if (r != r0) else s) for s, _, r in (case["pos"][g][name] for g in range(case["N"]))]
