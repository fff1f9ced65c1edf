"""The scoring schemes the DP and sum-of-pairs tests run under, one table for the CPU and the GPU tests.

The default scheme (HOXD70, -400 / -30) is symmetric and has one gap pair with |open| > |extend| > 0; each entry here takes away
one of the things that default cannot tell apart.  fill(cls, name) makes a `Scoring` structure of either binding from an entry,
so the library and the oracle are always given the same numbers."""
HOXD70 = [[91, -114, -31, -123], [-114, 100, -125, -31], [-31, -125, 100, -114], [-123, -31, -114, 91]]
DEFAULT_GAPS = (-400, -30)

# HOXD70 + 9 above the diagonal, - 6 below: S[a][b] != S[b][a] for every a != b, magnitudes of a real scheme
ASYM = [[HOXD70[a][b] + (9 if b > a else (-6 if b < a else 0)) for b in range(4)] for a in range(4)]
# nothing in common with HOXD70: positive mismatches, a negative identity score, no symmetry
SKEW = [[31, 67, -144, 68], [-24, -11, 20, -73], [114, -136, -75, -47], [4, -40, -115, -138]]
UNIT = [[1 if a == b else -1 for b in range(4)] for a in range(4)]

# name -> (matrix, gap_open, gap_extend)
SCHEMES = {
    "asym": (ASYM, -250, -45),              # transposed indices, realistic magnitudes
    "skew": (SKEW, -17, -3),                # a hard-coded matrix or gap pair, positive mismatches
    "unit": (UNIT, -2, -1),                 # dense ties with gaps that cost
    "zero_gaps": (ASYM, 0, 0),              # the tie rules alone; the scan's prefix sums E are all 0
    "open_only": (ASYM, -50, 0),            # E = 0 with a gap-open term that is not
    "ext_gt_open": (ASYM, -5, -60),         # anything that assumes |open| >= |extend|
    "edge": (ASYM, -200000, -30),           # the admission boundary of the scan kernels inside one launch
    "huge": (ASYM, -1000000, -7),           # every interval of >= 135 bases x sequences is inadmissible for the scans
    "pos_ext": (ASYM, -400, 1),             # inadmissible for every interval
}
NAMES = list(SCHEMES)
# Where the transposed matrix must give another result.  Not `unit` (symmetric), and not `zero_gaps`: every mismatch of ASYM is negative
# and gaps are free there, so no optimal alignment holds a mismatched pair and only the diagonal -- which a transposition keeps -- is ever read.
ASYMMETRIC = [n for n in NAMES if n not in ("unit", "zero_gaps")]


def transposed(matrix):
    return [[matrix[b][a] for b in range(4)] for a in range(4)]


def make(cls, matrix, gap_open, gap_extend):
    """a Scoring structure of `cls` (mauvealigner_amd._lib.Scoring or oracle.pyoracle.Scoring: the same fields)"""
    s = cls()
    s.gap_open, s.gap_extend = int(gap_open), int(gap_extend)
    for a in range(4):
        for b in range(4):
            s.matrix[a][b] = int(matrix[a][b])
    return s


def fill(cls, name, transpose=False):
    m, go, ge = SCHEMES[name]
    return make(cls, transposed(m) if transpose else m, go, ge)


def default(cls):
    return make(cls, HOXD70, *DEFAULT_GAPS)


DP_SCORE_MAX = 1 << 29


def dp_need(scheme, lens):
    """the magnitude a DP score of an interval can reach under (matrix, gap_open, gap_extend): include/mauve_hip.h's condition (2) at
    mauve_scoring, restated.  lens: the lengths of its sequence slots.  The scheme fits the interval iff this is below DP_SCORE_MAX
    (and gap_open <= 0: condition (1))"""
    m, go, ge = scheme
    assert go <= 0
    k, total, n = len(lens), sum(lens), max(lens)
    flat = [v for row in m for v in row]
    down = 2 * k * abs(go) + (total + k * n) * abs(ge) + k * max(abs(v) for v in flat)
    up = k * n * max(max(flat), 0) + (total + k * n) * max(ge, 0)
    return max(down, up)
