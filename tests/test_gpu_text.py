"""GPU tests of the alignment text (mauve_alignment_text, mauve_alignment_text_fetch) against the Python restatement of
tests/text_ref.py, the committed XMFA texts and mauve_write_xmfa of the same context.  Character work: every byte must match."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from tests.test_extract_cpu import COUNTS, load
from tests.test_gpu_coord import _disjoint_alignment
from tests.test_gpu_extract import HAND, HAND_GENOMES, _codes
from tests.text_ref import ContigJoin, TextRef

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _ref(a, gs, invalid=None):
    return TextRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], gs, invalid)


def _index(ctx, a):
    ctx.coord_index_alignment(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])


def _same_text(got, want):
    if got != want:
        n = min(len(got), len(want))
        d = next((k for k in range(n) if got[k] != want[k]), n)
        raise AssertionError("texts of %d and %d bytes differ at byte %d: %r / %r" % (len(got), len(want), d, got[max(d - 30, 0):d + 30], want[max(d - 30, 0):d + 30]))


def _check(ctx, T, **kw):
    """the device's text and block_off for one request against the restatement's; -> the text"""
    want, woff = T.text(**kw)
    nb, nk = ctx.alignment_text(**kw)
    got, boff = ctx.alignment_text_fetch(want_block_off=True)
    _same_text(got, want)
    assert nb == len(want) and np.array_equal(boff, woff), (boff, woff)
    assert nk == int(np.count_nonzero(np.diff(woff)))
    return got


def _planted(ivs, N, start=None, between=3):
    """an alignment from its rows: per interval a dict genome -> (presence over the interval's columns, reverse); every genome's intervals
    lie one after another from start[g] on -> (alignment, genome lengths)"""
    n_iv = len(ivs)
    left, right, rev = np.zeros((n_iv, N), np.int64), np.zeros((n_iv, N), np.int64), np.zeros((n_iv, N), np.int8)
    at = list(start) if start is not None else [1] * N
    parts = []
    for i, iv in enumerate(ivs):
        n = len(next(iter(iv.values()))[0])
        m = np.zeros(n, np.uint32)
        for g, (mask, r) in iv.items():
            mask = np.asarray(mask, bool)
            cnt = int(mask.sum())
            assert len(mask) == n and cnt
            m |= mask.astype(np.uint32) << np.uint32(g)
            left[i, g], right[i, g], rev[i, g] = at[g], at[g] + cnt - 1, int(r)
            at[g] += cnt + between
        parts.append(m)
    col_off = np.concatenate([[0], np.cumsum([len(m) for m in parts])]).astype(np.int64)
    return dict(left=left, right=right, reverse=rev, col_off=col_off, cols=np.concatenate(parts)), [x + 2 for x in at]


def _upload(ctx, rng, a, lens, invalid_frac=0.0):
    gs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
    inv = None
    if invalid_frac:
        inv = [rng.random(n) < invalid_frac if g % 2 == 0 else None for g, n in enumerate(lens)]
        ctx.set_genomes(gs, invalid=inv)
    else:
        ctx.set_genomes(gs)
    _index(ctx, a)
    return _ref(a, gs, inv)


def _names(N, k=0):
    """names of length 0, 1, 15, 16, 17 in turn, deflines different from them"""
    L = (0, 1, 15, 16, 17)
    names = ["abcdefghijklmnopqrstuvwxyz"[:L[(g + k) % 5]] for g in range(N)]
    defl = ["D%d_" % g + "z" * ((g * 7 + k) % 19) for g in range(N)]
    return names, defl


# ---- 1. fixtures ----
@pytest.mark.parametrize("name", sorted(COUNTS))
def test_text_golden_fixtures(ctx, name):
    """set_genomes + coord_index_alignment on the committed fixtures: the XMFA is the committed file, MAF and block_off the restatement's"""
    a, gs = load(name)
    N = len(gs)
    ctx.set_genomes(gs)
    _index(ctx, a)
    T = _ref(a, gs)
    names = ["g%d" % g for g in range(N)]
    with open(os.path.join(ROOT, "tests", "golden", name + ".xmfa"), "rb") as f:
        want = f.read()
    got = _check(ctx, T, fmt="xmfa", names=names)
    _same_text(got, want)
    _check(ctx, T, fmt="maf", names=names)
    _check(ctx, T, fmt="xmfa", names=names, wrap=7)


# ---- 2. the resident result ----
@pytest.mark.parametrize("run", ["c3_align", "c4_progressive", "c3_ambiguous", "three_50k"])
def test_text_of_the_resident_alignment(ctx, run):
    """mauve_align / mauve_progressive_align, mauve_coord_index, then the text equals mauve_write_xmfa of the same context (the host
    writer: independent of the new code) and the restatement; c3_ambiguous: ambiguous bases, which print N on both strands, and
    inversions; three_50k: several workgroups and many block records"""
    from mauvealigner_amd import _lib
    inv = None
    if run == "c4_progressive":
        gs = synth.make_config("C4", scale=0.02)
        ctx.set_genomes(gs)
        a = ctx.progressive_align(_lib.default_progressive_params(), want_xmfa=True)
    else:
        gs = synth.make_config("C3", scale=0.01)
        if run == "three_50k":
            gs = gs[:3]
            assert all(len(g) >= 45000 for g in gs)
        if run == "c3_ambiguous":
            rng = np.random.default_rng(5)
            inv = [rng.random(len(g)) < 0.003 for g in gs]
            inv[2] = None
            ctx.set_genomes(gs, invalid=inv)
        else:
            ctx.set_genomes(gs)
        a = ctx.align(_lib.default_params(), want_xmfa=True)
    N = len(gs)
    names = ["seq%d" % g for g in range(N)]
    ctx.coord_index()
    T = _ref(a, gs, inv)
    got = _check(ctx, T, fmt="xmfa", names=names)
    _same_text(got, a["xmfa"].encode())
    if run == "c3_ambiguous":
        assert np.any(a["reverse"] != 0) and b"N" in got
    if run == "three_50k":
        assert len(got) > 100_000 and a["n_cols"] > 10 * 448
    _check(ctx, T, fmt="maf", names=names)


def test_text_of_a_projection(ctx):
    """mauve_project + mauve_project_index: the text of the projection made the index in force, against the restatement on
    mauve_project_fetch's arrays"""
    from mauvealigner_amd import _lib
    gs = synth.make_config("C3", scale=0.01)
    ctx.set_genomes(gs)
    ctx.align(_lib.default_params())
    ctx.coord_index()
    pj = ctx.project([0, 2])
    assert pj["n_iv"] > 0
    ctx.project_index()
    pr = ctx.project_fetch()
    T = _ref(pr, gs)
    names = ["seq%d" % g for g in range(len(gs))]
    got = _check(ctx, T, fmt="xmfa", names=names)
    assert b"> 1:" in got and b"> 3:" in got and b"> 2:" not in got
    _check(ctx, T, fmt="maf", names=names)


# ---- 3. planted edges ----
def _mix(rng, n, p=0.7):
    m = rng.random(n) < p
    m[rng.integers(0, n)] = True
    return m


def test_text_row_lengths_and_wraps(ctx):
    """rows of 1 .. 449 columns, a genome absent from an interval; wrap 80, 1, 7 and larger than any row; names of every length"""
    rng = np.random.default_rng(2301)
    ivs = []
    for k, n in enumerate((1, 15, 16, 17, 79, 80, 81, 159, 160, 161, 447, 448, 449)):
        iv = {0: (_mix(rng, n), k % 2), 2: (np.ones(n, bool), 0)}
        if k % 4 != 3:
            iv[1] = (_mix(rng, n, 0.5), 1 - k % 2)
        ivs.append(iv)
    a, lens = _planted(ivs, 3)
    T = _upload(ctx, rng, a, lens, invalid_frac=0.02)
    for k, wrap in enumerate((80, 1, 7, 1000)):
        names, defl = _names(3, k)
        _check(ctx, T, fmt="xmfa", names=names, deflines=defl, wrap=wrap)
    _check(ctx, T, fmt="maf", names=_names(3, 1)[0])


@pytest.mark.parametrize("first", [63, 64, 65, 447, 448, 449])
def test_text_interval_starts_at_word_and_record_edges(ctx, first):
    """the second interval's first column in the whole array is `first`: its rows straddle words and block records (CO_BLOCK = 448)"""
    rng = np.random.default_rng(2310 + first)
    ivs = [{0: (_mix(rng, first), 0), 1: (_mix(rng, first), 1), 2: (np.ones(first, bool), 1)},
           {0: (_mix(rng, 500), 1), 1: (_mix(rng, 500), 0), 2: (np.ones(500, bool), 0)}]
    a, lens = _planted(ivs, 3)
    assert a["col_off"][1] == first
    T = _upload(ctx, rng, a, lens)
    names, defl = _names(3, first)
    _check(ctx, T, fmt="xmfa", names=names, deflines=defl)
    _check(ctx, T, fmt="maf", names=names)
    _check(ctx, T, fmt="xmfa", names=names, ranges=([1, 1, 0], [0, 1, first - 1], [500, 499, 1]), wrap=13)


def test_text_gap_runs_over_word_and_record_edges(ctx):
    """gap runs across columns 64 and 448 of the whole array, a row that is all gaps but for its first and last column, both strands"""
    rng = np.random.default_rng(2320)
    n = 1000
    runs = np.ones(n, bool)
    runs[50:70] = False
    runs[440:460] = False
    runs[880:910] = False
    ends = np.zeros(n, bool)
    ends[0] = ends[-1] = True
    ivs = [{0: (runs, 0), 1: (ends, 0), 2: (np.ones(n, bool), 0)}, {0: (runs, 1), 1: (ends, 1), 2: (np.ones(n, bool), 1)}]
    a, lens = _planted(ivs, 3)
    T = _upload(ctx, rng, a, lens)
    names, defl = _names(3, 2)
    _check(ctx, T, fmt="xmfa", names=names, deflines=defl)
    _check(ctx, T, fmt="maf", names=names)


@pytest.mark.parametrize("first", [31, 32, 33, 63, 64, 65])
def test_text_rows_straddle_packed_words(ctx, first):
    """rows whose bases begin at position 31 .. 65 of their genome, forward and reverse: the packed words of 32 bases and the
    ambiguity words of 64"""
    rng = np.random.default_rng(2330 + first)
    ivs = [{0: (_mix(rng, 70), 0), 1: (_mix(rng, 70), 1), 2: (np.ones(70, bool), 0)}]
    a, lens = _planted(ivs, 3, start=[first, first, 1])
    T = _upload(ctx, rng, a, lens, invalid_frac=0.1)
    names, defl = _names(3, first)
    _check(ctx, T, fmt="xmfa", names=names, deflines=defl, wrap=9)
    _check(ctx, T, fmt="maf", names=names)


def test_text_32_genomes_and_digit_changes(ctx):
    """32 genomes (g + 1 goes from 9 to 10); extents at 9/10, 99/100 and 999 999/1 000 000 in a genome of a million bases"""
    rng = np.random.default_rng(2340)
    n = 100
    iv = {g: (_mix(rng, n, 0.6), g % 3 == 1) for g in range(31)}
    iv[31] = (np.ones(n, bool), 0)
    a, lens = _planted([iv], 32)
    T = _upload(ctx, rng, a, lens)
    names, defl = _names(32)
    _check(ctx, T, fmt="xmfa", names=names, deflines=defl)
    _check(ctx, T, fmt="maf", names=names)
    # genome 0: rows 9-10, 99-100, 999999-1000000 forward; genome 1 the same extents on the reverse strand
    full2 = np.ones(2, bool)
    left = np.array([[9, 9], [99, 99], [999_999, 999_999]], np.int64)
    a = dict(left=left, right=left + 1, reverse=np.array([[0, 1]] * 3, np.int8), col_off=np.array([0, 2, 4, 6], np.int64), cols=np.full(6, 3, np.uint32))
    assert full2.all()
    T = _upload(ctx, rng, a, [1_000_100, 1_000_000])
    _check(ctx, T, fmt="xmfa", names=["m", "k"])
    got = _check(ctx, T, fmt="maf", names=["m", "k"])
    assert b"s m 999998 2 + 1000100 " in got and b"s k 0 2 - 1000000 " in got
    got = _check(ctx, T, fmt="xmfa", names=["m", "k"], ranges=([0, 0, 1, 2, 2], [0, 1, 1, 0, 1], [1, 1, 1, 1, 1]))
    assert b"> 1:9-9 " in got and b"> 1:10-10 " in got and b"> 2:99-99 " in got and b"> 1:1000000-1000000 " in got


def test_text_bodies_start_at_every_offset_mod_16(ctx):
    rng = np.random.default_rng(2350)
    ivs = [{0: (_mix(rng, 200), 0), 1: (_mix(rng, 200), 1)}, {0: (np.ones(33, bool), 1), 1: (_mix(rng, 33), 0)}]
    a, lens = _planted(ivs, 2)
    T = _upload(ctx, rng, a, lens)
    seen = set()
    for k in range(17):
        got = _check(ctx, T, fmt="xmfa", names=["n", "q"], deflines=["d" * k, "e" * (16 - k)])
        seen.add((got.index(b"\n", got.index(b"> 1:")) + 1) % 16)
        _check(ctx, T, fmt="maf", names=["n" * k, "q"])
    assert len(seen) == 16


# ---- 4. ranges ----
def test_text_ranges(ctx):
    rng = np.random.default_rng(2360)
    n = 300
    only0 = np.zeros(n, bool)
    only0[:100] = True                                                  # genome 0 has no residue behind column 100
    some = np.ones(n, bool)
    some[150:170] = False                                               # ... and columns 150..169 hold no genome at all
    ivs = [{0: (only0, 0), 1: (some, 1)}, {0: (_mix(rng, 90), 1), 1: (_mix(rng, 90), 0), 2: (_mix(rng, 90), 0)}]
    a, lens = _planted(ivs, 3)
    T = _upload(ctx, rng, a, lens)
    names, defl = _names(3, 3)
    kw = dict(names=names, deflines=defl)
    # sub-ranges, len = 0; genome 0 without a residue: its row is omitted; no genome with one: the block is omitted
    r = ([0, 0, 0, 0, 0, 1], [10, 50, 120, 150, 155, 0], [40, 0, 60, 20, 10, 90])
    for fmt in ("xmfa", "maf"):
        want, woff = T.text(fmt=fmt, ranges=r, **kw)
        assert woff[1] == woff[2] and woff[3] == woff[4] == woff[5] and woff[2] < woff[3]
        got = _check(ctx, T, fmt=fmt, ranges=r, **kw)
        assert got[woff[2]:woff[3]].count(b"> 1:" if fmt == "xmfa" else b"s " + names[0].encode() + b" ") == 0
    # a range ending at the interval's last column, overlapping and repeated ranges
    r = ([0, 0, 0, 1, 1, 1], [299, 0, 0, 89, 30, 30], [1, 300, 300, 1, 60, 60])
    _check(ctx, T, fmt="xmfa", ranges=r, wrap=11, **kw)
    _check(ctx, T, fmt="maf", ranges=r, names=names)
    # random ranges on and around the word edges
    iv = rng.integers(0, 2, 60)
    ln = a["col_off"][iv + 1] - a["col_off"][iv]
    c0 = (rng.random(60) * (ln + 1)).astype(np.int64)
    l0 = (rng.random(60) * (ln - c0 + 1)).astype(np.int64)
    _check(ctx, T, fmt="xmfa", ranges=(iv, c0, l0), wrap=5, **kw)
    # n_range = 0: the header alone
    z = (np.zeros(0, np.int64),) * 3
    for fmt in ("xmfa", "maf"):
        got = _check(ctx, T, fmt=fmt, ranges=z, names=names)
        assert got.count(b"\n") == (10 if fmt == "xmfa" else 1)
        assert ctx.alignment_text(fmt=fmt, ranges=z, names=names)[1] == 0


def test_text_random_alignments_with_ranges(ctx):
    """a random alignment of 5 genomes (gap runs over words, blocks and tiles), whole and in ranges that start and end on and around
    multiples of 64 and 448"""
    rng = np.random.default_rng(2365)
    N = 5
    a = _disjoint_alignment(rng, N, n_iv=8, length=24)
    gs = [rng.integers(0, 4, int(a["right"][:, g].max(initial=0)) + 3, dtype=np.uint8) for g in range(N)]
    inv = [rng.random(len(g)) < 0.02 if k % 2 else None for k, g in enumerate(gs)]
    ctx.set_genomes(gs, invalid=inv)
    _index(ctx, a)
    T = _ref(a, gs, inv)
    names, defl = _names(N, 4)
    _check(ctx, T, fmt="xmfa", names=names, deflines=defl)
    n_cols = len(a["cols"])
    edge = np.unique(np.concatenate([np.arange(0, n_cols, s)[:, None] + np.array([-1, 0, 1]) for s in (64, 448)], axis=None))
    edge = edge[(edge >= 0) & (edge < n_cols)]
    x0, x1 = rng.choice(edge, 120), rng.choice(edge, 120)
    x0, x1 = np.minimum(x0, x1), np.maximum(x0, x1) + 1
    iv = np.searchsorted(a["col_off"], x0, side="right") - 1
    x1 = np.minimum(x1, a["col_off"][iv + 1])
    r = (iv, x0 - a["col_off"][iv], x1 - x0)
    _check(ctx, T, fmt="xmfa", names=names, deflines=defl, ranges=r, wrap=61)
    _check(ctx, T, fmt="maf", names=names, ranges=r)


# ---- 5. fetch ----
def test_text_fetch_slices_and_buffers(ctx):
    from mauvealigner_amd import _lib
    a, gs = load("g4x3k_tree")
    ctx.set_genomes(gs)
    _index(ctx, a)
    want, woff = _ref(a, gs).text(fmt="xmfa", names=["g%d" % g for g in range(len(gs))])
    nb, _ = ctx.alignment_text(names=["g%d" % g for g in range(len(gs))])
    assert nb == len(want) > 3 * 4095
    assert ctx.alignment_text_fetch() == want                            # the whole text, pageable
    pin = _lib.pinned_empty(nb, np.uint8)
    got = ctx.alignment_text_fetch(out=pin)
    assert np.shares_memory(got, pin) and got.tobytes() == want                                        # ... and page-locked
    for step in (1, 15, 16, 17, 4095):
        for pinned in (False, True):
            buf = _lib.pinned_empty(step, np.uint8) if pinned else np.empty(step, np.uint8)
            parts = []
            for o in range(0, nb, step):
                parts.append(ctx.alignment_text_fetch(o, min(step, nb - o), out=buf).tobytes())
            _same_text(b"".join(parts), want)
    assert ctx.alignment_text_fetch(17, 0) == b"" and ctx.alignment_text_fetch(nb, 0) == b""
    boff = np.zeros(len(woff), np.int64)
    ctx._chk(ctx.L.mauve_alignment_text_fetch(ctx.h, C.c_int64(0), C.c_int64(0), None, boff.ctypes.data), "mauve_alignment_text_fetch")   # buf == NULL, len == 0
    assert np.array_equal(boff, woff)
    pb = _lib.pinned_empty(len(woff), np.int64)
    ctx._chk(ctx.L.mauve_alignment_text_fetch(ctx.h, C.c_int64(0), C.c_int64(0), None, pb.ctypes.data), "mauve_alignment_text_fetch")
    assert np.array_equal(pb, woff)
    # block_off cuts per-interval files
    i = len(woff) // 2
    assert ctx.alignment_text_fetch(int(woff[i]), int(woff[i + 1] - woff[i])) == want[woff[i]:woff[i + 1]]


# ---- 6. MAF ----
def test_text_maf_contigs(ctx):
    """the hand case (reverse-strand start), then a genome of three contigs: contig-local coordinates and srcSize, with and without contig
    names; a row across a join is refused with the range and the genome named, and passes once the ranges are split at the join"""
    gs = [_codes(s) for s in HAND_GENOMES]
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    T = _ref(HAND, gs)
    got = _check(ctx, T, fmt="maf", names=["n0", "n1", "n2"])
    assert got.decode() == ("##maf version=1 program=progressiveMauve\na\ns n0 0 20 + 22 ACGTACGTACGTACGTACGT\ns n1 100 15 + 115 CCCCCGGGGG-----TTTTT\n"
                            "s n2 3 20 - 223 TTACGTACGTAAAACCCGGT\n\n")
    contigs = [[0, 10], [0, 100], [0, 200]]
    cn = [["a", "b"], ["c", "d"], ["e", "f"]]
    with pytest.raises(ContigJoin):
        T.text(fmt="maf", names=["n0", "n1", "n2"], contigs=contigs, contig_names=cn)
    with pytest.raises(RuntimeError, match=r"\(-1\).*range 0, genome 0"):
        ctx.alignment_text(fmt="maf", names=["n0", "n1", "n2"], contigs=contigs, contig_names=cn)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):                    # no text is kept
        ctx.alignment_text_fetch()
    split = ([0, 0], [0, 10], [10, 10])
    got = _check(ctx, T, fmt="maf", names=["n0", "n1", "n2"], contigs=contigs, contig_names=cn, ranges=split)
    assert b"s n0.b 0 10 + 12 GTACGTACGT\n" in got and b"s n2.f 13 10 - 23 AAAACCCGGT\n" in got
    got = _check(ctx, T, fmt="maf", names=["n0", "n1", "n2"], contigs=contigs, ranges=split)
    assert b"s n0 0 10 + 12 GTACGTACGT\n" in got
    # three contigs in genome 0 (300 + 500 + the rest), rows in each of them on both strands, a second range across the second join
    rng = np.random.default_rng(2370)
    ivs = [{0: (_mix(rng, 250), 0), 1: (np.ones(250, bool), 0)}, {0: (_mix(rng, 400), 1), 1: (np.ones(400, bool), 1)}, {0: (_mix(rng, 350), 0), 1: (_mix(rng, 350), 1)}]
    a, lens = _planted(ivs, 2, start=[20, 1], between=60)
    T = _upload(ctx, rng, a, lens)
    c1 = int(a["left"][1, 0]) - 10
    c2 = int(a["left"][2, 0]) + 100                                      # inside the third interval's row of genome 0
    contigs = [[0, c1, c2], [0]]
    cn = [["one", "two", None], ["whole"]]
    want = None
    with pytest.raises(ContigJoin) as ei:
        want = T.text(fmt="maf", names=["G", "H"], contigs=contigs, contig_names=cn)
    assert want is None and (ei.value.range, ei.value.genome) == (2, 0)
    with pytest.raises(RuntimeError, match=r"\(-1\).*range 2, genome 0"):
        ctx.alignment_text(fmt="maf", names=["G", "H"], contigs=contigs, contig_names=cn)
    # the column of base c2 + 1 (1-based: the first of the third contig) splits the third interval
    _, col = ctx.seqpos_to_column([0], [c2 + 1])
    cut = int(col[0])
    r = ([0, 1, 2, 2], [0, 0, 0, cut], [250, 400, cut, 350 - cut])
    got = _check(ctx, T, fmt="maf", names=["G", "H"], contigs=contigs, contig_names=cn, ranges=r)
    assert b"s G.one " in got and b"s G.two " in got and b"s G. " in got and got.count(b"s H.whole ") == 4
    _check(ctx, T, fmt="maf", names=["G", "H"], contigs=contigs, ranges=r)


# ---- 7. errors and lifetime ----
def test_text_errors_and_state(ctx):
    from mauvealigner_amd import _lib
    gs = [_codes(s) for s in HAND_GENOMES]
    c2 = _lib.Context(0)
    try:
        c2.nseq = 3
        with pytest.raises(RuntimeError, match=r"\(-5\)"):                # no index
            c2.alignment_text(ranges=(np.zeros(0, np.int64),) * 3)
        with pytest.raises(RuntimeError, match=r"\(-5\)"):                # no text
            c2.alignment_text_fetch()
        c2.set_genomes(gs)
        _index(c2, HAND)
        c2.set_genomes(gs)                                                # the index was built before the last upload
        with pytest.raises(RuntimeError, match=r"\(-5\).*replaced"):
            c2.alignment_text()
        _index(c2, HAND)
        assert c2.alignment_text()[1] == 1
    finally:
        c2.close()
    ctx.set_genomes(gs)
    _index(ctx, HAND)
    T = _ref(HAND, gs)
    want, _ = T.text(fmt="xmfa", names=["a", "b", "c"])
    for kw in (dict(fmt=2), dict(fmt=-1), dict(wrap=0), dict(wrap=-3), dict(fmt="maf", wrap=80), dict(ranges=([1], [0], [1])), dict(ranges=([0], [0], [21])),
               dict(ranges=([0], [-1], [1])), dict(ranges=([0], [21], [0])), dict(contigs=[[0]] * 3), dict(fmt="maf", contigs=[[0], [0, 200], [0]]),
               dict(fmt="maf", contigs=[[1], [0], [0]]), dict(fmt="maf", contigs=[[0, 5, 5], [0], [0]])):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.alignment_text(names=["a", "b", "c"], **kw)
        with pytest.raises(RuntimeError, match=r"\(-5\)"):                # a refused call leaves no text behind
            ctx.alignment_text_fetch()
    assert ctx.alignment_text(names=["a", "b", "c"]) == (len(want), 1)
    for off, ln in ((0, len(want) + 1), (len(want), 1), (-1, 1), (len(want) + 1, 0), (5, -1)):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):                # a slice outside the text
            ctx.alignment_text_fetch(off, ln)
    assert ctx.alignment_text_fetch() == want                            # ... which is still there
    assert ctx.column_positions([0], [19])[0].tolist() == [[20, 115, -201]]
    assert ctx.alignment_text_fetch() == want                            # a query leaves it alone
    _index(ctx, HAND)                                                    # a new index ends it
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.alignment_text_fetch()
    assert ctx.alignment_text(names=["a", "b", "c"])[0] == len(want)
    ctx.set_genomes(gs)                                                  # ... and so does an upload
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        ctx.alignment_text_fetch()


def test_alignment_text_mirror():
    """mems::HipAlignmentText (include/libMems/AlignmentText.h) over IntervalLists read from committed golden XMFAs, with the genomes of
    the fixture: the bytes of the host IntervalList::WriteStandardAlignment, and MAF through ContigRanges (tests/cpp/text_mirror_test.cpp)"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "text_mirror_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "text_mirror_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        for name in ("g3x5k_inv", "g4x3k_tree"):
            a, gs = load(name)
            mfa = os.path.join(td, name + ".mfa")
            with open(mfa, "w") as f:
                for g, s in enumerate(gs):
                    f.write(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()))
            r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", name + ".xmfa"), mfa, "700"], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
