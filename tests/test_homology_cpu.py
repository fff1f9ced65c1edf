"""The homology pass without a GPU: the oracle's orc_homology_apply against the table Viterbi of tests/homology_ref.py
on alignments built to break a segment scan (tests/homology_cases.py), and the proof, taken from the reference's own path,
that those alignments do what they were built for -- a state change on every planted edge, state changes in both directions under
every scheme.  tests/test_gpu_homology.py runs the same cases on the device.  Integers throughout: every comparison is exact."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import homology_cases as HC
from tests import homology_ref as HR

CASES = {c["name"]: c for c in HC.small_cases()}


@functools.lru_cache(maxsize=None)
def ref(case, scheme):
    detail = {}
    off, cols, moved, flips = HR.homology_ref(*HC.args(CASES[case]), HC.SCHEMES[scheme], detail)
    cols.setflags(write=False); off.setflags(write=False)
    return off, cols, moved, flips, detail["keep"], detail["final"]


def orc_params(scheme):
    m, x, g, gh, gu = HC.SCHEMES[scheme]
    return O.hmm_params(match=m, mismatch=x, gap=g, go_homologous=gh, go_unrelated=gu)


@pytest.mark.parametrize("scheme", list(HC.SCHEMES))
def test_oracle_equals_the_table_viterbi(scheme):
    """every generator under one scheme: the oracle's columns, offsets and count are the reference's; and what must hold of any
    re-split, checked on the reference's output: every residue is in exactly one column afterwards (per interval and genome as many
    as before, which is what the interval table says, and the tables themselves are not written); n_moved is the number of
    single-genome columns that were added"""
    h = orc_params(scheme)
    for name, c in CASES.items():
        before = [a.copy() for a in HC.args(c)[1:]]
        off, cols, moved = ref(name, scheme)[:3]
        eoff, ecols, emoved = O.homology_apply(*HC.args(c), h)
        assert np.array_equal(off, eoff) and np.array_equal(cols, ecols) and moved == emoved, (name, scheme)
        for a, b in zip(before, HC.args(c)[1:]):
            assert np.array_equal(a, b), name                               # the caller's tables are read, not written
        old = c["cols"]
        single = lambda m: int(np.count_nonzero((m & (m - np.uint32(1))) == 0))
        assert moved == single(cols) - single(old), (name, scheme)
        assert (cols != 0).all()
        for i in range(len(c["left"])):                                      # per interval and genome: as many residues as before
            a, b = old[c["col_off"][i]:c["col_off"][i + 1]], cols[off[i]:off[i + 1]]
            for g in range(len(c["gs"])):
                n = int(np.count_nonzero(b >> np.uint32(g) & 1))
                assert n == int(np.count_nonzero(a >> np.uint32(g) & 1)) == (int(c["right"][i, g] - c["left"][i, g] + 1) if c["left"][i, g] else 0)


def test_planted_edges_flip_where_they_were_planted():
    """for N = 2 and N = 3, unaligned and aligned to the column array: for every b in 63 .. 8192 the reference path of pair (0, 1)
    leaves H exactly at interval column b in one interval and re-enters it exactly at b in another"""
    for name in ("planted1_N2", "planted2_N3", "planted3_N2_aligned"):
        c = CASES[name]
        flips = ref(name, HC.PLANT_SCHEME)[3]
        seen = set()
        for iv, b, state in c["planted"]:
            fl = flips[(iv, 0, 1)]                                           # the block: out of H, back into H, nothing else
            assert [f[1] for f in fl] == [0, 1] and fl[state] == (b, state), (name, iv, b, state, fl)
            seen.add((b, state))
            if "aligned" in name:
                assert c["col_off"][iv] % HC.SEG == 0
            else:
                assert c["col_off"][iv] % HC.STEP != 0
        assert seen == {(b, s) for b in HC.EDGES for s in (0, 1)}


def test_identity_runs_carry_the_state():
    """the stretches pair (0, 1) skips: of the lengths and at the starts that make a whole step, a whole segment and more consist of
    identity functions; the reference path changes state in front of and behind every one, and is in the same state on both sides"""
    c = CASES["identity1"]
    flips = ref("identity1", HC.PLANT_SCHEME)[3]
    assert {(s % HC.SEG == 0, s % HC.STEP == 0, n) for _, s, n, _ in c["runs"] if s} == {(a, a or b, n) for a in (0, 1) for b in (0, 1) for n in (64, 4096, 4166)}
    for iv, start, length, state in c["runs"]:
        cs = c["cols"][c["col_off"][iv]:c["col_off"][iv + 1]]
        assert (cs[start:start + length] == 4).all() and (cs[:start] & 3 == 3).all() and (cs[start + length:] & 3 == 3).all()
        fl = flips[(iv, 0, 1)]
        before = [f for f in fl if f[0] < start]; after = [f for f in fl if f[0] > start + length]
        assert len(before) + len(after) == len(fl) and after
        if start:
            assert before and before[-1][1] == state and after[0][1] == 1 - state
        else:                                                                # the path starts in U at the pair's first column, 5000 columns in,
            assert [f[1] for f in after] == [0, 1]                           # enters H in that very column, leaves it once and comes back
            assert ref("identity1", HC.PLANT_SCHEME)[4][iv][start + length] & 3 == 3


def test_tile_edges_split_on_both_sides():
    """several column offsets are multiples of 4096, the total included, and genome 1 leaves the column right in front of
    and right behind every one"""
    c = CASES["tiles1"]
    keep = ref("tiles1", HC.PLANT_SCHEME)[4]
    on_tile = [i for i in range(1, len(c["col_off"])) if c["col_off"][i] % HC.SEG == 0]
    assert len(on_tile) >= 4 and on_tile[-1] == len(c["left"])
    for i in on_tile:
        assert keep[i - 1][-1] == 0b101                                      # last column of the interval in front
        if i < len(c["left"]):
            assert keep[i][0] == 0b101


def test_every_scheme_flips_both_ways():
    """liveness, from the reference: under every scheme the mosaic and planted cases together (for the scheme at the score limits:
    with the cases built for it, since nothing shorter than 4096 columns can pay its transitions) have a change into H, a change out
    of H, residues that move, and a column in which two or more genomes stay"""
    for scheme in HC.SCHEMES:
        names = [n for n in CASES if n.startswith(("mosaic", "planted")) or (scheme == "limit" and n.startswith("limit"))]
        into = out = moved = kept = 0
        for n in names:
            _, cols, mv, flips = ref(n, scheme)[:4]
            into += sum(1 for f in flips.values() for _, s in f if s)
            out += sum(1 for f in flips.values() for _, s in f if not s)
            moved += mv
            kept += int(np.count_nonzero(cols & (cols - np.uint32(1))))
        assert into > 0 and out > 0 and moved > 0 and kept > 0, (scheme, into, out, moved, kept)


def test_ties_at_the_end_occur():
    """"H at the end" decides something: under each tie-heavy scheme some interval of the end-tie case finishes with
    v_H == v_U, and its last column's residues stay together where both genomes match there or the path was in H before"""
    c = CASES["endties1"]
    for scheme in ("ties1", "ties2"):
        final, keep = ref("endties1", scheme)[5], ref("endties1", scheme)[4]
        tied = [iv for (iv, _, _), (vh, vu) in final.items() if vh == vu]
        assert len(tied) >= 2, scheme
        assert any(keep[iv][-1] == 3 for iv in tied), scheme


def test_limit_scheme_cases():
    """at the largest scores the device takes: the path enters and leaves H once where 14000 identical columns lie between unrelated
    ones (a segment's sum reaches 2^28 there); 8192 one-sided columns cost exactly the two transitions, a tie, and the path stays;
    8193 cost one gap more, and it leaves; with half of those columns mismatches instead, the difference shows in the columns"""
    fl = ref("limit_flip", "limit")[3][(1, 0, 1)]
    assert [s for _, s in fl] == [1, 0] and 5990 <= fl[0][0] <= 6000 and fl[1][0] == 20000
    assert ref("limit_gap8192", "limit")[3][(0, 0, 1)] == [] and ref("limit_gap8192", "limit")[2] == 0
    assert [s for _, s in ref("limit_gap8193", "limit")[3][(0, 0, 1)]] == [0, 1]
    assert ref("limit_mix8192", "limit")[3][(0, 0, 1)] == [] and ref("limit_mix8192", "limit")[2] == 0
    assert ref("limit_mix8193", "limit")[3][(0, 0, 1)] == [(9000, 0), (9000 + 8193, 1)] and ref("limit_mix8193", "limit")[2] == 2 * 4097
    m, x, g, gh, gu = HC.SCHEMES["limit"]
    assert 2 * HC.SEG * g == gh + gu == -(1 << 29) and HC.SEG * m == -gh == 1 << 28


def test_wide_cases_use_every_pair_and_bit_31():
    c = CASES["wide2_N32_L8195"]
    flips = ref(c["name"], "default")[3]
    assert len(flips) == 32 * 31 // 2 and all(flips.values())                 # every pair changes state somewhere
    assert int(np.count_nonzero(c["cols"] >> np.uint32(31))) > 1000
    big = HC.big_case()
    n_seg = -(-len(big["cols"]) // HC.SEG)
    assert n_seg == 36 and 496 * n_seg > 256 * 64                            # more work items than the grid has waves
    assert int(np.count_nonzero(big["cols"] >> np.uint32(31))) > 1000
