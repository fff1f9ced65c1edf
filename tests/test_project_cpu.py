"""CPU-side checks of the projection onto a genome subset: the numpy restatement of tests/project_ref.py, which is the
expected value of the GPU tests, against things it did not produce -- a hand case with every array written out, the position rule of S14
(tests/coord_ref.py) on its output and on its source, pinned counts on the committed fixtures, the mirror's host projectIntervalList (tests/cpp/project_test.cpp), what the reference's own
program src/projectAndStrip.cpp wrote when built on the mirror (tests/golden/reference_project.json; built and run again where the
reference tree is present) -- and the new entry points in the export list of the built library."""
import ctypes as C
import hashlib
import itertools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, synth
from tests import project_ref as PR
from tests.coord_ref import CoordRef
from tests.extract_ref import ExtractRef, parse_xmfa
from tests.test_compat_headers import REFERENCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_PROJECT = os.path.join(GOLDEN, "reference_project.json")
NEW = ("mauve_default_project_params", "mauve_project", "mauve_project_fetch", "mauve_project_index")
FIXTURES = ("g3x5k_inv", "g4x3k_tree", "g5x3k_unique", "g4x6k_repeat")
# fixture: {projection list: (output intervals, source pieces, filler columns, columns with drop_empty)}, all pairs and the full set
COUNTS = {
    "g3x5k_inv": {(0, 1): (1, 3, 2, 5019), (0, 2): (3, 3, 0, 5008), (1, 2): (3, 3, 0, 5026), (0, 1, 2): (3, 3, 0, 5030)},
    "g4x3k_tree": {(0, 1): (5, 17, 54, 3507), (0, 2): (9, 12, 183, 3816), (0, 3): (8, 12, 122, 3702), (1, 2): (9, 12, 143, 3790), (1, 3): (8, 12, 73, 3667),
                   (2, 3): (5, 15, 93, 3696), (0, 1, 2, 3): (12, 12, 0, 4068)},
    "g5x3k_unique": {(0, 1): (1, 1, 0, 3025), (0, 2): (1, 1, 0, 3025), (0, 3): (1, 1, 0, 3025), (0, 4): (1, 1, 0, 3023), (1, 2): (1, 1, 0, 3007), (1, 3): (1, 1, 0, 3007),
                     (1, 4): (1, 1, 0, 3005), (2, 3): (1, 1, 0, 3006), (2, 4): (1, 1, 0, 3004), (3, 4): (1, 1, 0, 3004), (0, 1, 2, 3, 4): (1, 1, 0, 3032)},
    "g4x6k_repeat": {(0, 1): (1, 1, 0, 6031), (0, 2): (1, 1, 0, 6046), (0, 3): (1, 1, 0, 6056), (1, 2): (1, 1, 0, 6035), (1, 3): (1, 1, 0, 6045), (2, 3): (1, 1, 0, 6060),
                     (0, 1, 2, 3): (1, 1, 0, 6091)},
}


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return dict(left=z["left"], right=z["right"], reverse=z["reverse"], col_off=z["col_off"], cols=z["cols"])


def check_projection(a, proj, r, drop_empty):
    """what holds for any projection r of the alignment a, by the position rule of S14 on both"""
    N = a["left"].shape[1]
    proj = list(proj)
    pmask = sum(1 << g for g in proj)
    others = [g for g in range(N) if g not in proj]
    n_out, n_cols = len(r["left"]), len(r["cols"])
    assert r["col_off"][0] == 0 and r["col_off"][-1] == n_cols and np.all(np.diff(r["col_off"]) > 0)
    assert not np.any(r["cols"] & ~np.uint32(pmask)) and np.all(r["left"][:, proj] > 0)
    assert not np.any(r["left"][:, others]) and not np.any(r["right"][:, others]) and not np.any(r["reverse"][:, others])
    assert not np.any(r["reverse"][:, proj[0]])                                     # normalised: the first projected genome runs forward
    if drop_empty:
        assert np.all(r["cols"] != 0)
    bits = r["cols"][:, None] >> np.arange(N, dtype=np.uint32) & 1
    iv = np.repeat(np.arange(n_out), np.diff(r["col_off"]))
    for o in range(n_out):                                                          # residues per row = right - left + 1
        got = bits[r["col_off"][o]:r["col_off"][o + 1]].sum(axis=0)
        assert np.array_equal(got[proj], (r["right"][o] - r["left"][o] + 1)[proj])
    # every base of a projected genome inside an output interval lies in exactly one column
    E = CoordRef(r["left"], r["right"], r["reverse"], r["col_off"], r["cols"])
    pos, defined = E.column_positions(iv, np.arange(n_cols) - r["col_off"][iv])
    assert np.array_equal(defined, r["cols"])
    for g in proj:
        p = np.abs(pos[:, g][bits[:, g] != 0])
        want = np.concatenate([np.arange(r["left"][o, g], r["right"][o, g] + 1) for o in range(n_out)] + [np.zeros(0, np.int64)])
        assert np.array_equal(np.sort(p), np.sort(want)) and len(np.unique(p)) == len(p)
    # a column that came from the source keeps its positions, negated when its piece was flipped
    S = CoordRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"])
    from_src = r["src_col"] >= 0
    x = r["src_col"][from_src]
    siv = np.searchsorted(a["col_off"], x, side="right") - 1
    spos, sdef = S.column_positions(siv, x - a["col_off"][siv])
    flip_of_iv = np.zeros(len(a["left"]), bool)
    flip_of_iv[r["src_iv"]] = r["src_flip"] != 0
    assert np.all(np.isin(siv, r["src_iv"]))
    sign = np.where(flip_of_iv[siv], -1, 1)[:, None]
    keep = np.zeros(N, bool)
    keep[proj] = True
    assert np.array_equal(pos[from_src], np.where(keep[None, :], spos * sign, 0))
    assert np.array_equal(r["cols"][from_src], sdef & np.uint32(pmask))
    assert int(np.count_nonzero(~from_src)) == r["n_fill"] and np.all(np.isin(r["cols"][~from_src], [1 << g for g in proj]))
    # every kept source column appears once
    src_cols = np.concatenate([np.arange(a["col_off"][i], a["col_off"][i + 1]) for i in r["src_iv"]] + [np.zeros(0, np.int64)])
    if drop_empty:
        src_cols = src_cols[(a["cols"][src_cols] & np.uint32(pmask)) != 0]
    assert np.array_equal(np.sort(x), np.sort(src_cols))
    assert np.array_equal(np.sort(r["src_iv"]), np.flatnonzero(np.all(a["left"][:, proj] != 0, axis=1)))


def test_hand_case_every_array_written_out():
    a = PR.HAND
    r = PR.project(a, [0, 1])
    # interval 3 lacks genome 1; interval 0 is reversed in genome 0 and comes flipped, its column of genome 2 alone leaves; intervals 1 and 2
    # are collinear without genome 2, with the bases 9..11 of genome 0 and none of genome 1 between them
    assert r["left"].tolist() == [[1, 1, 0], [6, 6, 0]] and r["right"].tolist() == [[4, 4, 0], [14, 11, 0]]
    assert r["reverse"].tolist() == [[0, 1, 0], [0, 0, 0]]
    assert r["col_off"].tolist() == [0, 5, 15]
    assert r["cols"].tolist() == [3, 3, 2, 1, 3,  3, 2, 1, 3,  1, 1, 1,  3, 3, 3]
    assert r["src_off"].tolist() == [0, 1, 3] and r["src_iv"].tolist() == [0, 1, 2] and r["src_flip"].tolist() == [1, 0, 0]
    assert r["src_col"].tolist() == [5, 4, 2, 1, 0,  6, 7, 8, 9,  -1, -1, -1,  10, 11, 12]
    assert r["n_fill"] == 3
    check_projection(a, [0, 1], r, True)
    # without drop_empty the column stays as a zero mask
    r = PR.project(a, [0, 1], drop_empty=False)
    assert r["cols"].tolist() == [3, 3, 0, 2, 1, 3,  3, 2, 1, 3,  1, 1, 1,  3, 3, 3] and r["col_off"].tolist() == [0, 6, 16]
    assert r["src_col"].tolist()[:6] == [5, 4, 3, 2, 1, 0]
    # compact: rows and bits in proj order
    r = PR.project(a, [1, 0], compact=True)
    assert r["left"].tolist() == [[1, 1], [6, 6]] and r["right"].tolist() == [[4, 4], [11, 14]] and r["reverse"].tolist() == [[0, 1], [0, 0]]
    assert r["cols"].tolist() == [3, 2, 1, 3, 3,  3, 1, 2, 3,  2, 2, 2,  3, 3, 3] and r["src_flip"].tolist() == [0, 0, 0]
    # with genome 2 the strands of intervals 1 and 2 differ: nothing joins; proj[0] = 2 orders by genome 2 and flips interval 2
    r = PR.project(a, [2, 0], drop_empty=False)
    assert r["src_iv"].tolist() == [1, 0, 2, 3] and r["src_flip"].tolist() == [0, 0, 1, 0] and r["col_off"].tolist() == [0, 4, 10, 13, 17]
    assert r["reverse"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]] and r["cols"].tolist() == [5, 0, 5, 5,  5, 5, 4, 4, 1, 5,  5, 5, 5,  5, 5, 0, 5]
    check_projection(a, [2, 0], r, False)
    # one genome: everything kept is one run, the unaligned bases between the intervals are filler
    r = PR.project(a, [0])
    assert r["left"].tolist() == [[1, 0, 0]] and r["right"].tolist() == [[22, 0, 0]] and r["cols"].tolist() == [1] * 22 and r["src_flip"].tolist() == [1, 0, 0, 0]
    assert r["n_fill"] == 1 + 3 + 5
    # nothing kept
    b = dict(a, left=a["left"].copy(), right=a["right"].copy())
    b["left"][:3, 1] = b["right"][:3, 1] = 0
    b["cols"] = a["cols"] & np.uint32(5)
    r = PR.project(b, [1, 2])
    assert r["left"].shape == (0, 3) and r["col_off"].tolist() == [0] and r["src_off"].tolist() == [0] and len(r["cols"]) == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_invariants_and_pinned_counts(name):
    a = load(name)
    N = a["left"].shape[1]
    sets = list(itertools.combinations(range(N), 2)) + [tuple(range(N))]
    assert sorted(COUNTS[name]) == sorted(sets)
    for P in sets:
        for drop in (True, False):
            r = PR.project(a, P, drop_empty=drop)
            check_projection(a, P, r, drop)
            if drop:
                assert (len(r["left"]), len(r["src_iv"]), r["n_fill"], len(r["cols"])) == COUNTS[name][P], P
        c = PR.project(a, P, compact=True)
        w = PR.project(a, P)
        assert np.array_equal(c["left"], w["left"][:, list(P)]) and np.array_equal(c["cols"] != 0, w["cols"] != 0)
    # a permuted list: the same intervals when the first genome stays, rows of the compact form permuted
    if N > 2:
        p1, p2 = PR.project(a, [0, 1, 2]), PR.project(a, [0, 2, 1])
        assert np.array_equal(p1["left"], p2["left"]) and np.array_equal(p1["src_iv"], p2["src_iv"])
        check_projection(a, [2, 0], PR.project(a, [2, 0]), True)
    # the full set with no reversed genome-0 row and nothing collinear: the intervals that hold every genome, in genome 0's order, unchanged
    full = PR.project(a, range(N), drop_empty=False)
    assert not np.any(a["reverse"][:, 0])
    if len(full["left"]) == len(full["src_iv"]):
        iv = np.flatnonzero(np.all(a["left"] != 0, axis=1))
        iv = iv[np.argsort(a["left"][iv, 0])]
        assert np.array_equal(full["src_iv"], iv) and not np.any(full["src_flip"]) and full["n_fill"] == 0
        assert np.array_equal(full["left"], a["left"][iv]) and np.array_equal(full["right"], a["right"][iv]) and np.array_equal(full["reverse"], a["reverse"][iv])
        assert np.array_equal(np.diff(full["col_off"]), np.diff(a["col_off"])[iv])
        assert np.array_equal(full["cols"], np.concatenate([a["cols"][a["col_off"][i]:a["col_off"][i + 1]] for i in iv]))
    else:
        pytest.fail("the full projection of %s coalesces intervals: the fixture no longer shows the identity case" % name)


def test_new_entry_points_are_exported_and_the_defaults_work_on_the_host():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert C.sizeof(_lib.ProjectParams) == 4 + 4 * 32 + 4 and C.sizeof(_lib.ProjectSizes) == 32
    for n in (1, 3, 32):
        p = _lib.default_project_params(n)
        assert p.n_proj == n and list(p.proj)[:n] == list(range(n)) and not any(list(p.proj)[n:]) and p.drop_empty == 1


def _build_project_test(td):
    exe = os.path.join(td, "project_test")
    lib = os.path.join(ROOT, "mauvealigner_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "project_test.cpp"), "-o", exe,
                           "-L" + lib, "-lmauve_hip", "-Wl,-rpath," + lib])
    return exe


def parse_groups(stdout):
    """the lines of tests/cpp/project_test.cpp -> per LCB (source intervals, inverted flags, signed left ends, signed right ends)"""
    out = []
    for line in stdout.splitlines():
        if not line.startswith("lcb "):
            continue
        pieces, ends = line.split(":", 1)[1].split("|")
        pieces = pieces.split()
        ends = [e.split(":") for e in ends.split()]
        out.append(([int(p[:-1]) for p in pieces], [int(p[-1] == "-") for p in pieces], [int(e[0]) for e in ends], [int(e[1]) for e in ends]))
    return out


def test_mirror_project_interval_list_equals_the_restatement_groups():
    """tests/cpp/project_test.cpp on the golden XMFAs, host C++ only: the mirror's projectIntervalList keeps, inverts, orders and groups
    the intervals as the restatement does, and its LCB ends are the restatement's interval ends"""
    with tempfile.TemporaryDirectory() as td:
        exe = _build_project_test(td)
        for name in FIXTURES:
            a = load(name)
            N = a["left"].shape[1]
            for P in list(itertools.combinations(range(N), 2)) + [tuple(range(N)), (N - 1, 0), (N - 1,)]:
                r = subprocess.run([exe, os.path.join(GOLDEN, name + ".xmfa")] + [str(g) for g in P], capture_output=True, text=True)
                assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
                got = parse_groups(r.stdout)
                w = PR.project(a, P, compact=True)
                assert len(got) == len(w["left"]), (name, P)
                sign = np.where(w["reverse"] != 0, -1, 1)
                for o, (pieces, flips, le, re) in enumerate(got):
                    s = slice(w["src_off"][o], w["src_off"][o + 1])
                    assert pieces == w["src_iv"][s].tolist() and flips == w["src_flip"][s].tolist(), (name, P, o)
                    assert le == (w["left"][o] * sign[o]).tolist() and re == (w["right"][o] * sign[o]).tolist(), (name, P, o)


# ---- the reference's own programs on the mirror ----
PAS_FIXTURE, PAS_IDS = "g4x3k_tree", (0, 2)


def pas_inputs(name=PAS_FIXTURE, ids=PAS_IDS):
    """-> (the committed XMFA of the fixture, its genomes as FastA texts, the digest of them and the sequence ids)"""
    with open(os.path.join(GOLDEN, name + ".xmfa")) as f:
        xmfa = f.read()
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    fas = [">g%d\n%s\n" % (g, synth.to_ascii(z["genome%d" % g]).decode()) for g in range(z["left"].shape[1])]
    return xmfa, fas, hashlib.sha256((xmfa + "\0" + "\0".join(fas) + "\0" + " ".join(str(g) for g in ids)).encode()).hexdigest()


def build_project_and_strip(src_dir, td):
    exe = os.path.join(td, "projectAndStrip")
    lib = os.path.join(ROOT, "mauvealigner_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(src_dir, "projectAndStrip.cpp"), "-o", exe,
                           "-L" + lib, "-lmauve_hip", "-Wl,-rpath," + lib])
    return exe


def run_project_and_strip(exe, td, name=PAS_FIXTURE, ids=PAS_IDS):
    """`projectAndStrip in.xmfa out.xmfa ids...` in a directory that holds the XMFA and the sequence files it names (g0, g1, ...) -> out.xmfa"""
    xmfa, fas, _ = pas_inputs(name, ids)
    d = os.path.join(td, name)
    os.makedirs(d)
    with open(os.path.join(d, "in.xmfa"), "w") as f:
        f.write(xmfa)
    for g, t in enumerate(fas):
        with open(os.path.join(d, "g%d" % g), "w") as f:
            f.write(t)
    subprocess.run([exe, "in.xmfa", "out.xmfa"] + [str(g) for g in ids], capture_output=True, text=True, check=True, cwd=d)
    with open(os.path.join(d, "out.xmfa")) as f:
        return f.read()


def check_project_and_strip(out_xmfa, name=PAS_FIXTURE, ids=PAS_IDS):
    """the blocks of two or more sequences the program wrote against the restatement at drop_empty = 0: their count, ends and strands, and
    their rows, letter for letter -- with the filler columns (the mirror's Interval::SetMatches lays the bases between the pieces out as
    rule 4 does) and once they are taken out; the blocks of one sequence are the bases no projected interval covers"""
    a = load(name)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    gs = [z["genome%d" % g] for g in range(a["left"].shape[1])]
    w = PR.project(a, ids, drop_empty=False, compact=True)
    parsed = parse_xmfa(out_xmfa, len(ids))
    blocks = [b for b in parsed if len(b) >= 2]
    assert len(blocks) == len(w["left"]) > 1
    order = sorted(range(len(blocks)), key=lambda i: blocks[i][0][0])
    wide = PR.project(a, ids, drop_empty=False)
    letters = ExtractRef(wide["left"], wide["right"], wide["reverse"], wide["col_off"], wide["cols"], gs).extract(keep=list(ids))[0]
    for o, i in enumerate(order):
        blk = blocks[i]
        s = slice(w["col_off"][o], w["col_off"][o + 1])
        real = w["src_col"][s] >= 0
        for k in range(len(ids)):
            le, re, rev, row = blk[k]
            assert (le, re, rev) == (w["left"][o, k], w["right"][o, k], bool(w["reverse"][o, k])), (o, k)
            assert np.array_equal(row, letters[k][s]), (o, k)
            assert np.array_equal(row[real], letters[k][s][real]) and np.array_equal(row[real] != ord("-"), (w["cols"][s][real] >> k & 1) != 0), (o, k)
    assert np.any(np.diff(w["src_off"]) > 1) and w["n_fill"] > 0
    # the blocks of one sequence and the blocks of two tile every projected genome: each base is written once
    for k, g in enumerate(ids):
        spans = sorted((b[k][0], b[k][1]) for b in parsed if k in b)
        assert spans[0][0] == 1 and spans[-1][1] == len(gs[g]) and all(x[1] + 1 == y[0] for x, y in zip(spans, spans[1:])), k


def test_stored_project_and_strip_output_equals_the_restatement():
    """what src/projectAndStrip.cpp, built from its own source on the mirror, wrote for g4x3k_tree and the sequences 0 2
    (tests/golden/reference_project.json, tests/golden/make_reference_project_golden.py)"""
    with open(GOLDEN_PROJECT) as f:
        ref = json.load(f)
    digest = pas_inputs()[2]
    assert digest in ref, "the input differs from the one the stored output was made on"
    assert ref[digest]["fixture"] == PAS_FIXTURE and ref[digest]["ids"] == list(PAS_IDS)
    check_project_and_strip(ref[digest]["xmfa"])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present")
def test_reference_projection_programs_compile_unmodified_and_project_and_strip_runs():
    """src/projectAndStrip.cpp and src/alignmentProjector.cpp, where they lie, against -I include: they need projectIntervalList,
    IdentifyBreakpoints / ComputeLCBs_v2 over GappedAlignment*, Interval::SetMatches over those vectors and boost::tuple's name.
    projectAndStrip, built and run, writes what the stored output holds"""
    for tool in ("projectAndStrip.cpp", "alignmentProjector.cpp"):
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(REFERENCE, tool)])
    with open(GOLDEN_PROJECT) as f:
        ref = json.load(f)
    with tempfile.TemporaryDirectory() as td:
        out = run_project_and_strip(build_project_and_strip(REFERENCE, td), td)
    assert out == ref[pas_inputs()[2]]["xmfa"]
    check_project_and_strip(out)
