"""The repeat map on the device (mauve_repeat_matches / mauve_repeat_fetch) against the plain-Python reference
(tests/repeat_map_ref.py), bit for bit: the planted genomes of tests/repeat_map_cases.py -- walk rounds, chaining, the order rule,
even weights, nesting, multiplicity limits, tandem arrays, edges, emit-once, canonical order -- a randomised sweep, a three-genome
context, the error codes, forced wide window indices in a child process and the RepeatHash mirror."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import _lib, synth
from oracle import pyoracle as O
from tests import repeat_map_cases as RC
from tests import repeat_map_ref as RM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = {"w15": O.get_seed(15, 0), "solid8": O.get_seed(8, O.SOLID_SEED), "w12": O.get_seed(12, 0), "w11": O.get_seed(11, 0)}


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def device_records(ctx, codes, pattern, min_multi=2, max_multi=32, contig_starts=None, invalid=None):
    ctx.set_genomes([codes], contig_starts=None if contig_starts is None else [contig_starts], invalid=None if invalid is None else [invalid])
    return RM.from_csr(*ctx.repeat_matches(0, pattern, min_multi, max_multi))


def check_case(ctx, c, pattern):
    want = c.reference(pattern)
    c.aim(want)
    got = device_records(ctx, c.codes, pattern, c.min_multi, c.max_multi, c.contig_starts, c.invalid)
    assert got == want, (c.name, [r for r in got if r not in want][:5], [r for r in want if r not in got][:5])


@pytest.mark.parametrize("name", ["w15", "w12"])
def test_walk_rounds(ctx, name):
    """k_lo and k_hi of 0, 1, 62 .. 129 independently: the first, second and third 64-offset round of either walk, and their borders"""
    for lo in RC.EDGES:
        for hi in RC.EDGES:
            check_case(ctx, RC.walk(PATTERNS[name], lo, hi), PATTERNS[name])


@pytest.mark.parametrize("name", list(PATTERNS))
def test_planted_cases(ctx, name):
    cases = RC.all_cases(PATTERNS[name], walks=False)
    assert len(cases) >= 36
    for c in cases:
        check_case(ctx, c, PATTERNS[name])


@pytest.mark.parametrize("name", ["solid8", "w12"])
def test_even_weight_self_complementary_mer(ctx, name):
    """the family of a mer that is its own reverse complement: a forward hit with its own cluster; the reverse diagonal passes it"""
    for kind in ("inverted", "direct"):
        c = RC.selfcomp(PATTERNS[name], kind)
        assert c is not None
        check_case(ctx, c, PATTERNS[name])


def test_order_rule_odd_and_even(ctx):
    for name in ("w15", "solid8"):
        span = O.seed_length(PATTERNS[name])
        for spacer in (0, 1, 2, span - 1, span, 2 * span):
            for L in (2 * span + 3, 2 * span + 4):
                check_case(ctx, RC.inverted(PATTERNS[name], spacer, L), PATTERNS[name])


def test_multiplicity_limits_and_errors(ctx):
    pat = PATTERNS["w15"]
    c = RC.nesting(pat, "both", "FRF")
    full = c.reference(pat)
    assert {len(r[1]) for r in full} == {2, 3}
    for lo, hi in ((3, 32), (2, 2), (2, 3), (0, 32), (-5, 2), (4, 32), (3, 2)):
        want = RM.repeat_matches(c.codes, pat, lo, hi)
        assert device_records(ctx, c.codes, pat, lo, hi) == want, (lo, hi)
        assert want == [r for r in full if max(2, lo) <= len(r[1]) <= hi]
    for bad in (33, 1, 0, 1000):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.repeat_matches(0, pat, 2, bad)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.repeat_matches(1, pat)                                               # one genome set
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.repeat_matches(0, 0b1011)                                            # not a palindrome
    L = _lib.load()
    fresh = _lib.Context(0)
    try:
        n = np.zeros(4, np.int64)
        p = n.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64))
        assert L.mauve_repeat_fetch(fresh.h, p, p, p, p) == -5                   # no result in force
        assert L.mauve_repeat_matches(fresh.h, 0, _lib.C.c_uint64(pat), _lib.C.c_int64(2), _lib.C.c_int64(32), p, p) == -5      # no genomes
        assert L.mauve_repeat_matches(fresh.h, 0, _lib.C.c_uint64(pat), _lib.C.c_int64(2), _lib.C.c_int64(32), None, p) == -1
        fresh.set_genomes([c.codes])
        assert fresh.repeat_matches(0, pat)[0].size == len(full)
        fresh.set_genomes([c.codes])                                             # an upload ends the result
        assert L.mauve_repeat_fetch(fresh.h, p, p, p, p) == -5
    finally:
        fresh.close()


def test_three_genome_context(ctx):
    """the repeats of genome 1 when genomes 0 and 2 hold copies of the same element: the other genomes do not matter"""
    pat = PATTERNS["w15"]
    c = RC.nesting(pat, "both", "FRF")
    rng = np.random.default_rng(77)
    elem = c.codes[40:40 + 150]
    g0 = np.concatenate([rng.integers(0, 4, 333), elem, rng.integers(0, 4, 90), RC.rc(elem), rng.integers(0, 4, 20)]).astype(np.uint8)
    g2 = np.concatenate([elem, elem, rng.integers(0, 4, 57)]).astype(np.uint8)
    want = c.reference(pat)
    ctx.set_genomes([g0, c.codes, g2])
    assert RM.from_csr(*ctx.repeat_matches(1, pat)) == want
    assert RM.from_csr(*ctx.repeat_matches(0, pat)) == RM.repeat_matches(g0, pat)
    assert RM.from_csr(*ctx.repeat_matches(2, pat)) == RM.repeat_matches(g2, pat)
    # a seed pass's match list fetched after the repeat map is still the seed pass's
    ln, st = ctx.seed_mums(pat)
    eln, est = O.find_matches([g0, c.codes, g2], pat)
    assert np.array_equal(ln, eln) and np.array_equal(st, est)
    assert RM.from_csr(*ctx.repeat_matches(1, pat)) == want


def sweep_genome(rng):
    """300 to 3000 random bases with planted elements: random length, 2 to 6 copies, either strand, 0 to 8 % divergence"""
    n = int(rng.integers(300, 3001))
    g = rng.integers(0, 4, n).astype(np.uint8)
    for _ in range(int(rng.integers(1, 4))):
        e = rng.integers(0, 4, int(rng.integers(10, min(400, n // 3)))).astype(np.uint8)
        for _ in range(int(rng.integers(2, 7))):
            cp = e.copy()
            hit = rng.random(len(cp)) < rng.uniform(0, 0.08)
            cp[hit] = (cp[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
            if rng.random() < 0.5:
                cp = RC.rc(cp)
            at = int(rng.integers(0, n - len(cp) + 1))
            g[at:at + len(cp)] = cp
    return g


SWEEP_GENOMES = 150


def test_randomised_sweep(ctx):
    rng = np.random.default_rng(20261)
    seen = set()
    for i in range(SWEEP_GENOMES):
        g = sweep_genome(rng)
        w = 5 + i % 11                                                           # weights 5 .. 15: spans from 7 up
        pat = O.get_seed(w, int(rng.integers(0, 3))) if i % 4 else O.get_seed(w, O.SOLID_SEED)
        lo, hi = ((2, 32), (2, 32), (3, 32), (2, 4))[i % 4]
        want = RM.repeat_matches(g, pat, lo, hi)
        got = device_records(ctx, g, pat, lo, hi)
        assert got == want, (i, w, len(g), [r for r in got if r not in want][:3], [r for r in want if r not in got][:3])
        seen.update(len(r[1]) for r in want)
    assert {2, 3, 4, 5, 6} <= seen and max(seen) > 6


_WIDE_SUBSET = ["tests/test_gpu_repeat_map.py::test_planted_cases", "tests/test_gpu_repeat_map.py::test_three_genome_context",
                "tests/test_gpu_repeat_map.py::test_walk_rounds"]


def test_forced_wide_index():
    """MAUVE_WIDE_INDEX=1 in a fresh process: the 64-bit sort values of the repeat pass against the same reference"""
    env = dict(os.environ)
    env["MAUVE_WIDE_INDEX"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", "-k", "w15 or three_genome"] + _WIDE_SUBSET,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert " passed" in r.stdout and " skipped" not in r.stdout and " failed" not in r.stdout, r.stdout[-2000:]


def test_repeat_hash_mirror():
    """tests/cpp/repeat_map_test.cpp: a default RepeatHash gives the enumerator's rows, SetExtension(true) those of the repeat map"""
    g = RC.long_pair(PATTERNS["w11"], 0.05).codes
    g = np.concatenate([g, RC.nesting(PATTERNS["w11"], "both", "FRF").codes]).astype(np.uint8)
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "g.fa")
        with open(fa, "w") as f:
            f.write(">g\n%s\n" % synth.to_ascii(g).decode())
        exe = os.path.join(td, "repeat_map_test")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "repeat_map_test.cpp"),
                               "-o", exe, "-L" + os.path.join(ROOT, "mauvealigner_amd"), "-lmauve_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "mauvealigner_amd")])
        r = subprocess.run([exe, fa], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
