"""The kernels behind the sort of a seed pass (csrc/seed_pass.hip) where this file's change touches them: the run detection with 4, 8
and 16 windows per thread (mum_runs, mum_runs_group; MAUVE_RUNS_ITEMS forces one instantiation, unset the rule of runs_items chooses),
the genome table they and hits_scatter<true> index by a lane's genome (three, five and nine genomes), chunk_bound with its first probe
and the three behind it issued together, and join_hash behind it.  Every case compares Context.seed_mums (the host hits: Context.extend_hits) with
oracle.pyoracle.find_matches, lengths and starts exactly.

Tile edges: three random genomes of 13 000 bases (12 986 windows in genome 0: three tiles of 4096 and a part, 38 958 windows in all, so
the pass is not tiny) with common stretches planted so that, in genome 0,
  * matches start at the windows 0, 1024, 2047, 3073, 4096, 5121, 6144 and at the stretch that ends in the last window,
  * the windows 4095 and 4096 are hits of two different diagonals (the first stretch ends where the second begins: phase 3 of the run
    detection, across the edge of every tile size),
  * one stretch has a substitution just behind window 8192, so that a hit at or behind the edge has its nearest hit, more than one and
    at most a span back, in the tile in front (the halo),
  * one match straddles window 12288.
The classes are asserted from the oracle's lists before the device runs.  Tiny launch: three genomes of 2 500 bases.  Pair groups: the
pairwise finder over three and over nine genomes of 4 000 bases, a planted stretch per pair, the one of pair (0, 1) at the first window
of genome 0.  Host hits: extend_hits under MAUVE_WIDE_INDEX=1 (hits_scatter<true>) with five and nine genomes.  Chunk bounds: two
genomes, 40 000 list entries, 256 buckets, a run of 1 000 C (one mer, bucket 0x55) placed so that a chunk edge falls into that bucket
more than 256 entries in front of its end; the reference's list must show an edge of each class: boundary in the first probe, in
probes 2 - 4, beyond them.

The switches are read once per process, so a forced setting is a child process of its own, one at a time; after a child that exits
abnormally no further child is started."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = O.get_seed(11, 0)
SPAN = O.seed_length(PAT)
CARE = [i for i, ch in enumerate(bin(PAT)[2:]) if ch == "1"]
CHUNK, PROBE = 2048, 64                      # join_hash's nominal chunk, chunk_bound's probe
MEM, PAIRWISE = O.MODE_MEM, O.MODE_PAIRWISE


def _other(x):
    return np.uint8(int(x) ^ 1)


def _rc(s):
    return (3 - s)[::-1]


class _Planter:
    """copies of stretches of genome 0 in the other genomes, one behind the other, with the bases around a copy unequal to genome 0's"""

    def __init__(self, gs):
        self.gs = gs
        self.at = [0] + [200] * (len(gs) - 1)

    def plant(self, a, b, edit=None):
        g0 = self.gs[0]
        for k in range(1, len(self.gs)):
            d = self.at[k]
            self.gs[k][d:d + b - a] = g0[a:b]
            if a > 0:
                self.gs[k][d - 1] = _other(g0[a - 1])
            if b < len(g0):
                self.gs[k][d + b - a] = _other(g0[b])
            if edit is not None:
                self.gs[k][d + edit - a] = _other(g0[edit])
            self.at[k] = d + b - a + 40 + 7 * k


# ---- the genome sets -------------------------------------------------------------------------------------------------------------
TILE_L0 = 13000
STARTS = (0, 1024, 2047, 3073, 5121, 6144)               # stretches of 60 bases from these windows of genome 0
HALO_EDGE, STRADDLE_EDGE, JUNCTION = 8192, 12288, 4096


def _halo_base():
    """the base behind HALO_EDGE whose substitution leaves hits q < HALO_EDGE <= p with no hit between and 1 < p - q <= span"""
    for b in range(HALO_EDGE, HALO_EDGE + SPAN):
        dead = {b - t for t in CARE}
        alive = [w for w in range(HALO_EDGE - 2 * SPAN, HALO_EDGE + 2 * SPAN) if w not in dead]
        q, p = max(w for w in alive if w < HALO_EDGE), min(w for w in alive if w >= HALO_EDGE)
        if 1 < p - q <= SPAN:
            return b
    raise AssertionError("no base behind the edge gives a halo pair")


@functools.lru_cache(None)
def tile_genomes():
    rng = np.random.default_rng(1301)
    gs = [rng.integers(0, 4, L, dtype=np.uint8) for L in (TILE_L0, 13007, 12991)]
    pl = _Planter(gs)
    for s in STARTS:
        pl.plant(s, s + 60)
    pl.plant(JUNCTION - 56, JUNCTION - 1 + SPAN)          # windows 4040 .. 4095
    pl.plant(JUNCTION, JUNCTION + 60)                      # windows 4096 ..: another diagonal, one window on
    pl.plant(HALO_EDGE - 60, HALO_EDGE + 70, edit=_halo_base())
    pl.plant(STRADDLE_EDGE - 38, STRADDLE_EDGE + 42)
    pl.plant(TILE_L0 - 60, TILE_L0)
    return gs


@functools.lru_cache(None)
def tiny_genomes():
    rng = np.random.default_rng(1302)
    gs = [rng.integers(0, 4, L, dtype=np.uint8) for L in (2500, 2507, 2491)]
    pl = _Planter(gs)
    for s in (0, 1020, 2047, 2500 - 60):
        pl.plant(s, s + 60)
    return gs


@functools.lru_cache(None)
def pair_genomes(n):
    """a stretch of 40 bases per pair (i, j), at 100 * (stretches the genome holds already); pair (0, 1)'s at base 0 of genome 0"""
    rng = np.random.default_rng(1303 + n)
    gs = [rng.integers(0, 4, 4000 + 3 * g, dtype=np.uint8) for g in range(n)]
    held = [0] * n
    for i in range(n):
        for j in range(i + 1, n):
            s = rng.integers(0, 4, 40, dtype=np.uint8)
            for g in (i, j):
                gs[g][100 * held[g]:100 * held[g] + 40] = s if g == i or (i + j) % 3 else _rc(s)
                held[g] += 1
    return gs


@functools.lru_cache(None)
def hit_genomes(n):
    rng = np.random.default_rng(1304 + n)
    anc = rng.integers(0, 4, 1500, dtype=np.uint8)
    gs = []
    for g in range(n):
        x = anc.copy()
        x[37 + 11 * g::97 + g] ^= 1
        gs.append(_rc(x) if g == 2 else x)
    return gs


BOUND_SEED = 1305


@functools.lru_cache(None)
def bound_genomes(seed=BOUND_SEED):
    rng = np.random.default_rng(seed)
    g0, g1 = rng.integers(0, 4, 21000, dtype=np.uint8), rng.integers(0, 4, 20500, dtype=np.uint8)
    g0[3000:3000 + 1000 + SPAN - 1] = 1                     # 1 000 windows of C only: one mer
    g0[2999], g0[3000 + 1000 + SPAN - 1] = 0, 0
    for a, d in ((500, 700), (9000, 12000), (15000, 4000)):
        g1[d:d + 300] = g0[a:a + 300]
    return [g0, g1]


def bound_classes(gs):
    """the reference's sorted mer lists, ordered by the bits the partial sort orders, cut at multiples of CHUNK: per chunk edge the distance
    to the first bucket boundary at or behind it -> how many edges find it in the first probe, in probes 2 - 4, beyond them"""
    bits = 2 * len(CARE)
    keys = np.concatenate([O.sorted_mer_list(g, PAT)[0] >> np.uint64(64 - bits) for g in gs])      # (the list's mers are left-aligned, strand in bit 0)
    n = len(keys)
    sorted_bits = 0
    while sorted_bits < bits and (n >> sorted_bits) > 512:
        sorted_bits += 8
    high = np.sort(keys >> np.uint64(bits - min(sorted_bits, bits)))
    first = second = far = 0
    for start in range(CHUNK, n, CHUNK):
        same = np.flatnonzero(high[start:] != high[start - 1])
        d = int(same[0]) if len(same) else n - start
        first += d < PROBE; second += PROBE <= d < 4 * PROBE; far += d >= 4 * PROBE
    return n, sorted_bits, first, second, far


# ---- what the oracle says, once ---------------------------------------------------------------------------------------------------
SETTINGS = tuple((mask, extend) for mask in ("all", 0) for extend in (True, False))


@functools.lru_cache(None)
def expected(kind, n=0):
    gs = {"tile": tile_genomes, "tiny": tiny_genomes, "bound": bound_genomes}[kind]() if kind != "pairs" else pair_genomes(n)
    if kind == "pairs":
        return {ext: O.find_matches(gs, PAT, mode=PAIRWISE, extend=ext) for ext in (True, False)}
    full = (1 << len(gs)) - 1
    return {(mask, ext): O.find_matches(gs, PAT, mode=MEM, mask=full if mask == "all" else 0, extend=ext) for mask, ext in SETTINGS}


# ---- the device side: runs in this process (unforced) or in a child (forced) ----------------------------------------------------------
def _same(got, want, what):
    assert len(got[0]) == len(want[0]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def run_finder(ctx, kind):
    gs = {"tile": tile_genomes, "tiny": tiny_genomes, "bound": bound_genomes}[kind]()
    ctx.set_genomes(gs)
    full = (1 << len(gs)) - 1
    for mask, ext in SETTINGS:
        _same(ctx.seed_mums(PAT, mode=MEM, mask=full if mask == "all" else 0, extend=ext), expected(kind)[(mask, ext)], (kind, mask, ext))


def run_pairs(ctx, n):
    ctx.set_genomes(pair_genomes(n))
    for ext in (True, False):
        _same(ctx.seed_mums(PAT, mode=PAIRWISE, extend=ext), expected("pairs", n)[ext], ("pairs", n, ext))


def run_hits(ctx, n):
    from tests import seed_ref as R
    gs = hit_genomes(n)
    hits = R.find(gs, PAT)["hits"]
    assert len(hits) > 100
    order = np.random.default_rng(len(hits)).permutation(len(hits))
    m = np.array([hits[i][0] for i in order], np.uint32)
    p, s = np.zeros((len(hits), n), np.int64), np.zeros((len(hits), n), np.uint8)
    for row, i in enumerate(order):
        for g, w, f in zip(*hits[i][1:]):
            p[row, g], s[row, g] = w, f
    ctx.set_genomes(gs)
    for ext in (True, False):
        want = O.find_matches(gs, PAT, mode=MEM, extend=ext)
        assert len(want[0]) > 0
        _same(ctx.extend_hits(PAT, m, p, s, extend=ext), want, ("hits", n, ext))


def run_jobs(jobs):
    from mauvealigner_amd import _lib
    ctx = _lib.Context(0)
    try:
        for job in jobs:
            kind, _, arg = job.partition(":")
            if kind == "pairs":
                run_pairs(ctx, int(arg))
            elif kind == "hits":
                run_hits(ctx, int(arg))
            else:
                run_finder(ctx, kind)
            print("done", job, flush=True)
    finally:
        ctx.close()


_abnormal = []
_DEVICE_FAULT = re.compile(r"illegal memory access|hipError|HIP error|\bhip[A-Z]\w*\(.*\): |HSA_STATUS_ERROR|Memory access fault|unspecified launch failure")


@functools.lru_cache(None)
def _child(jobs, env):
    """-> (return code, stdout, stderr) of a fresh process that runs the jobs with env (a tuple of pairs) in its environment"""
    if _abnormal:
        return (None, "", "not started: the child of %s exited abnormally" % (_abnormal[0],))
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_seed_run_tiles as T; T.run_jobs(sys.argv[1:]); print('OK')" % ROOT
    full = {k: v for k, v in os.environ.items() if k != "MAUVE_RUNS_ITEMS"}
    full.update(dict(env))
    try:
        r = subprocess.run([sys.executable, "-c", code] + list(jobs), env=full, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _abnormal.append((jobs, env))
        raise
    if r.returncode < 0 or r.returncode in (134, 139) or (r.returncode != 0 and _DEVICE_FAULT.search(r.stderr)):
        _abnormal.append((jobs, env))
    return (r.returncode, r.stdout, r.stderr)


def _child_did(jobs, env, job):
    rc, out, err = _child(jobs, env)
    assert rc == 0 and out.strip().endswith("OK") and ("done " + job) in out.splitlines(), "child exit %s: " % rc + out[-1500:] + err[-3000:]


FORCED_JOBS = ("tile", "pairs:3", "pairs:9")


def _forced(items, job):
    _child_did(FORCED_JOBS, (("MAUVE_RUNS_ITEMS", str(items)),), job)


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ---- the planted classes are there (the oracle alone) ----------------------------------------------------------------------------------
def _tile_classes():
    gs = tile_genomes()
    span = SPAN
    assert sum(len(g) - span + 1 for g in gs) > 9216 and (len(gs[0]) - span + 1) // 4096 == 3
    for mask in ("all", 0):
        eln, est = expected("tile")[(mask, True)]
        hln, hst = expected("tile")[(mask, False)]
        three = (est != 0).all(axis=1)
        first = est[three][:, 0] - 1
        for s in STARTS + (JUNCTION,):
            assert s in first, ("no match of all three genomes starts at window", s)
        last = first + eln[three] - span                       # last window of the match in genome 0
        assert (last == len(gs[0]) - span).any() and (first == 0).any()
        assert ((first < STRADDLE_EDGE) & (last >= STRADDLE_EDGE)).any(), "no match straddles the edge"
        h3 = (hst != 0).all(axis=1)
        assert (hln == span).all()
        hw = hst[h3][:, 0] - 1
        diag = {int(w): tuple(r[1:] - r[0]) for w, r in zip(hw, hst[h3])}
        assert JUNCTION - 1 in diag and JUNCTION in diag and diag[JUNCTION - 1] != diag[JUNCTION], "no two diagonals across the edge"
        q, p = max(w for w in diag if w < HALO_EDGE), min(w for w in diag if w >= HALO_EDGE)
        assert 1 < p - q <= span and diag[p] == diag[q] and p - HALO_EDGE < span, ("no halo pair", q, p)


def _pair_classes(n):
    for ext in (True, False):
        eln, est = expected("pairs", n)[ext]
        for i in range(n):
            for j in range(i + 1, n):
                want = np.zeros(n, bool); want[[i, j]] = True
                sel = ((est != 0) == want).all(axis=1) & (eln >= (40 if ext else SPAN))
                assert sel.any(), ("no match of the pair", i, j)
                if (i, j) == (0, 1):
                    assert (est[sel][:, 0] == 1).any(), "no match at the first window of genome 0"


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("items", [4, 8, 16])
def test_tile_edges_forced(items):
    _tile_classes()
    _forced(items, "tile")


@pytest.mark.gpu
def test_tile_edges_by_the_rule(ctx):
    _tile_classes()
    run_finder(ctx, "tile")


@pytest.mark.gpu
def test_tiny_launch(ctx):
    gs = tiny_genomes()
    assert sum(len(g) - SPAN + 1 for g in gs) <= 9216
    for key in SETTINGS:
        eln, est = expected("tiny")[key]
        first = est[(est != 0).all(axis=1)][:, 0] - 1
        assert all(s in first for s in (0, 1020, 2047, 2500 - 60)), key
    run_finder(ctx, "tiny")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("items", [4, 8, 16])
def test_pair_groups_forced(items, n):
    _pair_classes(n)
    _forced(items, "pairs:%d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 9])
def test_pair_groups_by_the_rule(ctx, n):
    _pair_classes(n)
    run_pairs(ctx, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 9])
def test_host_hits_wide_index(n):
    _child_did(("hits:5", "hits:9"), (("MAUVE_WIDE_INDEX", "1"),), "hits:%d" % n)


@pytest.mark.gpu
def test_chunk_bounds():
    n, sorted_bits, first, second, far = bound_classes(bound_genomes())
    assert 38000 <= n <= 42000 and sorted_bits == 8, (n, sorted_bits)
    assert first > 0 and second > 0 and far > 0, ("chunk edges by the probe that finds the boundary", first, second, far)
    assert all(len(expected("bound")[key][0]) > 0 for key in SETTINGS)
    _child_did(("bound",), (("MAUVE_NO_TINY", "1"),), "bound")
