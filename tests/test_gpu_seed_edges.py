"""The seed pass (csrc/seed_pass.hip: tiny_join, join_hash with chunk_bound and the overflow slices, mum_runs, mum_extend) on the
planted genome sets of tests/seed_cases.py: buckets of the partially sorted list at 3071 / 3072 / 3073 entries from their chunk's
start, bucket boundaries 0 .. 257 entries behind a chunk edge, several overflow slices in one pass, 16 | 17 genomes, the routes of
seed_plan at 9215 | 9216 | 9217 windows, hits over the tile and wave edges of mum_runs, junctions and the phase-3 shape, walks over
repeats of 62 .. 66, 126 .. 130 and 200 offsets, gaps of span - 1 | span offsets around the round edge, genome ends, 9 / 12 / 32
components, contigs and ambiguous bases, and caller-made patterns of span 1 .. 49.  tests/test_seed_cpu.py shows from the
reference's facts that every case is where it was aimed.

Every case runs twice through ctx.seed_mums (equal results); lengths and starts must be the oracle's, and on the cases of up to
SMALL windows those of tests/seed_ref.py directly.  The trace must show the case's window count, the route that seed_cases.py
derives from the stated geometry (tiny_join, or the hash join) and, for a list whose ranges the reference's key table puts
beyond the limit, the line `join_hash handed back K range(s)` with that K -- no such line otherwise.  After a case that overflowed,
one that does not runs on the same context (the overflow path reuses the sort buffers and the counter block).

The switches are read once per process, so every variant is a child process of its own with a time limit: the default,
MAUVE_NO_TINY=1 (every small case through join_hash and the radix passes), MAUVE_SMALL_SORT=0 (with MAUVE_NO_TINY=1, so that the
small lists are sorted at all) and MAUVE_WIDE_INDEX=1 (the wide
instantiations on the bucket, tile and walk families); MAUVE_TRACE=1 in all.  After a child that exits abnormally -- a signal, an
abort, its time limit, or a failed HIP call in what it wrote to stderr -- no further child is started."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, re, sys, tempfile
import numpy as np
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib
from oracle import pyoracle as O
from tests import seed_cases as C, seed_ref as R

SMALL = 10000
no_tiny = "MAUVE_NO_TINY" in os.environ
wide = os.environ.get("MAUVE_WIDE_INDEX") == "1"


class Stderr:                                    # what the library writes to stderr during one call
    def __enter__(self):
        sys.stderr.flush()
        self.f = tempfile.TemporaryFile()
        self.old = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self
    def __exit__(self, *a):
        os.dup2(self.old, 2); os.close(self.old)
        self.f.seek(0); self.text = self.f.read().decode(errors="replace"); self.f.close()


def expected(case):
    valid = C.valid_intervals(case)
    if valid is None:
        return O.find_matches(case["genomes"], case["pattern"], mode=case["mode"], mask=case["mask"], extend=case["extend"])
    return O.find_matches_masked(case["genomes"], case["pattern"], valid, mode=case["mode"], mask=case["mask"], extend=case["extend"])


def run(ctx, case):
    ctx.set_genomes(case["genomes"], contig_starts=case["contigs"], invalid=case["invalid"])
    out = []
    for _ in range(2):
        with Stderr() as cap:
            ln, st = ctx.seed_mums(case["pattern"], mode=case["mode"], mask=case["mask"], extend=case["extend"])
        out.append((ln, st, cap.text))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), (case["name"], "two calls differ")
    return out


def check(ctx, case):
    name = case["name"]
    eln, est = expected(case)
    P = C.windows_of(case)
    ref = None
    if P <= SMALL:
        ref = R.find(case["genomes"], case["pattern"], mode=case["mode"], mask=case["mask"], extend=case["extend"], valid=C.valid_intervals(case))
        assert eln.tolist() == ref["length"] and est.tolist() == ref["start"], (name, "oracle against reference")
    tiny, hashed = C.takes_tiny(case, no_tiny), C.takes_hash_join(case, no_tiny)
    K = len(C.geometry_of(case)["declined"]) if hashed and C.valid_intervals(case) is None else None
    for ln, st, text in run(ctx, case):
        assert len(ln) == len(eln) and np.array_equal(ln, eln) and np.array_equal(st, est), (name, "against the oracle", len(ln), len(eln))
        if P == 0:
            continue
        seen = re.findall(r"seed pass: (\d+) windows, \d+-bit keys, (\w+) window index", text)
        assert seen == [(str(P), "wide" if wide else "narrow")], (name, seen, P)
        assert ("runs + extend (one round trip)" in text) == tiny, (name, "route", tiny, text[-800:])
        back = [int(x) for x in re.findall(r"join_hash handed back (\d+) range", text)]
        if K is not None:
            assert back == ([K] if K else []), (name, "declined ranges", back, K)
        else:
            assert not back or hashed, (name, back)
    return tiny, hashed, bool(K)


ctx = _lib.Context(0)
after = next(c for c in C.route_cases() if c["name"] == "windows_9217")        # the hash join in every variant, nothing declined
for fam in sys.argv[1:]:
    n = n_tiny = n_hash = n_over = 0
    if fam == "callback":
        for case in C.callback_cases():
            ref = R.find(case["genomes"], case["pattern"])
            hits = ref["hits"]
            N = len(case["genomes"])
            order = np.random.default_rng(len(hits)).permutation(len(hits))
            m = np.array([hits[i][0] for i in order], np.uint32)
            p, s = np.zeros((len(hits), N), np.int64), np.zeros((len(hits), N), np.uint8)
            for row, i in enumerate(order):
                for g, w, f in zip(*hits[i][1:]):
                    p[row, g], s[row, g] = w, f
            ctx.set_genomes(case["genomes"])
            for ext in (True, False):
                ln, st = ctx.extend_hits(case["pattern"], m, p, s, extend=ext)
                eln, est = ctx.seed_mums(case["pattern"], extend=ext)
                assert len(ln) > 0 and np.array_equal(ln, eln) and np.array_equal(st, est), (case["name"], ext)
                if ext:
                    assert ln.tolist() == ref["length"] and st.tolist() == ref["start"], case["name"]
            n += 1
        print("family", fam, n, 0, 0, 0)
        continue
    for case in C.family(fam):
        tiny, hashed, over = check(ctx, case)
        n += 1; n_tiny += tiny; n_hash += hashed; n_over += over
        if over:
            t, h, o = check(ctx, after)
            assert h and not o
    print("family", fam, n, n_tiny, n_hash, n_over)
ctx.close()
print("OK")
"""

_abnormal = []
# (the library's message for a failed HIP call is "<the call>: <hipGetErrorString> (file:line)")
_DEVICE_FAULT = re.compile(r"illegal memory access|hipError|HIP error|\bhip[A-Z]\w*\(.*\): |HSA_STATUS_ERROR|Memory access fault|unspecified launch failure")


def _child(families, **env):
    if _abnormal:
        pytest.fail("not started: the child of %s exited abnormally" % _abnormal[0])
    full = dict(os.environ, MAUVE_TRACE="1", **env)
    try:
        r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}] + list(families), env=full, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _abnormal.append(families)
        raise
    # killed by a signal, aborted, or a device fault that HIP reported as an error and Python as an exception (exit 1)
    if r.returncode < 0 or r.returncode in (134, 139) or (r.returncode != 0 and _DEVICE_FAULT.search(r.stderr)):
        _abnormal.append(families)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), "child exit %d: " % r.returncode + r.stdout[-2000:] + r.stderr[-3000:]
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("family ")]
    return {row[1]: tuple(int(x) for x in row[2:]) for row in rows}


ALL = ["bucket", "route", "tile", "walk", "pattern", "callback"]


@pytest.mark.gpu
def test_planted_cases_default_routes():
    got = _child(ALL)
    n, tiny, hashed, over = got["bucket"]
    assert n == hashed and tiny == 0 and over == 18                  # every bucket case takes the hash join; the ones beyond the limit hand ranges back
    n, tiny, hashed, over = got["route"]
    assert tiny == 18 and hashed == 11 and over == 0                     # 9217 windows, 17 genomes, weight 17, the longer masked sets: not tiny
    assert got["walk"][1] > 0 and got["walk"][2] > 0 and got["pattern"][1] > 0 and got["callback"][0] == 4
    assert got["tile"][2] > 0 and got["tile"][0] > got["tile"][2]       # (the pairwise cases take neither)


@pytest.mark.gpu
def test_every_case_through_the_hash_join():
    """MAUVE_NO_TINY=1: the small cases -- genome ends, masked stops, caller-made patterns, the routes -- through the partial sort,
    join_bounds / join_hash and the radix passes"""
    got = _child(ALL, MAUVE_NO_TINY="1")
    assert all(got[f][1] == 0 for f in got)
    assert got["route"][2] == got["route"][0] and got["pattern"][2] == got["pattern"][0] and got["walk"][2] == got["walk"][0]


@pytest.mark.gpu
def test_tiled_sorts_only():
    """MAUVE_SMALL_SORT=0: the overflow slices and the small lists take the tiled radix passes"""
    got = _child(["bucket", "route", "tile", "pattern"], MAUVE_SMALL_SORT="0", MAUVE_NO_TINY="1")
    assert got["bucket"][3] == 18 and got["tile"][0] > 0


@pytest.mark.gpu
def test_wide_window_index():
    """MAUVE_WIDE_INDEX=1: the 64-bit-value instantiations on the bucket, tile and walk families"""
    got = _child(["bucket", "tile", "walk"], MAUVE_WIDE_INDEX="1")
    assert got["bucket"][3] == 18 and got["tile"][0] > 0 and got["walk"][0] > 0
