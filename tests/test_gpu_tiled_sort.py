"""The tiled sort (mauvealigner_amd/csrc/tiled_sort.hpp): its standalone driver against std::stable_sort (tests/cpp/tiled_sort_test.cpp: tile
counts around the 8 classes of the tile order and the row-scan threshold, ragged last tiles, key patterns for the ranking, all four pair
widths, the bit ranges, the first pass from a strand bitmap), and through the library: one seed pass of two genomes whose 299 000 windows
are 73 tiles with a ragged last one -- the row-scan path, the histogram seed_extract_all leaves read in tile order -- against the oracle's
match list, as the process finds it, with 64-bit values (MAUVE_WIDE_INDEX=1) and with the small-sort engine off (MAUVE_SMALL_SORT=0).

The switches are read once per process, so a forced setting is a child process of its own; the child writes what the device found to
a file and the comparison with the oracle's list, computed once, is made here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as O
from tests.test_gpu_seed_run_tiles import MEM, PAT, SPAN, _Planter, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
MASKS = (0, 3)


@pytest.mark.gpu
def test_tiled_sort_driver_matches_stable_sort(tmp_path):
    exe = str(tmp_path / "tiled_sort_test")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "tiled_sort_test.cpp"), "-o", exe], timeout=600)
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]


@functools.lru_cache(None)
def genomes():
    rng = np.random.default_rng(1401)
    gs = [rng.integers(0, 4, L, dtype=np.uint8) for L in (149500 + SPAN - 1, 149500 + SPAN - 1)]
    pl = _Planter(gs)
    for s in (0, TILE - 30, 36 * TILE + 7, 149500 - 80):         # stretches of 60 bases: the first windows, across a tile edge, mid-list, the end
        pl.plant(s, s + 60)
    return gs


@functools.lru_cache(None)
def expected():
    gs = genomes()
    n = sum(len(g) - SPAN + 1 for g in gs)
    assert n == 299000 and (n + TILE - 1) // TILE == 73 and n % TILE != 0
    # mask 0: every window goes into the sort, the first pass takes seed_extract_all's histogram and strand bitmap; mask 3: the compacted
    # list, whose first histogram is rs_hist's
    want = [O.find_matches(gs, PAT, mode=MEM, mask=mask, extend=True) for mask in MASKS]
    assert all(len(w[0]) >= 4 for w in want)
    return want


def seed_pass():
    from mauvealigner_amd import _lib
    ctx = _lib.Context(0)
    try:
        ctx.set_genomes(genomes())
        return [ctx.seed_mums(PAT, mode=MEM, mask=mask, extend=True) for mask in MASKS]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_seed_pass_of_73_tiles():
    for got, want, mask in zip(seed_pass(), expected(), MASKS):
        _same(got, want, ("mask", mask))


@pytest.mark.gpu
@pytest.mark.parametrize("name,value", [("MAUVE_WIDE_INDEX", "1"), ("MAUVE_SMALL_SORT", "0")])
def test_seed_pass_of_73_tiles_forced(tmp_path, name, value):
    want = expected()
    out = str(tmp_path / "got.npz")
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; from tests import test_gpu_tiled_sort as T; "
            "r = T.seed_pass(); np.savez(sys.argv[1], **{'%%s%%d' %% (k, i): a for i, p in enumerate(r) for k, a in zip(('ln', 'st'), p)}); print('OK')" % ROOT)
    env = dict(os.environ)
    env[name] = value
    r = subprocess.run([sys.executable, "-c", code, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), "child exit %s: " % r.returncode + r.stdout[-1500:] + r.stderr[-3000:]
    got = np.load(out)
    for i, mask in enumerate(MASKS):
        _same((got["ln%d" % i], got["st%d" % i]), want[i], (name, value, "mask", mask))
