"""The backbone stage of the product (csrc/backbone_dev.hip, csrc/backbone_host.hpp) on the planted alignments of
tests/backbone_planted.py: gap runs on the island limit inside a word, across word, batch and chunk borders and with neither-columns
inside; regions that start, end and close on the chunk border or span up to 66 chunks; leading and trailing regions, chunks without a
column of the pair in front (1, 63, 64, 65 of them: both steps of the look-back over bb_chunk_last's bytes); components through chains
of pairs, 66 pairs on 64 grid rows, 32 genomes; segment and island ends on the rank tiles' and quarter-tiles' borders on both strands.
tests/test_backbone_planted_cpu.py shows from the reference that every case is where it was aimed.

Every case goes through mauve_backbone_alignment at each of its island_gap values in turn, on one context for all cases -- the island
limit cases at g and then at g + 1, so a call must give its own result and nothing of the call before -- and all seven arrays of
mauve_backbone_fetch must equal those of tests/backbone_ref.py, shapes and dtypes included.

Two routes: the default (the state in front of a chunk from bb_chunk_last's bytes) and MAUVE_BB_COLUMN_SCAN=1 (walking back over the
columns).  The switch is read once per process, so each route is a child process of its own, with a time limit; it stops at the first
mismatch and names the case.  The reference's tables are computed once, in the parent, and handed to the children in a file."""
import atexit
import functools
import os
import pickle
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import pickle, sys
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib
from tests import backbone_planted as P
from tests.backbone_ref import first_difference

with open(sys.argv[1], "rb") as f:
    WANT = pickle.load(f)


def same(r, e, what):
    diff = first_difference(r, e)
    if diff is not None:
        sys.exit("MISMATCH %%r %%s" %% (what, diff))


ctx = _lib.Context(0)
runs = 0
for fam in sys.argv[2:]:
    for c in P.family(fam):
        if c.get("sequence") not in (None, c["gaps"]):       # island_gap g and then g + 1, in this order, on the one context
            sys.exit("FAILED %%r: gaps %%r, declared sequence %%r" %% (c["name"], c["gaps"], c["sequence"]))
        for gap in c["gaps"]:
            try:
                r = ctx.backbone_alignment(*c["aln"], island_gap=gap)
            except Exception as ex:
                sys.exit("FAILED %%r: %%s" %% ((c["name"], gap), ex))
            same(r, WANT[(c["name"], gap)], (c["name"], gap))
            runs += 1
# island_gap outside 0 .. 2^31 - 1 is refused, and the call behind the refusal is not disturbed by it
c = P.family("ownership")[0]
refused = 0
for gap in (-1, 2 ** 31):
    try:
        ctx.backbone_alignment(*c["aln"], island_gap=gap)
    except RuntimeError as ex:
        refused += "(-1)" in str(ex) and "island_gap_size out of range" in str(ex)
same(ctx.backbone_alignment(*c["aln"], island_gap=c["gaps"][0]), WANT[(c["name"], c["gaps"][0])], (c["name"], "behind the refusals"))
ctx.close()
print("runs", runs, "refused", refused, "OK")
"""


@functools.lru_cache(maxsize=None)
def _wanted():
    """the reference's tables of every (case, island_gap), computed once and written where the children read them -> (path, count)"""
    from tests import backbone_planted as P, backbone_ref as R
    want = {}
    for c in P.all_cases():
        for gap in c["gaps"]:
            r = R.backbone(*c["aln"], island_gap=gap)
            want[(c["name"], gap)] = {k: r[k] for k in R.KEYS}
    fd, path = tempfile.mkstemp(suffix=".pkl", prefix="backbone_want_")
    with os.fdopen(fd, "wb") as f:
        pickle.dump(want, f)
    atexit.register(os.unlink, path)
    return path, len(want)


def _child(**env):
    from tests import backbone_planted as P
    full = {k: v for k, v in os.environ.items() if k != "MAUVE_BB_COLUMN_SCAN"}
    full.update(env)
    path, count = _wanted()
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, path] + list(P.FAMILIES), env=full, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    out = r.stdout.split()
    assert int(out[out.index("runs") + 1]) == count and int(out[out.index("refused") + 1]) == 2, r.stdout[-500:]


@pytest.mark.gpu
def test_planted_cases_with_the_start_up_state_from_the_chunk_bytes():
    _child()


@pytest.mark.gpu
def test_planted_cases_with_the_start_up_state_from_the_columns():
    """MAUVE_BB_COLUMN_SCAN=1: bb_pair_gaps walks back over the columns in front of its chunk, bb_chunk_last is not launched"""
    _child(MAUVE_BB_COLUMN_SCAN="1")
