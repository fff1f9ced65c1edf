"""The progressive path (progressive.cpp with the kernels of seed_finish.hip, dp_batch.hip and the placed-base mask of seed_pass.hip) on
the planted cases of tests/progressive_cases.py: guide tree, breakpoint counts, refinement and the walk, bit-exact against the plain
reference (tests/progressive_ref.py) and the CPU oracle.  tests/test_progressive_cpu.py holds the reference to the oracle and shows
that every case reaches the rule it aims at; it needs no GPU."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import progressive_cases as Cs
from tests import progressive_ref as R
from tests import progressive_worker as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("MAUVE_DP_DESC_MIN", "MAUVE_DP_DESC_HOST", "MAUVE_HOST_CHAIN", "MAUVE_WIDE_INDEX", "MAUVE_CANON_DEVICE_MIN")


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """the expected result of every refinement and walk set, computed once for this process and the children"""
    ref = W.reference()
    path = str(tmp_path_factory.mktemp("progressive") / "reference.pickle")
    with open(path, "wb") as f:
        pickle.dump(ref, f)
    return ref, path


def same_tree(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def hold_an_alignment(ctx, _lib):
    """leave a resident result in the context: the guide-tree passes reuse its buffers (materialize_tables)"""
    r = ctx.align(_lib.default_params(seed_weight=11))
    assert r["n_iv"] > 0


def test_guide_tree_cases(ctx):
    """mauve_guide_tree against R.distances / R.upgma and the oracle; once more with a resident alignment held, and again"""
    from mauvealigner_amd import _lib
    for c in Cs.tree_sets():
        gs = c["genomes"]
        dist = R.distances(gs, R.pair_records(gs, c["pattern"]))
        tree = R.upgma(dist)
        odist, oleft, oright = O.guide_tree(gs, c["pattern"])
        ctx.set_genomes(gs)
        for again in range(3):
            d, left, right = ctx.guide_tree(c["pattern"])
            assert np.array_equal(d, dist) and same_tree((left, right), tree), (c["name"], again)
            assert np.array_equal(d, odist) and same_tree((left, right), (oleft, oright)), (c["name"], again)
            if again == 0:
                hold_an_alignment(ctx, _lib)


def test_breakpoint_cases(ctx):
    """mauve_breakpoint_counts against R.breakpoint_counts and the oracle at every floor of every case; with a resident alignment held too"""
    from mauvealigner_amd import _lib
    for c in Cs.bp_sets():
        gs, N = c["genomes"], len(c["genomes"])
        rec = R.pair_records(gs, c["pattern"])
        ctx.set_genomes(gs)
        for again in range(3):
            for min_len, want in c["runs"]:
                bp = ctx.breakpoint_counts(c["pattern"], min_len)
                assert np.array_equal(bp, R.breakpoint_counts(rec, N, min_len)), (c["name"], min_len, again)
                assert np.array_equal(bp, O.breakpoint_counts(gs, c["pattern"], min_len)), (c["name"], min_len, again)
                for (a, b), v in want.items():
                    assert bp[a, b] == v, (c["name"], min_len, a, b)
            if again == 0:
                hold_an_alignment(ctx, _lib)


def test_breakpoint_sweep_with_duplications(ctx):
    """overlapping records and equal starts in the lower genome (Cs.DUP_SEED): the total order of S11c"""
    for seed in range(Cs.DUP_SEED, Cs.DUP_SEED + 24):
        gs = Cs.dup_pair(seed)
        rec = R.pair_records(gs, Cs.P11)
        ctx.set_genomes(gs)
        for min_len in (0, 22):
            assert np.array_equal(ctx.breakpoint_counts(Cs.P11, min_len), R.breakpoint_counts(rec, 2, min_len)), (seed, min_len)


def test_refinement_and_walk_sets(ctx, reference):
    """every refinement set (rounds 1, 2, 9), the clade set along its tree and every walk set at default switches: the library against
    the interval assembled from the reference, against the oracle, and check_walk on every result"""
    from mauvealigner_amd import _lib
    W.run(ctx, _lib, reference[0])


ROUTES = {
    "device_rotations": ({"MAUVE_DP_DESC_MIN": "1"}, "descriptor batch, device front"),
    "host_chain": ({"MAUVE_HOST_CHAIN": "1"}, None),
    "wide_index": ({"MAUVE_WIDE_INDEX": "1"}, "wide window index"),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_refinement_and_walk_sets_in_a_child(route, reference):
    """the same in a child process with one switch set on it alone.  MAUVE_DP_DESC_MIN=1 sends every node's batch through the device front,
    where the rotated candidates are made by dpf_rotate_desc: planted intervals with empty slots, k < N and neighbours without candidates
    instead of bulk input; the trace must show that route.  MAUVE_HOST_CHAIN=1: the root's chain on the host.  MAUVE_WIDE_INDEX=1: the
    64-bit seed pass under the placed-base mask"""
    extra, trace = ROUTES[route]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra, MAUVE_TRACE="1")
    r = subprocess.run([sys.executable, "-m", "tests.progressive_worker", reference[1]], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "OK", str(extra) + "\n" + r.stdout[-2000:] + r.stderr[-4000:]
    if trace:
        assert trace in r.stderr, r.stderr[-2000:]
    if route == "device_rotations":                    # rotations were made there, and some of them won
        found = re.findall(r"refinement: (\d+) candidate alignments of (\d+) intervals, (\d+) replaced", r.stderr)
        assert any(int(c) > 0 and int(w) > 0 for c, n, w in found), r.stderr[-2000:]
