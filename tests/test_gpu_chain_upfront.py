"""The chain stage with every genome's order and overlap clusters made up front (chain_device_graph, chain_dev.hip): the clusters
of all genomes are cut from the list as it enters the stage, and a genome's elimination is one launch.  The survivors must be
those of the oracle's whole-list elimination.

Random dense lists -- N = 2..4 genomes, 2..119 matches, lengths 1..59, starts in [1, span) with span 200..4000, 40 % reverse
components in genomes >= 1, lists with tied genome-0 starts kept and every list handed over in canonical order (the index that
decides among equal left ends is the caller's order for the oracle and the canonical one for the product:
tests/test_chain_cpu.py) -- go through ctx.align_matches (recursive=0, gapped=0,
extend_lcbs=0, lcb_weight=0: every LCB stays), which puts a caller's list where the seed pass leaves its own when
MAUVE_CANON_DEVICE_MIN=1, so chain_device_graph chains it.  The switches are read once per process: every variant runs in a
process of its own -- the default, MAUVE_CH_CL_MAX=2 (clusters of three and more hand the list back to the host chain) and
MAUVE_SMALL_SORT=0 (the batched sort falls back to one tiled sort per genome).  The segmented form (a recursion batch: all N
genomes sorted, matches that start dead) is a small C5-shaped pair through ctx.align with the recursion on."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTS_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib
from oracle import pyoracle as O
from tests import chain_ref
rng = np.random.default_rng(1)
cases = []
tied = 0
for _ in range(400):
    N = int(rng.integers(2, 5)); n = int(rng.integers(2, 120)); span = int(rng.integers(200, 4001))
    ln = rng.integers(1, 60, n).astype(np.int64)
    st = rng.integers(1, span, (n, N)).astype(np.int64)
    rev = rng.random((n, N)) < 0.4
    rev[:, 0] = False
    st[rev] = -st[rev]
    tied += len(np.unique(st[:, 0])) < n
    ln, st = chain_ref.canonicalise(ln, st)
    cases.append((span, np.asarray(ln, np.int64), np.asarray(st, np.int64)))
assert tied > 0
print("lists", len(cases), "small", sum(len(c[1]) <= 48 for c in cases))
assert len(cases) >= 100
ctx = _lib.Context(0)
p = _lib.default_params(recursive=0, gapped=0, extend_lcbs=0, lcb_weight=0)
grng = np.random.default_rng(2)
killed = 0
for span, ln, st in cases:
    N = st.shape[1]
    ctx.set_genomes([grng.integers(0, 4, span + 64, dtype=np.uint8) for _ in range(N)])
    r = ctx.align_matches(p, ln, st)
    el, es = O.eliminate_overlaps(ln, st)
    got = sorted((int(l), tuple(int(x) for x in s)) for l, s in zip(r["anchor_length"], r["anchor_start"]))
    want = sorted((int(l), tuple(int(x) for x in s)) for l, s in zip(el, es))
    assert got == want, (N, len(ln), span, len(got), len(want))
    killed += len(ln) - len(want)
assert killed > 0                                   # (the lists are dense: the elimination has work to do)
ctx.close()
print("OK")
"""

SEG_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r)
from mauvealigner_amd import _lib, synth
from oracle import pyoracle as O
gs = synth.make_config("C5", scale=0.004)
ctx = _lib.Context(0)
ctx.set_genomes(gs)
r = ctx.align(_lib.default_params(recursive=1))
e = O.align(gs, O.default_params(recursive=1))["aln"]
for k in ("anchor_length", "anchor_start", "anchor_lcb", "cols", "col_off", "dp_score"):
    assert np.array_equal(r[k], e[k]), k
ctx.close()
print("OK")
"""


def _run(script, **env):
    full = dict(os.environ, MAUVE_TRACE="1", MAUVE_CANON_DEVICE_MIN="1", **env)
    r = subprocess.run([sys.executable, "-c", script % {"root": ROOT}], env=full, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout.split(), r.stderr.splitlines()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"MAUVE_CH_CL_MAX": "2"}, {"MAUVE_SMALL_SORT": "0"}], ids=["default", "cl_max_2", "tiled_sorts"])
def test_random_dense_lists_equal_the_oracle(env):
    out, err = _run(LISTS_SCRIPT, **env)
    lists, small = int(out[out.index("lists") + 1]), int(out[out.index("small") + 1])
    dev = [l for l in err if "chain (device): eliminate+nodes+graph" in l]
    if "MAUVE_CH_CL_MAX" in env:
        assert len(dev) < lists, err[-20:]          # dense lists have clusters of three: those were handed back to the host chain
    else:
        assert small > 0 and len(dev) >= small, err[-20:]    # a list of up to CH_CL_MAX = 48 matches has no larger cluster: chain_device_graph chained it


@pytest.mark.gpu
def test_recursion_batch_equals_the_oracle():
    _, err = _run(SEG_SCRIPT)
    assert [l for l in err if "per-gap chaining" in l and "(device" in l], err[-20:]
