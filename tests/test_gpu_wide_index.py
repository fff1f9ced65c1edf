"""Genome sets of 2^31 bases or more: the limits of mauve_set_genomes*  and the wide seed pass (64-bit window
indices).  MAUVE_WIDE_INDEX=1 forces the wide instantiations for every pass, so the oracle's small inputs check
them bit for bit: a child process runs the parity tests of the seed pass, the aligner and the repeat penalty with it set."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(args, env_extra, timeout):
    env = dict(os.environ)
    env.update(env_extra)
    return subprocess.run([sys.executable] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


# every finder mode, recursion (segmented keys), contigs and ambiguity bitmaps, the extension rounds, extend_hits, SP scoring with the
# repeat penalty, progressive with and without a tree, the multiplicity pass, sorted lists and the enumerator, the planted guide-tree and
# breakpoint cases
WIDE_MATRIX = [
    "tests/test_gpu_seed.py",
    "tests/test_gpu_align.py::test_align_equals_oracle",
    "tests/test_gpu_align.py::test_align_options",
    "tests/test_gpu_align.py::test_align_recursion_hyperdivergent",
    "tests/test_gpu_align.py::test_lcb_extension",
    "tests/test_gpu_align.py::test_lcb_extension_on_the_device",
    "tests/test_gpu_align.py::test_sp_lcb_scoring",
    "tests/test_gpu_align.py::test_guide_tree_and_progressive_align",
    "tests/test_gpu_align.py::test_progressive_align_along_a_given_tree",
    "tests/test_gpu_repeat_penalty.py::test_multiplicity_matches_reference",
    "tests/test_gpu_repeat_penalty.py::test_penalized_alignments_equal_oracle",
    "tests/test_gpu_progressive.py::test_guide_tree_cases",
    "tests/test_gpu_progressive.py::test_breakpoint_cases",
]


def test_forced_wide_index_parity_matrix():
    r = _child(["-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu"] + WIDE_MATRIX, {"MAUVE_WIDE_INDEX": "1"}, 1500)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert " passed" in r.stdout and " skipped" not in r.stdout and " failed" not in r.stdout, r.stdout[-2000:]


_TRACE_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from mauvealigner_amd import _lib, synth
from oracle import pyoracle as O
gs = synth.make_config("C3", scale=0.01)
c = _lib.Context(0)
c.set_genomes(gs)
for pat in (O.get_seed(11, 0), O.get_seed(19, 0)):
    for mode, mask in ((0, 0), (1, 0), (2, 0)):
        ln, st = c.seed_mums(pat, mode=mode, mask=mask)
        eln, est = O.find_matches(gs, pat, mode=mode, mask=mask)
        assert np.array_equal(ln, eln) and np.array_equal(st, est), (pat, mode)
m = c.seed_multiplicity(1, O.get_seed(11, 0))
assert np.array_equal(m, O.seed_multiplicity(gs[1], O.get_seed(11, 0)))
c.close()
print("child ok")
"""


@pytest.mark.parametrize("wide", [False, True])
def test_trace_states_the_index_width(wide):
    """MAUVE_TRACE: every seed pass (and the multiplicity pass) names the width it ran; small sets run narrow unless forced."""
    env = {"MAUVE_TRACE": "1", "MAUVE_WIDE_INDEX": "1" if wide else "0"}
    r = _child(["-c", _TRACE_SCRIPT % ROOT], env, 600)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [s for s in r.stderr.splitlines() if "window index" in s]
    assert any("seed pass:" in s for s in lines) and any("multiplicity pass:" in s for s in lines), r.stderr[-2000:]
    want, other = ("wide window index (64-bit values)", "narrow") if wide else ("narrow window index (32-bit values)", "wide")
    assert all(want in s for s in lines) and not any(other in s for s in lines), lines


def test_genome_set_limits():
    """One genome of 2^31 bases, or genomes of 2^32 - 2^20 bases together, are refused with MAUVE_ERR_LIMIT before any upload
    (the message names the limit); the context stays usable and the next small call equals the oracle."""
    from mauvealigner_amd import _lib
    ctx = _lib.Context(0)
    try:
        big = 1 << 31
        zeros = np.zeros(_lib.load().mauve_packed_words(big), np.uint64)        # never touched: refused before the upload
        with pytest.raises(RuntimeError, match=r"\(-4\).*genome 0 .*per-genome limit"):
            ctx.set_genomes_packed([zeros], [big])
        half = big - 1
        with pytest.raises(RuntimeError, match=r"\(-4\).*total limit"):
            ctx.set_genomes_packed([zeros, zeros], [half, half])                   # each below 2^31, together past the total limit
        with pytest.raises(RuntimeError, match=r"\(-4\).*total limit"):
            ctx.set_genomes_packed([zeros, zeros, zeros], [half, half, half])
        assert int(_lib.MAX_GENOME_LEN) == 1 << 31 and int(_lib.MAX_TOTAL_LEN) == (1 << 32) - (1 << 20)
        del zeros
        gs = synth.make_config("C3", scale=0.01)
        ctx.set_genomes(gs)
        pat = O.get_seed(11, 0)
        ln, st = ctx.seed_mums(pat)
        eln, est = O.find_matches(gs, pat)
        assert np.array_equal(ln, eln) and np.array_equal(st, est)
        r = ctx.align(_lib.default_params())
        e = O.align(gs, O.default_params())["aln"]
        assert np.array_equal(r["cols"], e["cols"]) and np.array_equal(r["anchor_start"], e["anchor_start"])
    finally:
        ctx.close()
