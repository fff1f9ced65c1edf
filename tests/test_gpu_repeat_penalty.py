"""Repeat-penalized anchor scores (progressiveMauve --repeat-penalty) on the device against the CPU reference of
tests/repeat_ref.py and the oracle: base multiplicities, penalized match scores, the host chain end to end, the device chain of the
progressive root against the host chain, identity where nothing repeats, and OFF after NEGATIVE."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O
from tests import repeat_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _matrix():
    from mauvealigner_amd import _lib
    return np.array(_lib.default_scoring().matrix, dtype=np.int64)


def repeat_genomes(n, L, seed, copies=12, elem=(300, 1500), div=0.02):
    """n genomes of about L bases from one ancestor that carries `copies` planted copies (half of them reverse-complemented,
    each point-mutated by 3 %) of one repeat element, then mutated per genome at `div`"""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, L).astype(np.uint8)
    e = rng.integers(0, 4, int(rng.integers(*elem))).astype(np.uint8)
    for k, p in enumerate(np.sort(rng.choice(L - len(e), copies, replace=False)).tolist()):
        c = e.copy()
        hit = rng.random(len(c)) < 0.03
        c[hit] = (c[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        anc[p:p + len(c)] = synth.revcomp(c) if k % 2 else c
    return [synth.mutate(anc, div, np.random.default_rng(seed * 100 + g)) for g in range(n)]


def test_multiplicity_matches_reference(ctx):
    """m_g of every base equals the reference: planted forward and reverse-complement copies, the rank-0 w = 15 seed, a solid and
    the coding seed, contigs and ambiguous bases, palindromic windows, copy numbers above 255, a genome shorter than the span"""
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(11)
    gs = repeat_genomes(3, 30000, 5)
    half = rng.integers(0, 4, 6).astype(np.uint8)
    pal = np.concatenate([half, synth.revcomp(half)])           # its own reverse complement: a palindromic 12-base window
    sat = np.concatenate([np.tile(rng.integers(0, 4, 40).astype(np.uint8), 300), rng.integers(0, 4, 3000).astype(np.uint8)])
    for k in range(20):                                          # copies of the palindrome in genome 1
        p = 1000 + 700 * k
        gs[1][p:p + 12] = pal
    gs.append(sat)                                               # 300 tandem copies: counts saturate
    gs.append(rng.integers(0, 4, 9).astype(np.uint8))            # shorter than every span below
    pats = [_lib.get_seed(15, 0), _lib.get_seed(12, _lib.SOLID_SEED), _lib.get_seed(11, _lib.CODING_SEED), _lib.get_seed(9, 0)]
    ctx.set_genomes(gs)
    seen_sat = seen_rep = False
    for pat in pats:
        for g in range(len(gs)):
            got = ctx.seed_multiplicity(g, pat)
            exp = R.multiplicity(gs[g], pat)
            assert got.dtype == np.uint8 and np.array_equal(got, exp), (hex(pat), g, np.flatnonzero(got != exp)[:10])
            seen_sat |= bool((got == 255).any()); seen_rep |= bool(((got > 1) & (got < 255)).any())
    assert seen_sat and seen_rep
    assert (R.window_counts(gs[1], pats[1]) > 0).any()
    # contigs and ambiguous bases: the same genomes with joins and N runs
    cs = [[0, 5000, 12345], [0, 7777], [0], [0, 2999], [0]]
    inv = [None] * len(gs)
    inv[0] = np.zeros(len(gs[0]), bool); inv[0][[100, 101, 20000]] = True; inv[0][25000:25050] = True
    inv[2] = np.zeros(len(gs[2]), bool); inv[2][::997] = True
    ctx.set_genomes(gs, contig_starts=cs, invalid=inv)
    for pat in pats[:3]:
        for g in range(len(gs)):
            got = ctx.seed_multiplicity(g, pat)
            exp = R.multiplicity(gs[g], pat, contig_starts=cs[g], invalid=inv[g])
            assert np.array_equal(got, exp), (hex(pat), g, np.flatnonzero(got != exp)[:10])
    with pytest.raises(RuntimeError):
        ctx.seed_multiplicity(len(gs), pats[0])                  # no such sequence
    with pytest.raises(RuntimeError):
        ctx.set_repeat_penalty(3)                                # unknown mode


def test_penalized_match_scores(ctx):
    """mauve_match_sp_scores_repeat against the reference in both modes: forward and reverse components, absent components;
    mode 0 is mauve_match_sp_scores"""
    gs = repeat_genomes(4, 40000, 7)
    ctx.set_genomes(gs)
    M = _matrix()
    for pat in (O.get_seed(11, 0), O.get_seed(13, 0)):
        ln, st = O.find_matches(gs, pat)
        st = st.copy()
        st[::5, 2] = 0                                           # absent components
        st[1::7, 0] = 0
        assert (st < 0).any()
        mults = [R.multiplicity(g, pat) for g in gs]
        plain = ctx.match_sp_scores(ln, st)
        assert np.array_equal(ctx.match_sp_scores_repeat(pat, 0, ln, st), plain)
        assert np.array_equal(plain, R.sp_scores_repeat(gs, mults, ln, st, R.OFF, M))
        for mode in (R.NEGATIVE, R.ZERO):
            got = ctx.match_sp_scores_repeat(pat, mode, ln, st)
            assert np.array_equal(got, R.sp_scores_repeat(gs, mults, ln, st, mode, M)), mode
            assert (got < plain).any()


def _blocks_and_repeats(seed):
    """two genomes: unique blocks U0..U7 in the same order, an exact 300-base element E between every two; the caller's match
    list pairs U_k with U_k and the copies of E out of order"""
    rng = np.random.default_rng(seed)
    U = [rng.integers(0, 4, 800).astype(np.uint8) for _ in range(8)]
    E = rng.integers(0, 4, 300).astype(np.uint8)
    g0, pos_u, pos_e = [], [], []
    at = 0
    for k in range(8):
        pos_u.append(at); g0.append(U[k]); at += 800
        if k < 7:
            pos_e.append(at); g0.append(E); at += 300
    g0 = np.concatenate(g0)
    g1 = g0.copy()
    for p in pos_u:
        hit = np.flatnonzero(rng.random(800) < 0.01) + p
        g1[hit] = (g1[hit] + 1) & 3
    perm = [3, 0, 5, 1, 6, 2, 4]
    ln, st = [], []
    for p in pos_u:
        ln.append(800); st.append([p + 1, p + 1])
    for j, p in enumerate(pos_e):
        ln.append(300); st.append([p + 1, pos_e[perm[j]] + 1])
    order = np.argsort([s[0] for s in st], kind="stable")
    return [g0, g1], np.array(ln, np.int64)[order], np.array(st, np.int64)[order]


def _partition(ln, st, lcb):
    return sorted(tuple(sorted(map(tuple, st[lcb == k].tolist()))) for k in set(lcb.tolist()) if k >= 0)


@pytest.mark.parametrize("mode", [1, 2])
def test_host_chain_end_to_end(ctx, mode):
    """mauve_align_matches with SP scoring and the penalty: its LCBs are orc_compute_lcbs_w on the reference's penalized weights
    of the overlap-eliminated list, and the whole result is mauve_align_lcbs from that assignment"""
    from mauvealigner_amd import _lib
    gs, ln, st = _blocks_and_repeats(3)
    ctx.set_genomes(gs)
    kw = dict(lcb_scoring=1, seed_weight=11, lcb_weight=10000)
    pat = O.get_seed(11, 0)
    el, es = O.eliminate_overlaps(ln, st)
    mults = [R.multiplicity(g, pat) for g in gs]
    M = _matrix()
    pen = R.compute_lcbs_w(el, es, R.sp_scores_repeat(gs, mults, el, es, mode, M), 10000)
    off = R.compute_lcbs_w(el, es, R.sp_scores_repeat(gs, mults, el, es, R.OFF, M), 10000)
    assert pen["n_lcb"] == 1 and off["n_lcb"] > 1                # the repeat copies hold the blocks apart unless penalized
    ctx.set_repeat_penalty(mode)
    try:
        tab = ctx.align_matches(_lib.default_params(recursive=0, gapped=0, **kw), ln, st)
        assert tab["n_lcb"] == pen["n_lcb"]
        assert _partition(tab["anchor_length"], tab["anchor_start"], tab["anchor_lcb"]) == _partition(el, es, pen["match_lcb"])
        assert np.array_equal(np.sort(tab["lcb_weight"]), np.sort(pen["weight"]))
        whole = ctx.align_matches(_lib.default_params(**kw), ln, st)
        keep = pen["match_lcb"] >= 0
        res = ctx.align_lcbs(_lib.default_params(**kw), el[keep], es[keep], pen["match_lcb"][keep])
        for k in ("anchor_start", "anchor_length", "anchor_lcb", "left", "right", "reverse", "col_off", "cols", "dp_score"):
            assert np.array_equal(res[k], whole[k]), k
        ctx.set_repeat_penalty(0)
        plain = ctx.align_matches(_lib.default_params(recursive=0, gapped=0, **kw), ln, st)
        assert plain["n_lcb"] == off["n_lcb"]
    finally:
        ctx.set_repeat_penalty(0)


def _worker(host_chain, out):
    env = dict(os.environ, MAUVE_CANON_DEVICE_MIN="1", MAUVE_TRACE="1")     # (small lists, too, go down the device route)
    env.pop("MAUVE_HOST_CHAIN", None)
    if host_chain:
        env["MAUVE_HOST_CHAIN"] = "1"
    r = subprocess.run([sys.executable, "-m", "tests.repeat_worker", out], cwd=ROOT, env=env, check=True, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return np.load(out), r.stderr


def test_device_chain_equals_host_chain():
    """progressive_align with the penalty on: the device chain of the root (penalized ch_sp_scores) gives what the host chain
    (penalized sp_score_matches) gives, in two fresh processes"""
    with tempfile.TemporaryDirectory() as td:
        a, ta = _worker(False, os.path.join(td, "dev.npz"))
        b, tb = _worker(True, os.path.join(td, "host.npz"))
        mark = "chain (device): eliminate+nodes+graph"          # (the recursion's batches chain on the device on both routes; the root only on the first)
        assert ta.count(mark) > tb.count(mark)
        assert a["max_mult"] > 1
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k


def test_identity_without_repeats(ctx):
    """where every multiplicity is 1 the penalty changes nothing: progressive and align results with it on equal those with it off
    and the oracle's"""
    from mauvealigner_amd import _lib
    gs = synth.make_config("C4", scale=0.01)[:4]
    ctx.set_genomes(gs)
    kw = dict(lcb_scoring=1, seed_weight=19)
    pat = _lib.get_seed(19, 0)
    for g in range(len(gs)):
        assert (ctx.seed_multiplicity(g, pat) == 1).all()
    keys = ("left", "right", "reverse", "col_off", "cols", "dp_score")
    try:
        for mode in (0, 1, 2):
            ctx.set_repeat_penalty(mode)
            r = ctx.progressive_align(_lib.default_progressive_params(**kw))
            a = ctx.align(_lib.default_params(**kw))
            if mode == 0:
                r0, a0 = r, a
                e = O.progressive_align(gs, O.default_progressive_params(**kw))["aln"]
                f = O.align(gs, O.default_params(**kw))["aln"]
                for k in keys:
                    assert np.array_equal(r[k], e[k]), k
                    assert np.array_equal(a[k], f[k]), k
            for k in keys:
                assert np.array_equal(r[k], r0[k]), (mode, k)
                assert np.array_equal(a[k], a0[k]), (mode, k)
            assert np.array_equal(a["lcb_weight"], a0["lcb_weight"])
    finally:
        ctx.set_repeat_penalty(0)


def test_off_is_off(ctx):
    """NEGATIVE, then OFF on one context: the C4 progressive result at 0.1 scale is the oracle's"""
    from mauvealigner_amd import _lib
    gs = synth.make_config("C4", scale=0.1)
    ctx.set_genomes(gs)
    ctx.set_repeat_penalty(1)
    ctx.progressive_align(_lib.default_progressive_params())
    ctx.set_repeat_penalty(0)
    r = ctx.progressive_align(_lib.default_progressive_params())
    e = O.progressive_align(gs, O.default_progressive_params())["aln"]
    for k in ("left", "right", "reverse", "col_off", "cols", "dp_score"):
        assert np.array_equal(r[k], e[k]), k
