"""Repeat-penalized anchor scores (progressiveMauve --repeat-penalty) on the device against the CPU reference of
tests/repeat_ref.py and the oracle's restatement of S11d: base multiplicities (32- and 64-bit keys, spans up to 49, 16 genomes, tile
edges), the multiplicity cache, penalized match scores, align / progressive_align / the split phase end to end, the three chain
routes, the refusal of SP scoring above 16 genomes, identity where nothing repeats, OFF after NEGATIVE, and the golden fixture."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O
from tests import repeat_ref as R
from tests.repeat_ref import _blocks_and_repeats, repeat_genomes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALN_KEYS = ("left", "right", "reverse", "col_off", "cols", "dp_score")
ANCHOR_KEYS = ("anchor_start", "anchor_length", "anchor_lcb")


def _differs(a, b):
    """the penalty matters: two oracle alignments differ somewhere"""
    return not all(np.array_equal(a[k], b[k]) for k in ALN_KEYS)


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _matrix():
    from mauvealigner_amd import _lib
    return np.array(_lib.default_scoring().matrix, dtype=np.int64)


def _tile_genomes(n, span, seed):
    """n genomes of 4096 k + delta bases (delta cycling over -span, -1, 0, 1, 3, span - 1), each with copies of one element (some
    reverse-complemented) across every 4096 boundary, one ending on it and one starting on it"""
    rng = np.random.default_rng(seed)
    e = rng.integers(0, 4, 2 * span + 37).astype(np.uint8)
    out = []
    for i in range(n):
        L = 4096 * (1 + i % 3) + [-span, -1, 0, 1, 3, span - 1][i % 6]
        g = rng.integers(0, 4, L).astype(np.uint8)
        for k, b in enumerate(range(4096, L, 4096)):
            for p in (b - len(e) // 2 - k, b - len(e), b):
                if 0 <= p and p + len(e) <= L:
                    g[p:p + len(e)] = synth.revcomp(e) if (p + k) % 2 else e
        g[10:10 + len(e)] = e
        out.append(g)
    return out


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
    # 32-bit keys through the weight > 15 extract branch (w = 16), 64-bit keys (w = 17, 19, 21), the span-49 seed; 9 and 16 genomes
    # (genome_of's loop past 8 in rp_count) of 4096 k + delta bases, repeat copies across the 4096-position tiles of rp_span_min
    wide = [_lib.get_seed(16, 0), _lib.get_seed(17, 0), _lib.get_seed(19, 0), _lib.get_seed(21, 1), _lib.get_seed(31, 2)]
    assert O.seed_length(wide[-1]) == 49                         # MAUVE_MAX_SEED_SPAN
    for pat in wide:
        span = O.seed_length(pat)
        for n in (9, 16):
            tg = _tile_genomes(n, span, n * 100 + span)
            ctx.set_genomes(tg)
            seen_rep = False
            for g in range(n):
                got = ctx.seed_multiplicity(g, pat)
                exp = R.multiplicity(tg[g], pat)
                assert np.array_equal(got, exp), (hex(pat), n, g, len(tg[g]), np.flatnonzero(got != exp)[:10])
                seen_rep |= bool((got > 1).any())
            assert seen_rep
    ctx.set_genomes(gs)
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


def _worker(route, out):
    env = dict(os.environ, MAUVE_TRACE="1")
    env.pop("MAUVE_HOST_CHAIN", None)
    env.pop("MAUVE_CANON_DEVICE_MIN", None)
    if route in ("device", "host"):
        env["MAUVE_CANON_DEVICE_MIN"] = "1"                                 # (small lists, too, go down the device route)
    if route == "host":
        env["MAUVE_HOST_CHAIN"] = "1"
    r = subprocess.run([sys.executable, "-m", "tests.repeat_worker", out], cwd=ROOT, env=env, check=True, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return np.load(out), r.stderr


def test_device_chain_equals_host_chain():
    """progressive_align with the penalty on, in three fresh processes: the default route, the device chain of the root (penalized
    ch_sp_scores, MAUVE_CANON_DEVICE_MIN=1) and the host chain (penalized sp_score_matches, MAUVE_HOST_CHAIN=1) each give the
    oracle's result, which the penalty changes"""
    from tests.repeat_worker import worker_genomes
    with tempfile.TemporaryDirectory() as td:
        runs = {route: _worker(route, os.path.join(td, route + ".npz")) for route in ("default", "device", "host")}
    mark = "chain (device): eliminate+nodes+graph"          # (the recursion's batches chain on the device on both routes; the root only on the first)
    assert runs["device"][1].count(mark) > runs["host"][1].count(mark)
    gs = worker_genomes()
    off = O.progressive_align(gs, O.default_progressive_params())["aln"]
    for mode in (1, 2):
        e = O.progressive_align(gs, O.default_progressive_params(), repeat_penalty=mode)["aln"]
        assert _differs(e, off), mode
        for route, (a, _) in runs.items():
            assert a["max_mult"] > 1
            for k in ALN_KEYS:
                assert np.array_equal(a["m%d_%s" % (mode, k)], e[k]), (route, mode, k)
            assert int(a["m%d_n_gap_dp" % mode]) == e["n_gap_dp"], (route, mode)


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


def _penalty_genomes(name):
    """the genome sets of the end-to-end comparisons: 5 and 8 genomes with a planted family (the penalty changes every call on
    them), and C4 at 0.05 with a family appended as tests/repeat_worker.py builds it"""
    if name == "g5":
        return repeat_genomes(5, 12000, 9, copies=24, elem=(300, 800))
    if name == "g8":
        return repeat_genomes(8, 10000, 5, copies=16, elem=(300, 800))
    from tests.repeat_worker import worker_genomes
    return worker_genomes(scale=0.05)


def _random_tree(N, seed):
    """a random guide tree in the table form (leaves 0..N-1, internal nodes in merge order, left child = lower id)"""
    rng = np.random.default_rng(seed)
    act, left, right = list(range(N)), [-1] * N, [-1] * N
    while len(act) > 1:
        i, j = sorted(rng.choice(len(act), 2, replace=False).tolist())
        a, b = act[i], act[j]
        left.append(min(a, b)); right.append(max(a, b))
        act = [x for k, x in enumerate(act) if k not in (i, j)] + [len(left) - 1]
    return np.array(left, np.int32), np.array(right, np.int32)


def _same(r, e, keys, what):
    for k in keys:
        assert np.array_equal(r[k], e[k]), (what, k)
    assert r["n_gap_dp"] == e["n_gap_dp"], (what, "n_gap_dp")


@pytest.mark.parametrize("name", ["g5", "g8", "c4fam"])
def test_penalized_alignments_equal_oracle(ctx, name):
    """NEGATIVE and ZERO, bit-exact against the oracle's restatement of S11d: align with SP scoring (anchors and LCB weights
    included), progressive_align at the call site's defaults (weight and breakpoint scaling, refinement), along a random tree, with
    seed families and without refinement; on every case the oracle's penalized result differs from its OFF result"""
    from mauvealigner_amd import _lib
    gs = _penalty_genomes(name)
    N = len(gs)
    ctx.set_genomes(gs)
    tree = _random_tree(N, 3)
    cases = [("progressive", {}, None), ("tree", {}, tree), ("family", dict(seed_family=1), None), ("no refinement", dict(refine_rounds=0), None)]
    if name != "c4fam":                                       # (C4's own search gives no LCB that the penalty moves under ZERO)
        cases.insert(0, ("align", dict(lcb_scoring=1), None))
    try:
        for what, kw, t in cases:
            if what == "align":
                off = O.align(gs, O.default_params(**kw))["aln"]
            else:
                off = O.progressive_align(gs, O.default_progressive_params(**kw), tree=t)["aln"]
            for mode in (R.NEGATIVE, R.ZERO):
                ctx.set_repeat_penalty(mode)
                if what == "align":
                    e = O.align(gs, O.default_params(**kw), repeat_penalty=mode)
                    r = ctx.align(_lib.default_params(**kw))
                    _same(r, e["aln"], ALN_KEYS + ANCHOR_KEYS, (what, mode))
                    assert np.array_equal(r["lcb_weight"], e["lcbs"]["weight"]), (what, mode)
                    e = e["aln"]
                else:
                    e = O.progressive_align(gs, O.default_progressive_params(**kw), tree=t, repeat_penalty=mode)["aln"]
                    r = ctx.progressive_align(_lib.default_progressive_params(**kw), tree=t)
                    _same(r, e, ALN_KEYS, (what, mode))
                assert _differs(e, off), (what, mode)
    finally:
        ctx.set_repeat_penalty(0)


def test_split_phase_equals_align(ctx):
    """align_begin / align_dp / align_finish with the penalty on give what align gives, and that is the oracle's"""
    from mauvealigner_amd import _lib
    gs = _penalty_genomes("g5")
    ctx.set_genomes(gs)
    p = _lib.default_params(lcb_scoring=1)
    try:
        for mode in (R.NEGATIVE, R.ZERO):
            ctx.set_repeat_penalty(mode)
            whole = ctx.align(p)
            n_dp, cost, cap = ctx.align_begin(p)
            assert n_dp == whole["n_gap_dp"]
            idx = np.arange(n_dp, dtype=np.int64)
            cols, score, cells = ctx.align_dp(idx, cap)
            two = ctx.align_finish([cols[i].copy() for i in range(n_dp)], score[:n_dp], cells)
            for k in ALN_KEYS + ANCHOR_KEYS + ("lcb_weight",):
                assert np.array_equal(two[k], whole[k]), (mode, k)
            e = O.align(gs, O.default_params(lcb_scoring=1), repeat_penalty=mode)["aln"]
            _same(two, e, ALN_KEYS + ANCHOR_KEYS, mode)
    finally:
        ctx.set_repeat_penalty(0)


def test_multiplicity_cache_follows_genomes_and_pattern(ctx):
    """one context: a penalized align on genomes A, then on genomes B of the same lengths with other repeats, then with another
    seed weight on B -- each equals the oracle (the multiplicities are cached by genome generation and pattern)"""
    from mauvealigner_amd import _lib
    A = _penalty_genomes("g5")
    rng = np.random.default_rng(77)
    B = [np.concatenate([b, rng.integers(0, 4, max(0, len(a) - len(b))).astype(np.uint8)])[:len(a)]
         for a, b in zip(A, repeat_genomes(5, 12000, 10, copies=24, elem=(300, 800)))]
    assert [len(a) for a in A] == [len(b) for b in B]
    assert not np.array_equal(R.multiplicity(A[0], O.get_seed(11, 0)), R.multiplicity(B[0], O.get_seed(11, 0)))
    try:
        ctx.set_repeat_penalty(R.NEGATIVE)
        for gs, w, fresh in ((A, 11, True), (B, 11, True), (B, 12, False)):
            if fresh:
                ctx.set_genomes(gs)
            kw = dict(lcb_scoring=1, seed_weight=w)
            r = ctx.align(_lib.default_params(**kw))
            e = O.align(gs, O.default_params(**kw), repeat_penalty=R.NEGATIVE)["aln"]
            _same(r, e, ALN_KEYS + ANCHOR_KEYS, w)
            assert _differs(e, O.align(gs, O.default_params(**kw))["aln"]), w
    finally:
        ctx.set_repeat_penalty(0)


@pytest.mark.parametrize("n,seed,div", [(20, 49, 0.02), (32, 52, 0.005)])
def test_many_genomes_sp_scoring_is_refused(ctx, n, seed, div):
    """above 16 genomes sum-of-pairs scoring is refused (MAUVE_ERR_LIMIT, by sp_score_matches as by the device chain), whatever the
    mode: the penalty opens no route of its own there.  The oracle scores such sets, and the penalty changes its result; the context
    stays usable, and the next penalized call on 5 genomes is the oracle's"""
    from mauvealigner_amd import _lib
    gs = repeat_genomes(n, 4000, seed, copies=16, elem=(200, 500), div=div)
    e = O.align(gs, O.default_params(lcb_scoring=1), repeat_penalty=R.NEGATIVE)
    assert _differs(e["aln"], O.align(gs, O.default_params(lcb_scoring=1))["aln"])
    ctx.set_genomes(gs)
    try:
        for mode in (R.OFF, R.NEGATIVE, R.ZERO):
            ctx.set_repeat_penalty(mode)
            with pytest.raises(RuntimeError, match="at most 16 genomes"):
                ctx.align(_lib.default_params(lcb_scoring=1))
        small = _penalty_genomes("g5")
        ctx.set_genomes(small)
        ctx.set_repeat_penalty(R.NEGATIVE)
        r = ctx.align(_lib.default_params(lcb_scoring=1))
    finally:
        ctx.set_repeat_penalty(0)
    _same(r, O.align(small, O.default_params(lcb_scoring=1), repeat_penalty=R.NEGATIVE)["aln"], ALN_KEYS + ANCHOR_KEYS, n)


def test_golden_repeat_fixture(ctx):
    """the penalized progressive fixture (tests/golden/g4x6k_repeat, NEGATIVE, default progressive parameters) through the C-ABI"""
    from mauvealigner_amd import _lib
    z = np.load(os.path.join(ROOT, "tests", "golden", "g4x6k_repeat.npz"))
    N = int(z["nseq"])
    gs = [z["genome%d" % g] for g in range(N)]
    ctx.set_genomes(gs)
    try:
        ctx.set_repeat_penalty(int(z["repeat_penalty"]))
        r = ctx.progressive_align(_lib.default_progressive_params(), names=["g%d" % g for g in range(N)], want_xmfa=True)
    finally:
        ctx.set_repeat_penalty(0)
    assert np.array_equal(r["tree"][0], z["tree_left"]) and np.array_equal(r["tree"][1], z["tree_right"])
    for k in ALN_KEYS:
        assert np.array_equal(r[k], z[k]), k
    with open(os.path.join(ROOT, "tests", "golden", "g4x6k_repeat.xmfa")) as f:
        assert f.read() == r["xmfa"]
