"""The homology pass on the device (hom_seg_count, hom_fn, hom_pred, hom_keep, hom_count / hom_write / hom_offsets and the
host chaining of homology_core) on alignments aimed at its edges -- state changes on 64- and 4096-column boundaries, whole steps and
segments of identity functions, exact ties, column offsets on tile boundaries, 32 genomes, more work items than the grid has waves,
scores at the limits the entry point enforces -- against the oracle and, on the small cases, the table Viterbi of
tests/homology_ref.py as well, so that a mismatch says which of the two C implementations is off.  tests/test_homology_cpu.py shows
from the reference that the cases do what they were built for.  Integer work: everything is compared exactly."""
import functools

import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O
from tests import homology_cases as HC
from tests import homology_ref as HR

pytestmark = pytest.mark.gpu
KEYS = ("seg_iv", "seg_col", "seg_len", "seg_mask", "seg_left", "seg_right", "islands")
CASES = {c["name"]: c for c in HC.small_cases()}
REF_TOO = [n for n in CASES if not n.startswith("wide2")]      # 496 pairs x 8195 columns in Python belong to the CPU suite


@pytest.fixture(scope="module")
def ctx():
    from mauvealigner_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def case_of(name):
    return HC.big_case() if name == "big" else CASES[name]


def fields(scheme):
    return dict(zip(("match", "mismatch", "gap", "go_homologous", "go_unrelated"), HC.SCHEMES[scheme] if isinstance(scheme, str) else scheme))


@functools.lru_cache(maxsize=None)
def oracle(name, scheme):
    off, cols, moved = O.homology_apply(*HC.args(case_of(name)), O.hmm_params(**fields(scheme)))
    off.setflags(write=False); cols.setflags(write=False)
    return off, cols, moved


def same_backbone(b, eb):
    for k in KEYS:
        assert b[k].shape == eb[k].shape and np.array_equal(b[k], eb[k]), k


@pytest.mark.parametrize("name", list(CASES) + ["big"])
def test_device_equals_oracle_and_reference(ctx, name):
    """every generator under every scheme: col_off, cols and n_moved of mauve_apply_homology_alignment are the oracle's, and the
    Python reference's where that is cheap enough to run here"""
    c = case_of(name)
    ctx.set_genomes(c["gs"])
    for scheme in HC.SCHEMES:
        off, cols, moved = ctx.apply_homology_alignment(*HC.args(c)[1:], hmm=ctx.hmm_params(**fields(scheme)))
        eoff, ecols, emoved = oracle(name, scheme)
        if name in REF_TOO:
            roff, rcols, rmoved, _ = HR.homology_ref(*HC.args(c), HC.SCHEMES[scheme])
            dev = moved == rmoved and np.array_equal(off, roff) and np.array_equal(cols, rcols)
            orc = emoved == rmoved and np.array_equal(eoff, roff) and np.array_equal(ecols, rcols)
            assert dev and orc, "%s under %s: device %s, oracle %s the reference" % (name, scheme, "equals" if dev else "DIFFERS FROM", "equals" if orc else "DIFFERS FROM")
        first = int(np.argmax(cols[:len(ecols)] != ecols[:len(cols)])) if len(cols) and len(ecols) else -1
        assert moved == emoved and np.array_equal(off, eoff) and np.array_equal(cols, ecols), (name, scheme, moved, emoved, len(cols), len(ecols), first)


@pytest.mark.parametrize("name", ["mosaic1", "mosaic2", "wide1_N17_L700", "wide2_N32_L8195", "identity1", "tiles1"])
def test_backbone_of_the_rewritten_columns(ctx, name):
    """the backbone (S12) of the columns the device wrote equals the oracle's backbone of the columns the oracle wrote"""
    c = CASES[name]
    ctx.set_genomes(c["gs"])
    for scheme in ("default", "ties1"):
        off, cols, _ = ctx.apply_homology_alignment(*HC.args(c)[1:], hmm=ctx.hmm_params(**fields(scheme)))
        eoff, ecols, _ = oracle(name, scheme)
        same_backbone(ctx.backbone_alignment(c["left"], c["right"], c["reverse"], off, cols),
                      O.backbone(c["left"], c["right"], c["reverse"], eoff, ecols, island_gap=20))


def test_resident_result_rewritten_twice(ctx):
    """mauve_apply_homology on the alignment the context holds, then again on what the first call left there (the columns are the
    result's own from the first call on: swapped buffers, new offsets), then a call that moves nothing: each step equals the
    oracle applied to the oracle's previous step, the backbone afterwards is the oracle's, and the idle call changes no bit"""
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(3)
    anc = rng.integers(0, 4, 30000, dtype=np.uint8)
    gs = [np.ascontiguousarray(synth.mutate(anc, 0.05, rng, indel_frac=0.2)) for _ in range(3)]
    g1 = gs[1].copy(); g1[12000:12600] = rng.integers(0, 4, 600, dtype=np.uint8); gs[1] = g1        # unrelated sequence of the same length
    ctx.set_genomes(gs)
    ctx.align(_lib.default_params(seed_weight=11), fetch=False)
    a = O.align(gs, O.default_params(seed_weight=11))["aln"]
    off, cols = a["col_off"], a["cols"]
    steps = []
    for scheme in ("cheap", "default", (1, 1, 1, 0, 0)):        # the last: every score positive, entering H free -- all of it is homologous
        r = ctx.apply_homology(ctx.hmm_params(**fields(scheme)))
        off, cols, moved = O.homology_apply(gs, a["left"], a["right"], a["reverse"], off, cols, O.hmm_params(**fields(scheme)))
        assert r["n_moved"] == moved and r["n_cols"] == len(cols) and np.array_equal(r["col_off"], off) and np.array_equal(r["cols"], cols), scheme
        assert np.array_equal(r["left"], a["left"]) and np.array_equal(r["right"], a["right"]) and np.array_equal(r["reverse"], a["reverse"])
        steps.append((r, moved))
        if scheme == "default":
            same_backbone(ctx.backbone(island_gap=20), O.backbone(a["left"], a["right"], a["reverse"], off, cols, island_gap=20))
    assert steps[0][1] > 100 and steps[1][1] > 0                 # both rewriting calls rewrote something
    assert steps[2][1] == 0 and np.array_equal(steps[2][0]["cols"], steps[1][0]["cols"]) and np.array_equal(steps[2][0]["col_off"], steps[1][0]["col_off"])
    same_backbone(ctx.backbone(island_gap=20), O.backbone(a["left"], a["right"], a["reverse"], off, cols, island_gap=20))


def test_scores_outside_the_domain_are_refused(ctx):
    """|match|, |mismatch|, |gap| <= 65536 and -2^28 <= transitions <= 0 keep the int32 sums of a segment and the +-2^30 "no bound"
    marks apart: one past any of them is MAUVE_ERR_ARG, the limits themselves are served (and equal the oracle: the limit scheme of
    the parity test above); an alignment of another genome count or with an interval past its genome's end is refused too; and after
    every refusal the context still works"""
    c = CASES["limit_mix8193"]
    ctx.set_genomes(c["gs"])
    tables = HC.args(c)[1:]

    def serves(scheme="limit"):
        off, cols, moved = ctx.apply_homology_alignment(*tables, hmm=ctx.hmm_params(**fields(scheme)))
        eoff, ecols, emoved = oracle("limit_mix8193", scheme)
        assert moved == emoved and np.array_equal(off, eoff) and np.array_equal(cols, ecols)

    serves()
    bad = [dict(match=65537), dict(match=-65537), dict(mismatch=65537), dict(mismatch=-65537), dict(gap=65537), dict(gap=-65537),
           dict(go_homologous=-(1 << 28) - 1), dict(go_unrelated=-(1 << 28) - 1), dict(go_homologous=1), dict(go_unrelated=1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ctx.apply_homology_alignment(*tables, hmm=ctx.hmm_params(**kw))
        serves()
    for kw in (dict(match=65536, mismatch=65536, gap=65536), dict(match=-65536, mismatch=-65536, gap=-65536, go_homologous=-(1 << 28), go_unrelated=0)):
        off, cols, moved = ctx.apply_homology_alignment(*tables, hmm=ctx.hmm_params(**kw))
        eoff, ecols, emoved = O.homology_apply(*HC.args(c), O.hmm_params(**kw))
        assert moved == emoved and np.array_equal(off, eoff) and np.array_equal(cols, ecols), kw
    # another genome count: a third, absent genome in the tables
    left, right, rev, off, cols = tables
    wider = [np.concatenate([t, np.zeros((len(t), 1), t.dtype)], axis=1) for t in (left, right, rev)]
    with pytest.raises(RuntimeError, match="does not belong"):
        ctx.apply_homology_alignment(*wider, off, cols)
    serves()
    # the columns agree with the ends, but the ends lie one base past genome 1
    assert right[-1, 1] == len(c["gs"][1])
    l2, r2 = left.copy(), right.copy()
    l2[-1, 1] += 1; r2[-1, 1] += 1
    with pytest.raises(RuntimeError, match=r"\(-1\).*outside its genome"):
        ctx.apply_homology_alignment(l2, r2, rev, off, cols)
    serves()
