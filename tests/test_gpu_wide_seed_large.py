"""A genome set past 2^31 bases: the seed pass switches to 64-bit window indices by itself and equals the oracle
on the small cores the set is built from.  The oracle cannot hold 2^31 bases, so the set is built to have an exact small answer:

    genome 0 = core0 | sep | padA,   genome 1 = core1 | sep | padB,   genome 2 = core2

Cores come first (their coordinates are those of the cores alone); padA and padB are ~1.1 Gbp each, so core2's windows start past
2^31 in the global window index.  A pad repeats a random 64-base unit (a different one per genome): every pad mer occurs millions of
times in its own genome, so no pad window can seed under any finder rule.  sep is a run of ambiguous bases (bitmap): no window and no
extension runs from a core into a pad.  The alignment path is not verified at this size and refuses such a set."""
import numpy as np
import pytest

from mauvealigner_amd import synth
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

PAD_UNITS = 17_200_000                   # 64-base units per pad: 1.1008 Gbp
PATTERNS = [O.get_seed(15, 0), O.get_seed(19, 0)]      # a w <= 15 (32-bit keys) and a w >= 17 (64-bit keys) pattern


def _need_bytes(total, nseq):
    # seed pass, wide, 64-bit keys: 38.25 + 4N bytes per window, plus the packed genomes and both bitmaps on the device
    return int(total * (38.25 + 4 * nseq) + total * 0.5) + (4 << 30)


def _pack_genome(lib, head, unit, n_units):
    """head (length a multiple of 32) followed by n_units copies of the 64-base unit, in the boundary's 2-bit packing, without a
    byte-per-base array of the whole genome"""
    assert len(head) % 32 == 0 and len(unit) == 64
    L = len(head) + 64 * n_units
    out = np.zeros(lib.load().mauve_packed_words(L), np.uint64)
    hw = len(head) // 32
    out[:hw] = lib.pack_codes(head)[:hw]
    out[hw:hw + 2 * n_units].reshape(-1, 2)[:] = lib.pack_codes(unit)[:2]
    return out, L


def _units_clear_of_cores(cores, rng):
    """two pad units none of whose canonical mers (windows across the unit's end included) is a canonical core mer, for every pattern"""
    core_mers = [set(np.concatenate([O.mers(c, p)[0] for c in cores]).tolist()) for p in PATTERNS]
    units = []
    while len(units) < 2:
        u = rng.integers(0, 4, 64, dtype=np.uint8)
        wrap = np.tile(u, 3)
        if all(not (set(O.mers(wrap, p)[0].tolist()) & cm) for p, cm in zip(PATTERNS, core_mers)):
            units.append(u)
    for u in units:                      # the assertion the construction rests on
        for p, cm in zip(PATTERNS, core_mers):
            assert not (set(O.mers(np.tile(u, 3), p)[0].tolist()) & cm)
    return units


def test_seed_pass_past_2g_windows():
    import torch
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(2031)
    anc = rng.integers(0, 4, 40000, dtype=np.uint8)
    core0 = synth.mutate(anc, 0.02, rng)
    core1 = synth.mutate(anc, 0.02, rng)
    core2 = synth.mutate(anc, 0.03, rng)
    core2 = np.concatenate([core2[:9000], synth.revcomp(core2[9000:15000]), core2[15000:]])     # an inversion: reverse-strand matches
    core1[20000:20400] = core1[30000:30400]                                                       # a repeat in genome 1: the finder rules differ
    cores = [core0, core1, core2]
    unitA, unitB = _units_clear_of_cores(cores, rng)
    genomes, lens, bits = [], [], []
    for core, unit in ((core0, unitA), (core1, unitB)):
        sep = 64 + (-len(core)) % 32
        head = np.concatenate([core, np.zeros(sep, np.uint8)])
        w, L = _pack_genome(_lib, head, unit, PAD_UNITS)
        b = np.zeros(L // 64 + 1, np.uint64)
        for i in range(len(core), len(core) + sep):
            b[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        genomes.append(w); lens.append(L); bits.append(b)
    genomes.append(_lib.pack_codes(core2)); lens.append(len(core2)); bits.append(None)
    total = sum(lens)
    span = max(O.seed_length(p) for p in PATTERNS)
    assert lens[0] + lens[1] - 2 * (span - 1) > 1 << 31 and total < _lib.MAX_TOTAL_LEN     # core2's windows lie past 2^31
    free, _ = torch.cuda.mem_get_info(0)
    need = _need_bytes(total, 3)
    if free < need:
        pytest.skip("needs %.1f GB of free device memory for a %.2f Gbp seed pass, %.1f GB free" % (need / 1e9, total / 1e9, free / 1e9))
    ctx = _lib.Context(0)
    try:
        ctx.set_genomes_packed(genomes, lens, invalid_bits=bits)
        del genomes
        for pat in PATTERNS:
            for mode, mask in ((O.MODE_MEM, 0), (O.MODE_MEM, 7), (O.MODE_UNIQUE, 0), (O.MODE_PAIRWISE, 0)):
                for ext in (False, True):
                    ln, st = ctx.seed_mums(pat, mode=mode, mask=mask, extend=ext)
                    eln, est = O.find_matches(cores, pat, mode=mode, mask=mask, extend=ext)
                    assert len(eln) > 10, (pat, mode, mask, ext)
                    assert np.array_equal(ln, eln) and np.array_equal(st, est), (pat, mode, mask, ext)
                    print("seed pass past 2^31: w=%d mode=%d mask=%d extend=%d: %d matches equal the oracle" % (O.seed_weight(pat), mode, mask, ext, len(ln)), flush=True)
                    if mode != O.MODE_PAIRWISE:
                        assert np.count_nonzero(st[:, 2]) > 0                                     # genome 2 (past 2^31) takes part
            mer, pos = ctx.sorted_mer_list(2, pat)
            emer, epos = O.sorted_mer_list(core2, pat)
            assert np.array_equal(mer, emer) and np.array_equal(pos, epos), pat
            m, o, s = ctx.seed_match_enumerate(2, pat, 2, 1000, False)
            em, eo, es = O.seed_match_enumerate(core2, pat, 2, 1000, False)
            assert np.array_equal(m, em) and np.array_equal(o, eo) and np.array_equal(s, es), pat
            assert np.array_equal(ctx.seed_multiplicity(2, pat), O.seed_multiplicity(core2, pat)), pat
        # the alignment path is not verified at this size: refused, and the context stays usable
        with pytest.raises(RuntimeError, match=r"\(-4\).*2\^31 bases"):
            ctx.align(_lib.default_params(seed_weight=15))
        with pytest.raises(RuntimeError, match=r"\(-4\).*2\^31 bases"):
            ctx.progressive_align(_lib.default_params(seed_weight=15))
        small = synth.make_config("C3", scale=0.01)
        ctx.set_genomes(small)
        r = ctx.align(_lib.default_params())
        e = O.align(small, O.default_params())["aln"]
        assert np.array_equal(r["cols"], e["cols"]) and np.array_equal(r["anchor_start"], e["anchor_start"])
    finally:
        ctx.close()


def test_packed_upload_with_bitmaps_equals_per_base_upload():
    """set_genomes_packed(contig_starts=, invalid_bits=) -- packed genomes with packed ambiguity bitmaps -- gives the matches of
    set_genomes(..., invalid=) with the same genomes as per-base arrays"""
    from mauvealigner_amd import _lib
    rng = np.random.default_rng(7)
    anc = rng.integers(0, 4, 20000, dtype=np.uint8)
    gs = [synth.mutate(anc, 0.02, rng) for _ in range(3)]
    contigs = [[0, 5000, 12000], [0], [0, 9000]]
    invalid = [np.zeros(len(g), bool) for g in gs]
    invalid[0][7000:7100] = True
    invalid[2][15000:15040] = True
    for g in range(3):
        gs[g] = gs[g].copy(); gs[g][invalid[g]] = 0
    bits = []
    for g in range(3):
        b = np.zeros((len(gs[g]) // 64 + 1) * 64, np.uint8)
        b[:len(gs[g])] = invalid[g]
        bits.append(np.packbits(b, bitorder="little").view(np.uint64).copy() if invalid[g].any() else None)
    ctx = _lib.Context(0)
    try:
        for pat, mode in ((O.get_seed(11, 0), O.MODE_MEM), (O.get_seed(15, 0), O.MODE_UNIQUE)):
            ctx.set_genomes(gs, contig_starts=contigs, invalid=invalid)
            a = ctx.seed_mums(pat, mode=mode)
            ctx.set_genomes_packed([_lib.pack_codes(g) for g in gs], [len(g) for g in gs], contig_starts=contigs, invalid_bits=bits)
            b = ctx.seed_mums(pat, mode=mode)
            assert len(a[0]) > 20 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        with pytest.raises(ValueError):
            ctx.set_genomes_packed([_lib.pack_codes(g) for g in gs], [len(g) for g in gs], contig_starts=contigs[:2])
        with pytest.raises(ValueError):
            ctx.set_genomes_packed([_lib.pack_codes(g) for g in gs], [len(g) for g in gs], invalid_bits=[bits[0][:10], None, None])
    finally:
        ctx.close()
