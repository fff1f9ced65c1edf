"""Helpers that several GPU test files and their child processes share: sequences of exact lengths, the pair that leaves the band of
S7b, and the comparison of a whole-path result with the oracle's."""
import numpy as np


def seqs(rng, lens, div=0.15):
    """related sequences of exactly these lengths (0: an empty member)"""
    from mauvealigner_amd import synth
    base = rng.integers(0, 4, max(max(lens), 1), dtype=np.uint8)
    out = []
    for L in lens:
        if L == 0:
            out.append(np.zeros(0, np.uint8))
            continue
        x = synth.mutate(base, div, rng, indel_frac=0.3)[:L]
        if len(x) < L:
            x = np.concatenate([x, rng.integers(0, 4, L - len(x), dtype=np.uint8)])
        out.append(x)
    return out


def long_gap_pair(rng, L, shift, div=0.05):
    """Two related sequences whose optimal alignment leaves the band: `shift` extra bases early in b, `shift` bases
    dropped later (the lengths stay close, so the band does not widen with them)."""
    a = rng.integers(0, 4, L, dtype=np.uint8)
    b = a.copy()
    mut = rng.random(L) < div
    b[mut] = (b[mut] + 1) % 4
    b = np.concatenate([b[:L // 6], rng.integers(0, 4, shift, dtype=np.uint8), b[L // 6:L // 2], b[L // 2 + shift:]])
    return [a, b]


def whole_compare(r, e, kind, N, dist=True):
    """a result of the library against the oracle's, everything bit for bit;
    dist: the distance matrix of the guide tree was computed, not given"""
    from oracle import pyoracle as O
    a = e["aln"]
    if kind == "progressive":
        if dist:
            assert np.array_equal(r["dist"], e["dist"])
        assert np.array_equal(r["tree"][0], e["tree"][0]) and np.array_equal(r["tree"][1], e["tree"][1])
    else:
        eml, ems = O.multiplicity_filter(e["mums"][0], e["mums"][1], N)
        assert np.array_equal(r["mum_length"], eml) and np.array_equal(r["mum_start"], ems)
        assert r["n_lcb"] == e["lcbs"]["n_lcb"]
        assert np.array_equal(r["lcb_weight"], e["lcbs"]["weight"])
        for k in ("anchor_length", "anchor_start", "anchor_lcb"):
            assert np.array_equal(r[k], a[k]), k
    assert r["n_iv"] == a["n_iv"]
    for k in ("left", "right", "reverse", "col_off", "cols", "dp_score"):
        assert np.array_equal(r[k], a[k]), k
    assert r["n_gap_dp"] == a["n_gap_dp"] and r["n_dp_cells"] == a["n_dp_cells"]
    assert r["xmfa"] == e["xmfa"]
