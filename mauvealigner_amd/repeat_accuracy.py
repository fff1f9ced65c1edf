"""Planted repeats with their truth: the input of the repeat-map score (Context.repeat_score), the counterpart for one
genome of what synth.star_genomes(track=True) and accuracy.truth_alignment are for a genome set.

A family is one random element copied m times into random background, every copy mutated on its own through synth.mutate(..., origin=...)
and some of them reverse-complemented.  The truth is one interval per family whose rows are the copy slots: row c of interval f is copy c
of family f, present iff c < m, reverse iff the copy was reverse-complemented (S14's rule: the k-th residue of a reverse row lies at
right - k).  The rows carry genome coordinates, so row_offset is zeros.  Two bases of two copies share a column iff they descend from the
same base of the element (accuracy._truth_columns).  Everything is deterministic from seed_key."""
import numpy as np

from . import accuracy, synth


def planted_repeats(length, families, seed_key):
    """families: list of (element_length, copies, mutation_rate), 2 <= copies <= 32.  -> (genome codes uint8 [length], truth) with truth =
    dict(left, right, reverse [n_families, max copies], col_off, cols) as Context.score_truth takes it, plus `place`: per family the
    0-based start of every copy"""
    if not families or any(m < 2 or m > 32 or el < 1 for el, m, _ in families):
        raise ValueError("planted_repeats: families = [(element_length, copies in 2 .. 32, rate), ...]")
    copies, origins, revs = [], [], []
    for f, (el, m, rate) in enumerate(families):
        element = synth.random_genome(el, synth._rng(seed_key, 1 + f, 0))
        flip = synth._rng(seed_key, 1 + f, 1).random(m) < 0.4
        flip[0] = False
        if m > 1 and not flip.any():
            flip[m - 1] = True                                   # every family has a reversed copy
        for c in range(m):
            x, o = synth.mutate(element, rate, synth._rng(seed_key, 1 + f, 2 + c), origin=np.arange(1, el + 1, dtype=np.int64))
            copies.append((f, c, x))
            origins.append(o)
            revs.append(bool(flip[c]))
    total = sum(len(x) for _, _, x in copies)
    K = len(copies)
    free = int(length) - total
    if free < K + 1:
        raise ValueError("planted_repeats: the copies (%d bases) do not fit into %d bases with background between them" % (total, length))
    rng = synth._rng(seed_key, 0)
    genome = synth.random_genome(length, rng)
    cuts = np.sort(rng.integers(1, free - K + 1, size=K + 1))   # background in front of every copy, at least one base each
    gaps = np.diff(np.concatenate([[0], cuts]))[:K] + 1
    order = np.argsort(rng.random(K), kind="stable")
    place = [0] * K
    at = 0
    for slot, k in enumerate(order.tolist()):
        at += int(gaps[slot])
        place[k] = at
        x = copies[k][2]
        genome[at:at + len(x)] = synth.revcomp(x) if revs[k] else x
        at += len(x)
    assert at <= length
    nrow = max(m for _, m, _ in families)
    F = len(families)
    left, right, rev = np.zeros((F, nrow), np.int64), np.zeros((F, nrow), np.int64), np.zeros((F, nrow), np.int8)
    col_off, cols, places = [0], [], []
    k0 = 0
    for f, (el, m, rate) in enumerate(families):
        allk, col, ncol = accuracy._truth_columns(origins[k0:k0 + m], "planted_repeats")
        c = np.zeros(ncol, np.uint32)
        np.bitwise_or.at(c, col, np.uint32(1) << allk[:, 3].astype(np.uint32))
        cols.append(c)
        col_off.append(col_off[-1] + ncol)
        for r in range(m):
            ln = len(copies[k0 + r][2])
            if ln:
                left[f, r], right[f, r], rev[f, r] = place[k0 + r] + 1, place[k0 + r] + ln, int(revs[k0 + r])
        places.append(place[k0:k0 + m])
        k0 += m
    truth = dict(left=left, right=right, reverse=rev, col_off=np.array(col_off, np.int64), cols=np.concatenate(cols), place=places)
    return genome, truth
