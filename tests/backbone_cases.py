"""Alignments the backbone tests share: tests/test_gpu_backbone.py runs them on the device, tests/test_backbone_host_cpu.py
through the stage's host steps alone; both compare with the oracle."""
import numpy as np

KEYS = ("seg_iv", "seg_col", "seg_len", "seg_mask", "seg_left", "seg_right", "islands")
RANDOM_N = [2, 3, 5, 8, 17, 32]                              # genomes of the six random cases
GAPS = (0, 3, 20, 500)                                       # island_gap values the GPU test runs every random case with (the host test: 20)


def random_alignment(rng, N, n_iv, length, long_runs=False):
    """intervals over random genome subsets: stretches where a random subset is present (the rest gapped), with
    per-column dropouts; lengths chosen so that runs cross the 64-column words and the 4096-column chunks"""
    left, right, rev, col_off, cols = [], [], [], [0], []
    for _ in range(n_iv):
        k = int(rng.integers(1, N + 1))
        S = np.sort(rng.choice(N, k, replace=False))
        full = 0
        for g in S:
            full |= 1 << int(g)
        out = []
        L = int(rng.integers(1, length))
        while len(out) < L:
            kind = rng.random()
            if kind < 0.45:                                   # everybody present, a few dropouts
                n = int(rng.integers(1, 200))
                m = np.full(n, full, np.uint32)
                drop = rng.random(n) < 0.05
                m[drop] &= ~np.uint32(1 << int(rng.choice(S)))
            elif kind < 0.9:                                  # a subset present: short or long run
                n = int(rng.integers(1, 9000 if long_runs and rng.random() < 0.2 else 70))
                sub = 0
                for g in S:
                    if rng.random() < 0.5:
                        sub |= 1 << int(g)
                m = np.full(n, sub, np.uint32)
            else:                                             # alternating single genomes
                n = int(rng.integers(1, 60))
                m = np.array([1 << int(rng.choice(S)) for _ in range(n)], np.uint32)
            out.append(m[m != 0])
        m = np.concatenate(out) if out else np.zeros(0, np.uint32)
        for g in S:                                           # every genome of the interval has a residue
            if not np.any(m >> np.uint32(g) & 1):
                m = np.concatenate([m, np.array([1 << int(g)], np.uint32)])
        lo = np.zeros(N, np.int64)
        hi = np.zeros(N, np.int64)
        rv = np.zeros(N, np.int8)
        for g in S:
            cnt = int(np.count_nonzero(m >> np.uint32(g) & 1))
            lo[g] = int(rng.integers(1, 1 << 20))
            hi[g] = lo[g] + cnt - 1
            rv[g] = int(rng.random() < 0.4)
        left.append(lo)
        right.append(hi)
        rev.append(rv)
        cols.append(m)
        col_off.append(col_off[-1] + len(m))
    return np.array(left), np.array(right), np.array(rev), np.array(col_off, np.int64), np.concatenate(cols)


def random_case(seed):
    """case `seed` of the six: (left, right, reverse, col_off, cols)"""
    rng = np.random.default_rng(1000 + seed)
    return random_alignment(rng, RANDOM_N[seed], n_iv=12, length=[3000, 9000, 20000][seed % 3], long_runs=seed >= 2)


def hand_case():
    """genome 1 lacks five columns the other two share"""
    cols = np.array([7] * 10 + [5] * 5 + [7] * 5, np.uint32)
    return np.array([[1, 101, 201]]), np.array([[20, 115, 220]]), np.array([[0, 0, 1]], np.int8), np.array([0, 20], np.int64), cols
