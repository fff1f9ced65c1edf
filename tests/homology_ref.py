"""The homology pass once more, written from that text alone: plain Python integers, both Viterbi values of every
pair-column, a predecessor table, the walk back, then the split.  No clamp form, no scan, no segments -- what the device's segment
scan (csrc/homology_dev.hip) and the oracle's loop (orc_homology_apply) are both compared with.

numpy only looks up the base of every (column, genome) and the emission score of every pair-column; the recurrence runs on Python
ints, which do not overflow, so the score limits of the device (|score| <= 65536, transitions >= -2^28) mean nothing here."""
import collections

import numpy as np

Scheme = collections.namedtuple("Scheme", "match mismatch gap go_homologous go_unrelated")
NEG = -(1 << 200)                                   # "no path ends here": below every sum of scores this module can form


def as_scheme(h):
    """a Scheme from a tuple or from anything with the five fields (the ctypes structs of the library and the oracle)"""
    if isinstance(h, tuple):
        return Scheme(*[int(v) for v in h])
    return Scheme(int(h.match), int(h.mismatch), int(h.gap), int(h.go_homologous), int(h.go_unrelated))


def strand_bases(gs, left, right, reverse, iv, g, present):
    """bases of genome g in the columns `present` marks, read on the interval's strand (complemented on the reverse strand)"""
    k = np.cumsum(present) - present                                  # ordinal of the residue in column order
    l, r = int(left[iv][g]), int(right[iv][g])
    pos = (r - k) if reverse[iv][g] else (l + k)                      # 1-based position
    pos = np.where(present, pos, 1)
    x = np.asarray(gs[g])[pos - 1].astype(np.int64) & 3
    return 3 - x if reverse[iv][g] else x


def pair_path(scores, h):
    """Viterbi path of one pair over its pair-columns (emission scores as Python ints) -> (list of states, 1 = H; final v_H, v_U).
    The path starts in U; ties prefer staying; H wins a tie at the end."""
    vh, vu = NEG, 0
    goh, gou = h.go_homologous, h.go_unrelated
    from_h_h, from_u_u = [], []                                       # predecessor table: did H come from H, did U come from U
    for s in scores:
        enter_h, enter_u = vu + goh, vh + gou
        if vh >= enter_h:
            from_h_h.append(True); nh = vh + s
        else:
            from_h_h.append(False); nh = enter_h + s
        if vu >= enter_u:
            from_u_u.append(True); nu = vu
        else:
            from_u_u.append(False); nu = enter_u
        vh, vu = nh, nu
    st = 1 if vh >= vu else 0
    states = [0] * len(scores)
    for c in range(len(scores) - 1, -1, -1):
        states[c] = st
        st = (1 if from_h_h[c] else 0) if st else (0 if from_u_u[c] else 1)
    return states, vh, vu


def homology_ref(gs, left, right, reverse, col_off, cols, hmm, detail=None):
    """-> (col_off, cols, n_moved, flips).  flips[(interval, a, b)] lists (interval column, new state) wherever the state of the pair
    differs from its state at the previous pair-column (1 = into H, 0 = out of H; the first pair-column has no previous one).
    `detail`, a dict, receives 'keep': per interval the mask of the genomes that stay in every column, and 'final': per (interval, a, b)
    the two Viterbi values behind the last pair-column."""
    h = as_scheme(hmm)
    N = len(gs)
    cols = np.asarray(cols, np.uint32)
    out_cols, out_off, moved, flips = [], [0], 0, {}
    keeps, finals = [], {}
    for iv in range(len(left)):
        cs = cols[int(col_off[iv]):int(col_off[iv + 1])].astype(np.int64)
        present = [int(left[iv][g]) != 0 for g in range(N)]
        has = {g: (cs >> g & 1).astype(bool) for g in range(N) if present[g]}
        base = {g: strand_bases(gs, left, right, reverse, iv, g, has[g]) for g in has}
        keep = [0] * len(cs)
        for a in range(N):
            for b in range(a + 1, N):
                if not (present[a] and present[b]):
                    continue
                either, both = has[a] | has[b], has[a] & has[b]
                where = np.flatnonzero(either)                        # the pair-columns: columns neither genome has are skipped
                if not len(where):
                    continue
                sc = np.where(both, np.where(base[a] == base[b], h.match, h.mismatch), h.gap)[where]
                states, vh, vu = pair_path([int(v) for v in sc], h)
                finals[(iv, a, b)] = (vh, vu)
                fl = []
                bit = 1 << a | 1 << b
                wl, bl = where.tolist(), both[where].tolist()
                for k, c in enumerate(wl):
                    if k and states[k] != states[k - 1]:
                        fl.append((c, states[k]))
                    if states[k] and bl[k]:
                        keep[c] |= bit
                flips[(iv, a, b)] = fl
        for c, m in enumerate(cs.tolist()):
            k = keep[c] & m
            if k:
                out_cols.append(k)
            rest = m & ~k
            g = 0
            while rest:
                if rest & 1:
                    out_cols.append(1 << g)
                    moved += 1 if m & (m - 1) else 0                  # a residue alone in its column was not aligned to begin with
                rest >>= 1; g += 1
        out_off.append(len(out_cols))
        keeps.append(keep)
    if detail is not None:
        detail["keep"] = keeps
        detail["final"] = finals
    return np.array(out_off, np.int64), np.array(out_cols, np.uint32), moved, flips
