"""numpy restatement of the projection onto a genome subset: the expected value of every device answer in
tests/test_gpu_project.py, pinned itself in tests/test_project_cpu.py.  It works on the arrays of mauve_align_fetch, shares no code with
the product, and takes its collinearity labels from the oracle's LCB chain (O.compute_lcbs(..., 0, False)) on records of length 1 at the
signed left ends.

Rules: (1) an interval is kept iff every genome of proj is present; (2) one whose row proj[0] is reversed is flipped (columns descending,
strands of the projected rows toggled); (3) the kept intervals by left end in proj[0], consecutive ones with one label form an output
interval; (4) between two pieces every projected genome, in proj order, gets its bases strictly between them as filler columns of its bit
alone; (5) wide columns restricted to proj, the empty ones dropped on request; (6) provenance."""
import numpy as np

from oracle import pyoracle as O


def project(a, proj, drop_empty=True, compact=False):
    left, right = np.asarray(a["left"], np.int64), np.asarray(a["right"], np.int64)
    rev = np.asarray(a["reverse"]) != 0
    col_off, cols = np.asarray(a["col_off"], np.int64), np.asarray(a["cols"], np.uint32)
    n_iv, N = left.shape
    proj = [int(g) for g in proj]
    assert 1 <= len(proj) <= N and len(set(proj)) == len(proj) and all(0 <= g < N for g in proj)
    pmask = np.uint32(sum(1 << g for g in proj))
    kept = np.flatnonzero(np.all(left[:, proj] != 0, axis=1)) if n_iv else np.zeros(0, np.int64)
    kept = kept[np.argsort(left[kept, proj[0]], kind="stable")]
    flip = rev[kept, proj[0]]
    prev = rev[kept][:, proj] ^ flip[:, None]                                        # strands after normalisation, proj order
    K = len(kept)
    if K:
        start = np.where(prev, -left[kept][:, proj], left[kept][:, proj])
        label = O.compute_lcbs(np.ones(K, np.int64), start, 0, False)["match_lcb"]
    else:
        label = np.zeros(0, np.int64)
    o_left, o_right, o_rev, o_off, parts, srcs, s_off, s_iv, s_flip = [], [], [], [0], [], [], [0], [], []
    n_cols = n_fill = 0
    for q in range(K):
        i = int(kept[q])
        if q == 0 or label[q] != label[q - 1]:
            if q:
                o_off.append(n_cols)
                s_off.append(len(s_iv))
            l, r, v = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int8)
            l[proj], r[proj], v[proj] = left[i, proj], right[i, proj], prev[q]
            o_left.append(l), o_right.append(r), o_rev.append(v)
        else:
            p = int(kept[q - 1])
            for k, g in enumerate(proj):
                assert prev[q, k] == prev[q - 1, k]
                d = int(left[p, g] - right[i, g] - 1 if prev[q, k] else left[i, g] - right[p, g] - 1)
                assert d >= 0
                parts.append(np.full(d, 1 << g, np.uint32))
                srcs.append(np.full(d, -1, np.int64))
                n_cols += d
                n_fill += d
                o_left[-1][g] = min(o_left[-1][g], left[i, g])
                o_right[-1][g] = max(o_right[-1][g], right[i, g])
        x = np.arange(col_off[i], col_off[i + 1], dtype=np.int64)
        if flip[q]:
            x = x[::-1]
        m = cols[x] & pmask
        if drop_empty:
            x, m = x[m != 0], m[m != 0]
        parts.append(m), srcs.append(x)
        n_cols += len(x)
        s_iv.append(i), s_flip.append(int(flip[q]))
    o_off.append(n_cols)
    s_off.append(len(s_iv))
    n_out = len(o_left)
    if n_out == 0:
        o_off, s_off = [0], [0]
    out = dict(left=np.array(o_left, np.int64).reshape(n_out, N), right=np.array(o_right, np.int64).reshape(n_out, N),
               reverse=np.array(o_rev, np.int8).reshape(n_out, N), col_off=np.array(o_off, np.int64),
               cols=np.concatenate(parts + [np.zeros(0, np.uint32)]).astype(np.uint32), src_off=np.array(s_off, np.int64),
               src_iv=np.array(s_iv, np.int64), src_flip=np.array(s_flip, np.int8), src_col=np.concatenate(srcs + [np.zeros(0, np.int64)]).astype(np.int64),
               n_fill=n_fill)
    if compact:
        for k in ("left", "right", "reverse"):
            out[k] = np.ascontiguousarray(out[k][:, proj])
        c = np.zeros(len(out["cols"]), np.uint32)
        for k, g in enumerate(proj):
            c |= (out["cols"] >> np.uint32(g) & np.uint32(1)) << np.uint32(k)
        out["cols"] = c
    return out


ARRAYS = ("left", "right", "reverse", "col_off", "cols", "src_off", "src_iv", "src_flip", "src_col")


def same(got, want, names=ARRAYS):
    """the names in which two projections differ (arrays compared by shape, type and value)"""
    return [k for k in names if not (got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]


# the hand case of tests/test_project_cpu.py and tests/test_gpu_project.py: three genomes, four intervals.  Interval 0 is reversed in genome 0;
# intervals 1 and 2 are split by genome 2 alone (3 bases of genome 0 and none of genome 1 between them); interval 3 lacks genome 1.
HAND = dict(
    left=np.array([[1, 1, 30], [6, 6, 10], [12, 9, 40], [20, 0, 50]], np.int64),
    right=np.array([[4, 4, 34], [8, 8, 12], [14, 11, 42], [22, 0, 52]], np.int64),
    reverse=np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 0]], np.int8),
    col_off=np.array([0, 6, 10, 13, 17], np.int64),
    cols=np.array([7, 5, 6, 4, 3, 7,  7, 2, 5, 7,  7, 7, 7,  5, 5, 0, 5], np.uint32))
