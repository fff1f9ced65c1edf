"""numpy restatement of the coordinate translation rules: the expected value of every device answer in
tests/test_gpu_coord.py, pinned itself against a column-by-column walk in tests/test_coord_cpu.py.  Independent of the product
(no import of it): a cumulative sum of the per-genome bit columns, and searchsorted for the interval and for the column.

The alignment is what mauve_align_fetch describes: left/right/reverse [n_iv, nseq], col_off [n_iv + 1], one presence mask per column.
Genome g is present in interval i iff left[i, g] != 0; its residue with ordinal k in column order sits at left + k, at right - k on
the reverse strand, and is reported signed (negative = reverse strand)."""
import numpy as np


class CoordRef:
    def __init__(self, left, right, reverse, col_off, cols):
        self.left, self.right = np.asarray(left, np.int64), np.asarray(right, np.int64)
        self.rev = np.asarray(reverse) != 0
        self.col_off = np.asarray(col_off, np.int64)
        self.n_iv, self.N = self.left.shape
        cols = np.asarray(cols, np.uint32)
        self.bits = (cols[:, None] >> np.arange(self.N, dtype=np.uint32) & 1).astype(bool)          # [n_cols, nseq]
        self.cum = np.zeros((len(cols) + 1, self.N), np.int64)                                       # residues of g in columns [0, x)
        np.cumsum(self.bits, axis=0, out=self.cum[1:])
        self.by_left = []                                                                            # per genome: its intervals by left end
        for g in range(self.N):
            iv = np.flatnonzero(self.left[:, g])
            self.by_left.append(iv[np.argsort(self.left[iv, g], kind="stable")])

    def _signed(self, iv, k):
        """signed position of the residue with ordinal k[q, g] of every genome in interval iv[q]"""
        return np.where(self.rev[iv], -(self.right[iv] - k), self.left[iv] + k)

    def column_positions(self, iv, col, nearest=False):
        """rule 1: (interval, column) -> pos[n, nseq], defined[n]"""
        iv, col = np.asarray(iv, np.int64), np.asarray(col, np.int64)
        x = self.col_off[iv] + col
        r = self.cum[x] - self.cum[self.col_off[iv]]                     # residues of the interval in front of the column
        present = self.left[iv] != 0
        here = self.bits[x] & present
        k = np.where(here, r, np.maximum(r - 1, 0))                      # gapped: the residue before the column, else the first one
        pos = np.where(here | (present & bool(nearest)), self._signed(iv, k), 0)
        defined = (here.astype(np.uint64) << np.arange(self.N, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
        return pos, defined

    def seqpos_to_column(self, seq, pos):
        """rule 2: (genome, 1-based position) -> (interval, column in it), (-1, -1) where no interval covers the base"""
        seq, pos = np.asarray(seq, np.int64), np.asarray(pos, np.int64)
        iv, col = np.full(len(seq), -1, np.int64), np.full(len(seq), -1, np.int64)
        for g in np.unique(seq):
            t, q = self.by_left[g], np.flatnonzero(seq == g)
            if len(t) == 0:
                continue
            e = np.searchsorted(self.left[t, g], pos[q], side="right") - 1             # the last interval that starts at or before the base
            i = t[np.maximum(e, 0)]
            hit = (e >= 0) & (pos[q] <= self.right[i, g])
            q, i, p = q[hit], i[hit], pos[q][hit]
            k = np.where(self.rev[i, g], self.right[i, g] - p, p - self.left[i, g])     # its ordinal in column order
            x = np.searchsorted(self.cum[1:, g], self.cum[self.col_off[i], g] + k, side="right")   # the first column with more than that many in front of its end
            iv[q], col[q] = i, x - self.col_off[i]
        return iv, col

    def translate_positions(self, seq, pos, nearest=False):
        """rule 3: rule 2, then rule 1 at that column -> out[n, nseq], defined[n], interval[n]"""
        iv, col = self.seqpos_to_column(seq, pos)
        out, defined = np.zeros((len(iv), self.N), np.int64), np.zeros(len(iv), np.uint32)
        hit = iv >= 0
        out[hit], defined[hit] = self.column_positions(iv[hit], col[hit], nearest)
        return out, defined, iv

    def covered(self, g, length):
        """per base 1..length of genome g: does some [left, right] hold it?  (the definition rule 2's -1 is checked against)"""
        c = np.zeros(length + 2, np.int64)
        for i in np.flatnonzero(self.left[:, g]):
            c[self.left[i, g]] += 1
            c[self.right[i, g] + 1] -= 1
        return np.cumsum(c)[1:length + 1] > 0
