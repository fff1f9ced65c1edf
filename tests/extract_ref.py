"""numpy restatement of the column extraction: the expected value of every device answer in tests/test_gpu_extract.py,
pinned itself in tests/test_extract_cpu.py against the rows of the committed XMFA texts (written by the oracle's writer, not by this
file), against counts from a separate column walk, and against a scalar walk of its own.  Independent of the product (no import of it).

The alignment is what mauve_align_fetch describes (see tests/coord_ref.py, whose rule 1 gives the signed position of every cell); the
genomes are arrays of 0..3 codes, `invalid` per genome a boolean array (True = ambiguous base) or None."""
import numpy as np

from tests.coord_ref import CoordRef

LETTERS = np.frombuffer(b"ACGT", np.uint8)


class ExtractRef:
    def __init__(self, left, right, reverse, col_off, cols, genomes, invalid=None):
        self.R = CoordRef(left, right, reverse, col_off, cols)
        self.col_off, self.cols = self.R.col_off, np.asarray(cols, np.uint32)
        self.n_iv, self.N = self.R.n_iv, self.R.N
        self.genomes = [np.asarray(g, np.uint8) for g in genomes]
        self.invalid = [None if invalid is None or invalid[g] is None else np.asarray(invalid[g], bool) for g in range(self.N)]

    def cells(self, iv, col, keep):
        """cell rule: the letters of the columns (iv[j], col[j]) in the genomes of `keep` -> uint8 [len(keep), n]"""
        pos, _ = self.R.column_positions(iv, col)
        out = np.full((len(keep), len(iv)), ord("-"), np.uint8)
        for k, g in enumerate(keep):
            p = pos[:, g]
            here = np.flatnonzero(p)
            b = self.genomes[g][np.abs(p[here]) - 1]
            ch = LETTERS[np.where(p[here] < 0, 3 - b, b)]
            if self.invalid[g] is not None:
                ch = np.where(self.invalid[g][np.abs(p[here]) - 1], ord("N"), ch)
            out[k, here] = ch
        return out

    def extract(self, keep=None, require=0, drop_empty=False, polymorphic=False, ranges=None):
        """-> (rows uint8 [n_keep, n_sel], sel_iv, sel_col, range_off)"""
        keep = list(range(self.N)) if keep is None else [int(g) for g in keep]
        if ranges is None:
            r_iv, r_col, r_len = np.arange(self.n_iv, dtype=np.int64), np.zeros(self.n_iv, np.int64), np.diff(self.col_off)
        else:
            r_iv, r_col, r_len = (np.asarray(x, np.int64) for x in ranges)
        # the candidates: the columns of the ranges one after another
        r = np.repeat(np.arange(len(r_iv)), r_len)
        start = np.concatenate([[0], np.cumsum(r_len)]).astype(np.int64)
        iv = r_iv[r]
        col = r_col[r] + np.arange(len(r), dtype=np.int64) - start[r]
        m = self.cols[self.col_off[iv] + col]
        keepmask = np.uint32(sum(1 << g for g in keep))
        sel = (m & np.uint32(require)) == np.uint32(require)
        if drop_empty:
            sel &= (m & keepmask) != 0
        rows = self.cells(iv, col, keep)
        if polymorphic:
            seen = np.zeros(len(iv), np.uint32)
            for c in range(4):
                seen |= np.any(rows == LETTERS[c], axis=0).astype(np.uint32) << np.uint32(c)
            sel &= (seen & (seen - np.uint32(1))) != 0
        range_off = np.concatenate([[0], np.cumsum(sel)]).astype(np.int64)[start]
        return np.ascontiguousarray(rows[:, sel]), iv[sel], col[sel], range_off


def parse_xmfa(text, N):
    """the rows of an XMFA text -> per interval {genome: (left, right, reverse, row as uint8 array)}"""
    out, cur, g = [], {}, None
    for line in text.splitlines():
        if line.startswith("#") or not line:
            continue
        if line.startswith("="):
            out.append({k: (v[0], v[1], v[2], np.frombuffer("".join(v[3]).encode(), np.uint8)) for k, v in cur.items()})
            cur, g = {}, None
        elif line.startswith(">"):
            f = line[1:].split()
            g, ends = f[0].split(":")
            g = int(g) - 1
            assert 0 <= g < N
            le, re = ends.split("-")
            cur[g] = (int(le), int(re), f[1] == "-", [])
        else:
            cur[g][3].append(line)
    return out


def xmfa_matrix(text, N):
    """the unconditioned matrix an XMFA text spells: all genomes, every interval whole, a genome without an entry all '-'"""
    parts = []
    for iv in parse_xmfa(text, N):
        n = len(next(iter(iv.values()))[3])
        m = np.full((N, n), ord("-"), np.uint8)
        for g, (_, _, _, row) in iv.items():
            assert len(row) == n
            m[g] = row
        parts.append(m)
    return np.concatenate(parts, axis=1) if parts else np.zeros((N, 0), np.uint8)
