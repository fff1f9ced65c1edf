"""Plain Python restatement of the alignment text (rules 1-6): the expected value of every device answer in
tests/test_gpu_text.py, pinned itself in tests/test_text_cpu.py against the committed XMFA texts (written by the oracle's writer, not by
this file) and against MAF texts spelled out by hand.  Independent of the product (no import of it).  The letters are ExtractRef.cells
(tests/extract_ref.py); the extents come from counts of the column bits."""
import numpy as np

from tests.extract_ref import ExtractRef


class ContigJoin(ValueError):
    """a MAF row whose ends lie in different contigs: .range, .genome"""

    def __init__(self, r, g):
        ValueError.__init__(self, "range %d, genome %d: the row crosses a contig join" % (r, g))
        self.range, self.genome = r, g


class TextRef:
    def __init__(self, left, right, reverse, col_off, cols, genomes, invalid=None):
        self.E = ExtractRef(left, right, reverse, col_off, cols, genomes, invalid)
        self.left, self.right, self.reverse = (np.asarray(x) for x in (left, right, reverse))
        self.col_off = np.asarray(col_off, np.int64)
        self.n_iv, self.N = self.E.n_iv, self.E.N
        self.lens = [len(g) for g in genomes]
        cols = np.asarray(cols, np.uint32)
        # residues of genome g in front of column x of the whole array
        self.cum = [np.concatenate([[0], np.cumsum((cols >> np.uint32(g)) & np.uint32(1))]).astype(np.int64) for g in range(self.N)]

    def rows(self, i, c, l):
        """rule 2: the rows of block (i, c, l) -> [(g, lo, hi, reverse, cells as bytes)]"""
        x = int(self.col_off[i]) + c
        cells = self.E.cells(np.full(l, i, np.int64), c + np.arange(l, dtype=np.int64), list(range(self.N))) if l else None
        out = []
        for g in range(self.N):
            if not self.left[i, g]:
                continue
            base = int(self.cum[g][self.col_off[i]])
            k0, k1 = int(self.cum[g][x]) - base, int(self.cum[g][x + l]) - base
            if k1 <= k0:
                continue
            rev = bool(self.reverse[i, g])
            le, ri = int(self.left[i, g]), int(self.right[i, g])
            lo, hi = (ri - k1 + 1, ri - k0) if rev else (le + k0, le + k1 - 1)
            out.append((g, lo, hi, rev, cells[g].tobytes()))
        return out

    def text(self, fmt="xmfa", names=None, deflines=None, contigs=None, contig_names=None, ranges=None, wrap=None):
        """-> (the text as bytes, block_off int64 [n_range + 1]); ContigJoin for a MAF row across a join"""
        N = self.N
        nm = ["" if names is None or names[g] is None else names[g] for g in range(N)]
        df = nm if deflines is None else ["" if deflines[g] is None else deflines[g] for g in range(N)]
        if ranges is None:
            ranges = (np.arange(self.n_iv), np.zeros(self.n_iv, np.int64), np.diff(self.col_off))
        r_iv, r_col, r_len = ([int(v) for v in x] for x in ranges)
        if fmt == "xmfa":
            wrap = 80 if wrap is None else wrap
            assert wrap >= 1
            parts = ["#FormatVersion Mauve1\n"]
            for g in range(N):
                parts.append("#Sequence%dFile\t%s\n#Sequence%dEntry\t%d\n#Sequence%dFormat\tFastA\n" % (g + 1, nm[g], g + 1, g + 1, g + 1))
        else:
            assert fmt == "maf" and not wrap
            parts = ["##maf version=1 program=progressiveMauve\n"]
            starts = [[0] if contigs is None else [int(s) for s in contigs[g]] for g in range(N)]
        out = ["".join(parts).encode()]
        size = len(out[0])
        block_off = [size]
        for r, (i, c, l) in enumerate(zip(r_iv, r_col, r_len)):
            blk = []
            for g, lo, hi, rev, cells in self.rows(i, c, l):
                if fmt == "xmfa":
                    blk.append(("> %d:%d-%d %s %s\n" % (g + 1, lo, hi, "-" if rev else "+", df[g])).encode())
                    for at in range(0, l, wrap):
                        blk.append(cells[at:at + wrap] + b"\n")
                else:
                    st = starts[g]
                    k = max(q for q in range(len(st)) if st[q] <= lo - 1)
                    end = st[k + 1] if k + 1 < len(st) else self.lens[g]
                    if hi > end:
                        raise ContigJoin(r, g)
                    lo_local, n, src_size = lo - st[k], hi - lo + 1, end - st[k]
                    start = src_size - lo_local - n + 1 if rev else lo_local - 1
                    src = nm[g] if contig_names is None else "%s.%s" % (nm[g], "" if contig_names[g][k] is None else contig_names[g][k])
                    blk.append(("s %s %d %d %s %d " % (src, start, n, "-" if rev else "+", src_size)).encode() + cells + b"\n")
            if blk:
                blk = ([b"a\n"] if fmt == "maf" else []) + blk + [b"\n" if fmt == "maf" else b"=\n"]
                out += blk
                size += sum(len(b) for b in blk)
            block_off.append(size)
        return b"".join(out), np.array(block_off, np.int64)
