"""CPU-side checks of the alignment text: the Python restatement of tests/text_ref.py, which is the expected value of the
GPU tests, against things it did not produce -- the committed XMFA texts (the oracle's writer), byte for byte, and MAF texts spelled out
here by hand -- the new entry points in the export list of the built library, and the mirror header in C++."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mauvealigner_amd import _lib
from tests.test_extract_cpu import COUNTS, GOLDEN, load
from tests.test_gpu_extract import HAND, HAND_GENOMES, _codes
from tests.text_ref import ContigJoin, TextRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mauve_default_text_params", "mauve_alignment_text", "mauve_alignment_text_fetch")
MAF_HEAD = "##maf version=1 program=progressiveMauve\n"


def ref_of(a, gs, invalid=None):
    return TextRef(a["left"], a["right"], a["reverse"], a["col_off"], a["cols"], gs, invalid)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_restatement_equals_the_golden_xmfa(name):
    a, gs = load(name)
    with open(os.path.join(GOLDEN, name + ".xmfa"), "rb") as f:
        want = f.read()
    text, boff = ref_of(a, gs).text("xmfa", names=["g%d" % g for g in range(len(gs))])
    assert text == want
    assert len(boff) == len(a["left"]) + 1 and boff[-1] == len(want) and text[:boff[0]].count(b"\n") == 1 + 3 * len(gs)
    for i in range(len(a["left"])):                               # block_off cuts at the "=" lines
        assert text[boff[i]:boff[i + 1]].startswith(b"> ") and text[boff[i]:boff[i + 1]].endswith(b"\n=\n")
        assert text[boff[i]:boff[i + 1]].count(b"=") == 1


def test_hand_maf():
    """the alignment of test_extract_hand_case: genome 0 forward 1..20 of 22 bases, genome 1 forward 101..115 of 115 (columns 10..14
    gapped), genome 2 reverse 201..220 of 223: its start is 223 - 220 = 3 on the other strand"""
    gs = [_codes(s) for s in HAND_GENOMES]
    T = ref_of(HAND, gs)
    text, boff = T.text("maf", names=["n0", "n1", "n2"])
    want = (MAF_HEAD + "a\n"
            "s n0 0 20 + 22 ACGTACGTACGTACGTACGT\n"
            "s n1 100 15 + 115 CCCCCGGGGG-----TTTTT\n"
            "s n2 3 20 - 223 TTACGTACGTAAAACCCGGT\n"
            "\n")
    assert text.decode() == want and boff.tolist() == [len(MAF_HEAD), len(want)]
    # a window: columns 8..13; genome 1 has residues in 8 and 9 only, genome 2's extent shrinks from the right (reverse strand)
    text, boff = T.text("maf", names=["n0", "n1", "n2"], ranges=([0], [8], [6]))
    want = (MAF_HEAD + "a\n"
            "s n0 8 6 + 22 ACGTAC\n"
            "s n1 108 2 + 115 GG----\n"
            "s n2 11 6 - 223 GTAAAA\n"
            "\n")
    assert text.decode() == want
    # the same window as XMFA, wrapped at 4
    text, boff = T.text("xmfa", names=["n0", None, "n2"], deflines=["d0", "d1", ""], ranges=([0], [8], [6]), wrap=4)
    head = "#FormatVersion Mauve1\n" + "".join("#Sequence%dFile\t%s\n#Sequence%dEntry\t%d\n#Sequence%dFormat\tFastA\n" % (g + 1, n, g + 1, g + 1, g + 1)
                                               for g, n in enumerate(["n0", "", "n2"]))
    want = head + "> 1:9-14 + d0\nACGT\nAC\n> 2:109-110 + d1\nGG--\n--\n> 3:207-212 - \nGTAA\nAA\n=\n"
    assert text.decode() == want and boff.tolist() == [len(head), len(want)]


def test_two_contig_maf():
    """genome 0 = contigs of 10 and 12 bases, genome 1 = 100 and 15, genome 2 = 200 and 23: the whole interval crosses the join of genome 0;
    split at column 10 every row lies in one contig, with contig-local coordinates and the contig's length"""
    gs = [_codes(s) for s in HAND_GENOMES]
    T = ref_of(HAND, gs)
    contigs = [[0, 10], [0, 100], [0, 200]]
    cn = [["a", "b"], ["c", "d"], ["e", "f"]]
    with pytest.raises(ContigJoin) as ei:
        T.text("maf", names=["n0", "n1", "n2"], contigs=contigs, contig_names=cn)
    assert (ei.value.range, ei.value.genome) == (0, 0)
    text, boff = T.text("maf", names=["n0", "n1", "n2"], contigs=contigs, contig_names=cn, ranges=([0, 0], [0, 10], [10, 10]))
    b0 = ("a\n"
          "s n0.a 0 10 + 10 ACGTACGTAC\n"
          "s n1.d 0 10 + 15 CCCCCGGGGG\n"
          "s n2.f 3 10 - 23 TTACGTACGT\n"
          "\n")
    b1 = ("a\n"
          "s n0.b 0 10 + 12 GTACGTACGT\n"
          "s n1.d 10 5 + 15 -----TTTTT\n"
          "s n2.f 13 10 - 23 AAAACCCGGT\n"
          "\n")
    assert text.decode() == MAF_HEAD + b0 + b1
    assert boff.tolist() == [len(MAF_HEAD), len(MAF_HEAD) + len(b0), len(MAF_HEAD) + len(b0) + len(b1)]
    # without contig names the source is the genome's name alone
    text, _ = T.text("maf", names=["n0", "n1", "n2"], contigs=contigs, ranges=([0], [10], [10]))
    assert text.decode() == MAF_HEAD + b1.replace("n0.b", "n0").replace("n1.d", "n1").replace("n2.f", "n2")


def test_blocks_without_rows_and_repeated_ranges():
    gs = [_codes(s) for s in HAND_GENOMES]
    T = ref_of(HAND, gs)
    # columns 10..14 of genome 1 alone would be a block without a row; with all genomes the row of genome 1 is left out
    text, boff = T.text("maf", names=["x", "y", "z"], ranges=([0, 0, 0, 0], [10, 3, 10, 20], [5, 0, 5, 0]))
    blk = "a\ns x 10 5 + 22 GTACG\ns z 13 5 - 223 AAAAC\n\n"
    assert text.decode() == MAF_HEAD + blk + blk
    assert boff.tolist() == [41, 41 + len(blk), 41 + len(blk), 41 + 2 * len(blk), 41 + 2 * len(blk)]
    text, boff = T.text("xmfa", ranges=(np.zeros(0, np.int64),) * 3)
    assert text.count(b"\n") == 10 and boff.tolist() == [len(text)]


def test_new_entry_points_are_exported_and_defaults():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    L.mauve_default_text_params.restype = None
    for fmt, wrap in ((_lib.TEXT_XMFA, 80), (_lib.TEXT_MAF, 0)):
        p = _lib.TextParams()
        L.mauve_default_text_params(fmt, C.byref(p))
        assert (p.format, p.wrap) == (fmt, wrap)
    assert C.sizeof(_lib.TextParams) == 8


def test_mirror_header_compiles():
    """include/libMems/AlignmentText.h through tests/cpp/text_mirror_test.cpp (the GPU suite builds and runs it)"""
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "text_mirror_test.cpp")])
