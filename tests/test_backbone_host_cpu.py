"""The host steps of the backbone stage and of the homology pass (csrc/backbone_host.hpp) without a GPU:
tests/cpp/backbone_host_test.cpp makes what the kernels would hand the host by a plain column walk, runs it through bb_sort_records,
bb_sweep, bb_query_slots and bb_tables, and the tables must equal the oracle's -- on the hand case and the six random alignments of the
GPU test (tests/backbone_cases.py), and once with the queries made unique from 8 on, the path no GPU test reaches.  The two chaining
loops of the homology pass are compared with a column-by-column evaluation inside the program.  A stand-alone program under the address
and undefined-behaviour sanitizers (the runtimes are linked into it).  Integers throughout: every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from tests import backbone_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = 1 << 62                                                # a threshold no case reaches: the query slots are used as laid out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("backbone_host") / "backbone_host_test")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I" + os.path.join(ROOT, "mauvealigner_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "backbone_host_test.cpp"), "-o", exe])
    return exe


def host_tables(exe, tmp_path, aln, island_gap, dedupe_above):
    """the program's tables of one alignment -> (dict like O.backbone's, query slots, queries made)"""
    left, right, rev, col_off, cols = aln
    left = np.ascontiguousarray(left, np.int64)
    src, dst = str(tmp_path / "aln.bin"), str(tmp_path / "tables.bin")
    with open(src, "wb") as f:
        np.array([left.shape[1], left.shape[0], island_gap, dedupe_above], np.int64).tofile(f)
        for a in (left, right, rev, col_off):
            np.ascontiguousarray(a, np.int64).tofile(f)
        np.ascontiguousarray(cols, np.uint32).tofile(f)
    r = subprocess.run([exe, "tables", src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
    words, out, at = np.fromfile(dst, np.int64), [], 0
    while at < len(words):
        n = int(words[at])
        out.append(words[at + 1:at + 1 + n])
        at += 1 + n
    assert len(out) == 8 and at == len(words)
    N, n = left.shape[1], len(out[1])
    t = dict(zip(BC.KEYS, out[1:]))
    t["seg_mask"] = t["seg_mask"].astype(np.uint32)
    t["seg_left"], t["seg_right"], t["islands"] = t["seg_left"].reshape(n, N), t["seg_right"].reshape(n, N), t["islands"].reshape(-1, 8)
    return t, int(out[0][0]), int(out[0][1])


def same(r, e):
    for k in BC.KEYS:
        assert r[k].shape == e[k].shape and r[k].dtype == e[k].dtype, (k, r[k].shape, e[k].shape)
        assert np.array_equal(r[k], e[k]), k


def test_hand_case(program, tmp_path):
    aln = BC.hand_case()
    for gap in (3, 5):
        t, slots, made = host_tables(program, tmp_path, aln, gap, OFF)
        same(t, O.backbone(*aln, island_gap=gap))
        assert made == slots
    t = host_tables(program, tmp_path, aln, 3, OFF)[0]
    assert t["seg_mask"].tolist() == [7, 5, 7] and t["islands"].tolist() == [[0, 0, 1, 0, 10, 14, 11, 15], [0, 1, 2, 2, 10, 14, -206, -210]]


@pytest.mark.parametrize("seed", range(6))
def test_random_alignments(program, tmp_path, seed):
    aln = BC.random_case(seed)
    t, slots, made = host_tables(program, tmp_path, aln, 20, OFF)
    same(t, O.backbone(*aln, island_gap=20))
    assert len(t["seg_iv"]) > 0 and len(t["islands"]) > 0 and made == slots


def test_unique_queries_equal_the_slots_as_laid_out(program, tmp_path):
    """dedupe_above = 8: the queries are sorted, made unique and every slot looked up -- the tables are those of the run with the threshold
    off, and the oracle's"""
    aln = BC.random_case(1)
    plain, slots, made = host_tables(program, tmp_path, aln, 3, OFF)
    uniq, slots_u, made_u = host_tables(program, tmp_path, aln, 3, 8)
    assert slots_u == slots == made and 8 < made_u < slots                      # the unique path was taken and had columns to merge
    same(uniq, plain)
    same(uniq, O.backbone(*aln, island_gap=3))


def test_homology_chaining(program):
    r = subprocess.run([program, "chains"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
