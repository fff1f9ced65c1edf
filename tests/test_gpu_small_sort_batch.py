"""The batched small sort (small_sort_batch, mauvealigner_amd/csrc/small_sort.hpp): S sorts of n pairs each in one set of
launches, as the chain stage makes the orders of all genomes.  Its standalone driver compares every segment with
std::stable_sort of that segment alone over S x n x key_bits x key pattern (ragged tiles, the tile-class edges, one to four
passes, both result parities) and checks the sentinel words around and between the segments."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_small_sort_batch_driver_matches_stable_sort(tmp_path):
    exe = str(tmp_path / "small_sort_batch_test")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-pthread", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "small_sort_batch_test.cpp"), "-o", exe], timeout=600)
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok 528 cases"), r.stdout[-4000:] + r.stderr[-2000:]
