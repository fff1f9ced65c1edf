"""The tile order of the tiled sort (mauvealigner_amd/csrc/tile_swz.hpp) on the host: tests/cpp/swz_host_test.cpp, plain g++, once as it is
and once as a stand-alone program under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "swz_host_test.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_swz_is_a_contiguous_permutation(tmp_path, flags):
    exe = str(tmp_path / "swz_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok 4202 tile counts"), r.stdout[-2000:] + r.stderr[-2000:]
