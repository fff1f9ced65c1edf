"""The small-sort engine (mauvealigner_amd/csrc/small_sort.hpp): its standalone driver against std::stable_sort, and the
whole pipeline with the engine (default) and without it (MAUVE_SMALL_SORT=0, the tiled two-launch path), which must give
identical result arrays."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_small_sort_driver_matches_stable_sort(tmp_path):
    exe = str(tmp_path / "small_sort_test")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "small_sort_test.cpp"), "-o", exe], timeout=600)
    r = subprocess.run([exe, "check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]


def _dump(tmp_path, config, scale, small):
    out = str(tmp_path / ("%s_%s" % (config, "on" if small else "off")))
    env = dict(os.environ)
    if small:
        env.pop("MAUVE_SMALL_SORT", None)
    else:
        env["MAUVE_SMALL_SORT"] = "0"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                           "--config", config, "--scale", str(scale), "--no-cpu-baseline", "--no-secondary",
                           "--dump-outputs", out], env=env, cwd=ROOT, stdout=subprocess.DEVNULL, timeout=900)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("config,scale", [("C3", 0.2), ("C4", 0.05), ("C5", 0.05)])
def test_small_sort_engine_same_results(tmp_path, config, scale):
    on, off = _dump(tmp_path, config, scale, True), _dump(tmp_path, config, scale, False)
    names = sorted(os.listdir(off))
    assert names and names == sorted(os.listdir(on))
    for f in names:
        assert np.array_equal(np.load(os.path.join(on, f)), np.load(os.path.join(off, f))), f
