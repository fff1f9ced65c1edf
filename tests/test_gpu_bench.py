"""bench.py's two kinds of run: a plain one prints the headline line and nothing beyond its timed steps; --full adds the side
measurements (wide fetch, device-resident pass, stage times, kernel profile and roofline, accuracy) and the other BASELINE configs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ("fetch_wide", "device_resident", "kernel_share_of_resident_pass", "lcb_extension_off", "backbone", "homology_pass", "c2", "c4", "c5")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--scale", "0.05", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _headline(line):
    assert line["metric"] == "aligned Mbp/s (seed+extend+DP)" and line["unit"] == "Mbp/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0


@pytest.mark.gpu
def test_plain_run_is_the_headline_only():
    line = _bench()
    _headline(line)
    assert line["full"] is False
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["accuracy_vs_truth"] is None
    assert line["stages_ms"] == {} and line["kernels_ms"] == {}
    assert not [k for k in SIDE if k in line]


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements():
    line = _bench("--full", "--no-cpu-baseline")
    _headline(line)
    assert line["full"] is True and line["cpu_baseline"] is None
    assert line["roofline"]["kernel"] and line["stages_ms"] and line["kernels_ms"]
    assert 0.0 < line["accuracy_vs_truth"]["sensitivity"] <= 1.0
    missing = [k for k in SIDE if k not in line]
    assert not missing, missing
    for leg in ("c2", "c4", "c5"):
        assert "error" not in line[leg] and line[leg]["value"] > 0, line[leg]
