"""Cost of the excursions of the column scores on the GPU.  Prints ONE JSON line: C3 at full size aligned with defaults,
indexed on the device (mauve_coord_index).  After a warm-up round, `reps` rounds each of

  pairs_all   mauve_excursions_pairs for all pairs a < b (ten at C3), every interval whole
  pairs_one   ... for the pair (0, 1)
  core_all    mauve_excursions_core for the group of every genome

as wall time of the call (it ends in a stream synchronise) with the median and the spread (min, max) in milliseconds, then one profiled
call of each (mauve_profile_enable: every launch timed on its own with HIP events) with, per launch class, the time, the bytes it has to
read and write, and the resulting fraction of the HBM roofline.  The bytes are counted from the algorithm, not measured: per column and
genome a walk reads the index record (64 bytes per 448 columns) and the packed bases (a quarter byte per residue), per (set, chunk) its
64-bit words of the element arrays; a record is 16 bytes.

For comparison the host loop of tests/cpp/excursion_test.cpp (getLocalRecordHeights of evd.cpp over GetAlignment rows, single-threaded)
is built and timed on the same alignment, written out as an XMFA; --no-host skips it.

usage: python tools/excursion_time.py [--reps R] [--config C3] [--scale S] [--no-host]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mauvealigner_amd import _lib, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X: HBM3E 8 TB/s spec (bench.py)
CLASSES = ("exc_maps", "exc_scan", "exc_count", "exc_write")


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def algorithmic_bytes(n_cols, n_need, n_el, n_stream, n_exc):
    """bytes per launch class of one call: n_need genomes named by the sets, n_el = sets x chunks elements"""
    cells = n_cols * n_need * (64 / 448 + 0.25)
    return {"exc_maps": cells + 16 * n_el,                      # the two words of the map out
            "exc_scan": 2 * ((16 + 16 + 8) * n_el) + 24 * n_stream + 16 * n_stream,     # two scans: read twice, write once; the streams' counts
            "exc_count": cells + (8 + 16) * n_el,
            "exc_write": cells + 24 * n_el + 16 * n_exc}


def host_loop_ms(a, gs):
    """tests/cpp/excursion_test.cpp --time on the alignment -> the milliseconds its host loop over all pairs took"""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "excursion_test")
        lib = os.path.join(ROOT, "mauvealigner_amd")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "excursion_test.cpp"),
                               "-o", exe, "-L" + lib, "-lmauve_hip", "-Wl,-rpath," + lib])
        xmfa, mfa = os.path.join(td, "a.xmfa"), os.path.join(td, "g.mfa")
        with open(xmfa, "w") as f:
            f.write(a["xmfa"])
        with open(mfa, "w") as f:
            for g, s in enumerate(gs):
                f.write(">g%d\n%s\n" % (g, synth.to_ascii(s).decode()))
        r = subprocess.run([exe, xmfa, mfa, "--time"], capture_output=True, text=True)        # a fresh process with a context of its own
        if r.returncode or not r.stdout.strip().endswith("OK"):
            raise RuntimeError("excursion_test failed: " + r.stdout + r.stderr)
        m = re.search(r"host loop, all pairs: ([\d.]+) ms; device call and fetch: ([\d.]+) ms", r.stdout)
        return float(m.group(1)), float(m.group(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    try:
        gs = synth.make_config(a.config, scale=a.scale)
        N = len(gs)
        ctx.set_genomes(gs)
        aln = ctx.align(_lib.default_params(), want_xmfa=not a.no_host)
        ctx.coord_index()
        n_iv, n_cols = int(len(aln["left"])), int(len(aln["cols"]))
        lens = np.diff(aln["col_off"])
        gs0 = aln["col_off"][:-1]
        units = np.where(lens > 0, ((gs0 + lens - 1) >> 6) - (gs0 >> 6) + 1, 0)
        n_chunks = int(np.sum((units + _lib.EXCURSION_CHUNK // 64 - 1) // (_lib.EXCURSION_CHUNK // 64)))
        runs = {"pairs_all": (lambda: ctx.excursions_pairs(), N * (N - 1) // 2, N),
                "pairs_one": (lambda: ctx.excursions_pairs(([0], [1])), 1, 2),
                "core_all": (lambda: ctx.excursions_core(), 1, N)}
        out = {"workload": a.config, "scale": a.scale, "device": ctx.device_name(), "nseq": N, "n_iv": n_iv, "n_cols": n_cols, "n_chunks": n_chunks,
               "chunk": _lib.EXCURSION_CHUNK, "reps": a.reps, "hbm_peak_gbs": HBM_PEAK_GBS}
        for name, (call, n_set, n_need) in runs.items():
            ms = []
            for rnd in range(a.reps + 1):                        # round 0 warms up: code objects, buffer growth
                t0 = time.perf_counter()
                n_exc = call()
                if rnd:
                    ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            ctx.excursions_fetch(want=(True, False, False, False))
            fetch_ms = (time.perf_counter() - t0) * 1e3
            ctx.profile(True)
            ctx.profile_reset()
            call()
            ctx.profile(False)
            prof = ctx.profile_get()
            need = algorithmic_bytes(n_cols, n_need, n_set * n_chunks, n_set * n_iv, n_exc)
            launches = {}
            for k in CLASSES:
                p = prof[k]
                gbs = need[k] / (p["ms"] * 1e-3) / 1e9 if p["ms"] else None
                launches[k] = {"ms": round(p["ms"], 4), "launches": p["launches"], "bytes": int(need[k]), "gb_per_s": round(gbs, 1) if gbs else None,
                               "hbm_frac": round(gbs / HBM_PEAK_GBS, 5) if gbs else None}
            out[name] = {"sets": n_set, "n_exc": int(n_exc), "call_ms": spread(ms), "fetch_heights_ms": round(fetch_ms, 3), "launches": launches,
                         "kernels_ms": round(sum(v["ms"] for v in launches.values()), 4)}
        if not a.no_host:
            host, dev = host_loop_ms(aln, gs)
            out["host_loop_all_pairs_ms"] = host
            out["mirror_device_call_and_fetch_ms"] = dev
        print(json.dumps(out), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
