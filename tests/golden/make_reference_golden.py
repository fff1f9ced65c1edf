#!/usr/bin/env python3
"""Regenerates tests/golden/reference_tools.json: what two of the reference's own programs, built from their sources
against include/ (the libMems / libGenome mirror), print and write on the inputs the tests give them.

  score_alignment  -- src/scoreAlignment.cpp <truth XMFA> <oracle XMFA> on the cases of tests/test_accuracy.py
                      (stdout, and the digests of the two files)
  mfa2xmfa         -- src/mfa2xmfa.cpp in.mfa out.xmfa un.fa on the multi-FastA of
                      tests/test_compat_headers.py::test_reference_mfa2xmfa_runs_on_the_mirror (both files it writes)
  mfa2xmfa_blocks  -- src/mfa2xmfa.cpp b.mfa b.xmfa on every all-forward block of the oracle alignment of
                      test_oracle_xmfa_blocks_equal_what_mfa2xmfa_writes (keyed by the digest of the multi-FastA)

The reference source tree is not part of this repository.  Build first (libmauve_hip.so), then from the repo root:
    python tests/golden/make_reference_golden.py <mauveAligner source tree>/src
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_accuracy as TA  # noqa: E402
from tests import test_compat_headers as TC  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_tools.json")


def build_tool(src_dir, name, td, link_lib):
    exe = os.path.join(td, name)
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(src_dir, name + ".cpp"), "-o", exe]
    if link_lib:
        lib = os.path.join(ROOT, "mauvealigner_amd")
        cmd += ["-L" + lib, "-lmauve_hip", "-Wl,-rpath," + lib]
    subprocess.check_call(cmd)
    return exe


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "scoreAlignment.cpp")):
        raise SystemExit(__doc__)
    src = os.path.abspath(sys.argv[1])
    out = {}
    with tempfile.TemporaryDirectory() as td:
        score = build_tool(src, "scoreAlignment", td, True)
        mfa2xmfa = build_tool(src, "mfa2xmfa", td, False)

        cases = []
        for case in TA.SCORE_CASES:
            t, c, _, _ = TA.score_case(*case)
            tp, cp = os.path.join(td, "t.xmfa"), os.path.join(td, "c.xmfa")
            with open(tp, "w") as f:
                f.write(t)
            with open(cp, "w") as f:
                f.write(c)
            stdout = subprocess.run([score, tp, cp], capture_output=True, text=True, check=True).stdout
            cases.append({"case": list(case), "truth_sha256": TA.sha256(t), "calculated_sha256": TA.sha256(c), "stdout": stdout})
        out["score_alignment"] = cases

        run = os.path.join(td, "run")
        os.mkdir(run)
        mfa = TC.mfa2xmfa_input(TC.mfa2xmfa_rows())
        with open(os.path.join(run, "in.mfa"), "w") as f:
            f.write(mfa)
        subprocess.check_call([mfa2xmfa, "in.mfa", "out.xmfa", "un.fa"], cwd=run)
        with open(os.path.join(run, "out.xmfa")) as f, open(os.path.join(run, "un.fa")) as g:
            out["mfa2xmfa"] = {"input_sha256": TC._sha256(mfa), "xmfa": f.read(), "fa": g.read()}

        blocks = {}
        for _, mfa, _ in TC.oracle_xmfa_blocks():
            with open(os.path.join(run, "b.mfa"), "w") as f:
                f.write(mfa)
            subprocess.check_call([mfa2xmfa, "b.mfa", "b.xmfa"], cwd=run)
            with open(os.path.join(run, "b.xmfa")) as f:
                blocks[TC._sha256(mfa)] = f.read()
        out["mfa2xmfa_blocks"] = blocks

    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d scoreAlignment cases, %d mfa2xmfa blocks, %d bytes" % (OUT, len(cases), len(blocks), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
