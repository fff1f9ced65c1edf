#!/usr/bin/env python3
"""Regenerates tests/golden/reference_project.json: what the reference's own program src/projectAndStrip.cpp, built from its source
against include/ (the libMems / libGenome mirror), writes for the committed fixture g4x3k_tree and the sequences 0 2.  The program runs
as `projectAndStrip in.xmfa out.xmfa 0 2` in a directory that holds the committed XMFA and the fixture's genomes as the FastA files the
XMFA names; the entry is keyed by the digest of those texts and the ids (tests/test_project_cpu.py::pas_inputs).  Only what the program
wrote is stored, nothing of the program.

The reference source tree is not part of this repository.  Build first (libmauve_hip.so), then from the repo root:
    python tests/golden/make_reference_project_golden.py <mauveAligner source tree>/src
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_project_cpu as TP  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "projectAndStrip.cpp")):
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as td:
        exe = TP.build_project_and_strip(os.path.abspath(sys.argv[1]), td)
        out = {TP.pas_inputs()[2]: {"fixture": TP.PAS_FIXTURE, "ids": list(TP.PAS_IDS), "xmfa": TP.run_project_and_strip(exe, td)}}
    with open(TP.GOLDEN_PROJECT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % TP.GOLDEN_PROJECT)


if __name__ == "__main__":
    main()
