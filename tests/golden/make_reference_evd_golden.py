#!/usr/bin/env python3
"""Regenerates tests/golden/reference_evd.json: what the reference's own program src/evd.cpp, built from its source against include/
(the libMems / libGenome mirror), prints on the committed fixtures.  Per fixture the program runs in a directory that holds
alignjob.0/evolved.dat (the committed XMFA) and alignjob.0/evolved_seqs.fas (the fixture's genomes) as `evd 1`; the entry is keyed by the
digest of those two texts (tests/test_excursion_cpu.py::evd_inputs).

The reference source tree is not part of this repository.  Build first (libmauve_hip.so), then from the repo root:
    python tests/golden/make_reference_evd_golden.py <mauveAligner source tree>/src
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_excursion_cpu as TX  # noqa: E402


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "evd.cpp")):
        raise SystemExit(__doc__)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        exe = TX.build_evd(os.path.abspath(sys.argv[1]), td)
        for name in sorted(TX.TOTALS):
            out[TX.evd_inputs(name)[2]] = {"fixture": name, "stdout": TX.run_evd(exe, name, td)}
    with open(TX.GOLDEN_EVD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d fixtures)" % (TX.GOLDEN_EVD, len(out)))


if __name__ == "__main__":
    main()
